"""--save_replay / --offline_replay without a device: the command line and its refusals, ReplayMemory.peek on a file
written by a host-only stand-in of the header, main's comparison of the header with the run's flags, Agent.train_offline's schedule of
learns, target refreshes and library calls on stand-in objects, and Statistics' row of a phase without an environment step."""
import csv
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from simple_dqn_amd import main  # noqa: E402
from simple_dqn_amd.agent import Agent, priority_beta  # noqa: E402
from simple_dqn_amd.replay_memory import ReplayMemory  # noqa: E402
from simple_dqn_amd.statistics import Statistics  # noqa: E402
from util import make_args  # noqa: E402


def _write_header(path, size=2000, count=500, current=500, H=84, W=84, hist=4, magic=b"SDQNRING1\n", words=6):
    """what ReplayMemory.save writes in front of the ring, and nothing behind it"""
    with open(path, "wb") as f:
        f.write(magic)
        np.array([size, count, current, H, W, hist][:words], dtype=np.int64).tofile(f)
    return str(path)


def test_parser_defaults_and_refusals_before_any_device_call(tmp_path):
    d = main.build_parser().parse_args([])
    assert d.save_replay is None and d.offline_replay is None
    assert main.check_offline(d) == (None, None)
    assert main.check_offline(main.build_parser().parse_args(["--save_replay", "x.ring"])) == ("x.ring", None)
    assert main.check_offline(main.build_parser().parse_args(["--offline_replay", "x.ring", "--eval_envs", "32", "--cql_alpha", "1"])) == (None, "x.ring")
    ring = _write_header(tmp_path / "d.ring")
    base = ["--environment", "catch", "--replay_size", "2000", "--batch_size", "32", "--epochs", "0"]
    for extra, words in ((["--save_replay", "x.ring", "--train_envs", "4"], ("--save_replay", "--train_envs")),
                         (["--offline_replay", ring, "--train_envs", "4"], ("--offline_replay", "--train_envs")),
                         (["--offline_replay", ring, "--play_games", "1"], ("--offline_replay", "--play_games")),
                         (["--offline_replay", ring, "--save_replay", "y.ring"], ("--offline_replay", "--save_replay"))):
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:
            main.check_offline(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never this ValueError
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))


def test_peek_reads_the_header_alone(tmp_path):
    p = _write_header(tmp_path / "a.ring", size=1234, count=77, current=78, H=64, W=48, hist=2)
    assert ReplayMemory.peek(p) == dict(size=1234, count=77, current=78, H=64, W=48, hist=2)
    with pytest.raises(ValueError) as ei:
        ReplayMemory.peek(_write_header(tmp_path / "b.ring", magic=b"NOTARING1\n"))
    assert "b.ring" in str(ei.value)
    with pytest.raises(ValueError):
        ReplayMemory.peek(_write_header(tmp_path / "c.ring", words=4))


@pytest.mark.parametrize("field,flag,theirs,ours", [("size", "--replay_size", 2000, 3000), ("H", "--screen_height", 64, 84),
                                                    ("W", "--screen_width", 48, 84), ("hist", "--history_length", 2, 4)])
def test_a_mismatched_dataset_is_refused_naming_both_values(tmp_path, field, flag, theirs, ours):
    kw = dict(size=3000, H=84, W=84, hist=4)
    kw[field] = theirs
    p = _write_header(tmp_path / "m.ring", **kw)
    args = main.build_parser().parse_args(["--environment", "catch", "--replay_size", "3000", "--offline_replay", p, "--epochs", "0"])
    for call in (lambda: main.check_offline_file(args, p), lambda: main.run(args)):      # (run: before the memory is allocated, before any device call)
        with pytest.raises(ValueError) as ei:
            call()
        msg = str(ei.value)
        assert flag in msg and str(theirs) in msg and str(ours) in msg, msg
    ok = _write_header(tmp_path / "ok.ring", size=3000)
    assert main.check_offline_file(args, ok)["count"] == 500


class _Env:
    def numActions(self):
        return 3


class _Net:
    """records what the agent asks of it"""
    def __init__(self):
        self.log, self.callback, self.train_iterations = [], None, 0

    def update_target_network(self):
        self.log.append(("target",))

    def set_epoch(self, epoch):
        pass

    def train_from_memory(self, mem, n):
        self.log.append(("train", n, mem.beta))
        self.train_iterations += n


class _Mem:
    _h, batch_size, count, beta = object(), 32, 1000, None

    def __init__(self, prioritized=False):
        self.prioritized = prioritized

    def can_sample(self):
        return self.count > self.batch_size

    def set_priority_beta(self, beta):
        self.beta = beta


def _agent(chunk=None, per=False, **kw):
    args = make_args(priority_beta=0.4, priority_beta_steps=100, **kw)
    net, mem = _Net(), _Mem(per)
    agent = Agent(_Env(), mem, net, args) if chunk is None else Agent(_Env(), mem, net, args, offline_chunk=chunk)
    return agent, net, mem


def _replay(log, repeat):
    """(learn numbers before which the target was refreshed, sizes of the library calls in learns)"""
    t, refreshed, calls = 0, [], []
    for ev in log:
        if ev[0] == "target":
            refreshed.append(t)
        else:
            assert ev[1] % repeat == 0
            calls.append(ev[1] // repeat)
            t += ev[1] // repeat
    return refreshed, calls


def test_train_offline_default_chunk_is_64():
    agent, net, _ = _agent(target_steps=10000)
    assert agent.offline_chunk == 64
    agent.train_offline(200)
    assert _replay(net.log, 1) == ([0], [64, 64, 64, 8]) and agent.total_train_steps == 200


@pytest.mark.parametrize("chunk", [1, 7, 64])
@pytest.mark.parametrize("repeat", [1, 2])
def test_train_offline_refreshes_where_the_rule_says_and_chunks_between(chunk, repeat):
    agent, net, _ = _agent(chunk, target_steps=50, train_repeat=repeat)
    agent.train_offline(120, 0)
    agent.train_offline(45, 1)                                    # a second epoch goes on counting: the next refresh is before learn 150
    refreshed, calls = _replay(net.log, repeat)
    assert refreshed == [0, 50, 100, 150] and sum(calls) == 165 and max(calls) <= chunk and agent.total_train_steps == 165
    # no call spans a refresh, and between two refreshes the calls are as large as the chunk allows
    t = 0
    for k in calls:
        assert all((t + i) % 50 for i in range(1, k))
        edge = min(50 - t % 50, 120 - t if t < 120 else 165 - t)
        assert k == min(chunk, edge), (t, k, edge)
        t += k


def test_train_offline_with_target_tau_copies_once_and_without_target_never():
    agent, net, _ = _agent(16, target_steps=50, target_tau=0.01)
    agent.train_offline(120)
    agent.train_offline(30, 1)
    assert _replay(net.log, 1)[0] == [0] and _replay(net.log, 1)[1] == [16] * 7 + [8] + [16, 14]
    agent, net, _ = _agent(16, target_steps=0)
    agent.train_offline(40)
    assert _replay(net.log, 1) == ([], [16, 16, 8])


def test_train_offline_sets_beta_once_per_chunk_from_its_first_learn():
    agent, net, mem = _agent(30, per=True, target_steps=50)
    agent.train_offline(100)
    t = 0
    for ev in net.log:
        if ev[0] == "train":
            assert ev[2] == priority_beta(0.4, 100, t), (t, ev)
            t += ev[1]
    assert [ev[1] for ev in net.log if ev[0] == "train"] == [30, 20, 30, 20]


def test_train_offline_refuses_an_empty_memory():
    agent, net, mem = _agent()
    mem.count = 10
    with pytest.raises(ValueError):
        agent.train_offline(5)
    assert net.log == []


def test_statistics_writes_a_phase_without_environment_steps(tmp_path):
    """zero games and zero steps: the train row of an offline epoch.  Sixteen columns as ever, no division by zero, nr_games 0"""
    class _SNet:
        train_iterations, callback = 0, None

        def predict(self, states):
            return np.zeros((states.shape[0], 3), np.float32)

    class _SMem:
        count, batch_size = 100, 8

        def getMinibatch(self):
            return np.zeros((8, 4, 84, 84), np.uint8), None, None, None, None

    class _SAgent:
        callback, total_train_steps = None, 300

    p = str(tmp_path / "s.csv")
    net = _SNet()
    st = Statistics(_SAgent(), net, _SMem(), None, make_args(csv_file=p))
    st.reset()
    for i, c in enumerate([2.0, 4.0]):
        net.train_iterations = i + 1
        st.on_train(c)
    st.write(1, "train")
    st.close()
    rows = list(csv.reader(open(p)))
    assert len(rows[0]) == 16 and len(rows[1]) == 16
    assert rows[1][:7] == ["1", "train", "0", "0", "0", "0", "0"] and rows[1][8] == "300" and float(rows[1][11]) == 3.0
    assert float(rows[1][15]) == 0.0
