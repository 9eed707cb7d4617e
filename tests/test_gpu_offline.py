"""--save_replay / --offline_replay / Agent.train_offline on the GPU: a dataset written by ReplayMemory.save trains
through main.run without an environment step; the chunk size of the library calls does not change a bit of the result on a uniform
memory; the target net is refreshed at the learns the rule names; a dataset of another size is refused; and the CQL regulariser holds
the value of an action the dataset never took below the values of those it did."""
import csv
import random

import numpy as np
import pytest

from util import make_args

pytestmark = pytest.mark.gpu

SIZE = 2000


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _catch_args(**kw):
    base = dict(environment="catch", catch_balls=10, batch_size=32, replay_size=SIZE, random_starts=8, random_seed=5)
    base.update(kw)
    return make_args(**base)


@pytest.fixture(scope="module")
def dataset(sd, tmp_path_factory):
    """2 000 slots of random play on catch, written by ReplayMemory.save"""
    args = _catch_args()
    random.seed(5)
    env, mem, net = sd.CatchEnvironment(args, seed=5), sd.ReplayMemory(SIZE, args), sd.DeepQNetwork(3, args)
    sd.Agent(env, mem, net, args).play_random(SIZE + 100)
    path = str(tmp_path_factory.mktemp("offline") / "catch.ring")
    mem.save(path)
    assert sd.ReplayMemory.peek(path) == dict(size=SIZE, count=SIZE, current=100, H=84, W=84, hist=4)
    return path


def _argv(path, tmp, *extra):
    return ["--environment", "catch", "--replay_size", str(SIZE), "--offline_replay", path, "--train_steps", "300", "--test_steps", "64",
            "--eval_envs", "32", "--epochs", "1", "--target_steps", "128", "--random_seed", "7", "--csv_file", str(tmp)] + list(extra)


def test_main_trains_offline_and_the_chunk_size_changes_no_bit(sd, dataset, tmp_path, monkeypatch):
    from simple_dqn_amd import agent as agent_mod, main as M
    weights, logs = [], []
    for chunk in (64, 1):
        refreshed = []

        class _Agent(agent_mod.Agent):
            def __init__(self, *a, **kw):
                kw["offline_chunk"] = chunk
                super().__init__(*a, **kw)
                net, me = self.net, self
                orig = net.update_target_network
                net.update_target_network = lambda: (refreshed.append(me.total_train_steps), orig())[1]

            def play_random(self, *a):
                raise AssertionError("offline training collects nothing")

            def train(self, *a):
                raise AssertionError("offline training collects nothing")

        monkeypatch.setattr(sd, "Agent", _Agent)
        out = tmp_path / ("c%d.csv" % chunk)
        random.seed(7)
        stats = M.run(M.build_parser().parse_args(_argv(dataset, out)))
        assert stats.agent.offline_chunk == chunk and stats.agent.total_train_steps == 300 and stats.net.train_iterations == 300
        assert refreshed == [0, 128, 256]                        # before learn t with t % target_steps == 0
        rows = list(csv.reader(open(out)))
        assert [r[1] for r in rows[1:]] == ["train", "test"] and rows[1][2:4] == ["0", "0"] and rows[1][9] == str(SIZE)
        assert int(rows[2][2]) == 64                             # the test phase played on the device games
        weights.append([np.array(w) for w in stats.net.get_weights()] + [np.array(w) for w in stats.net.get_weights(1)])
        logs.append(rows[1][11])
    for a, b in zip(*weights):
        assert np.array_equal(a, b)
    assert logs[0] == logs[1]                                    # the running mean of the costs too


def test_save_replay_through_main_is_what_offline_replay_accepts(sd, tmp_path):
    """main.run --save_replay after a random phase, and after --play_games, writes the memory as the run leaves it; --offline_replay loads it"""
    from simple_dqn_amd import main as M
    base = ["--environment", "catch", "--replay_size", "600", "--random_seed", "3", "--test_steps", "0"]
    p1, p2 = str(tmp_path / "random.ring"), str(tmp_path / "played.ring")
    st = M.run(M.build_parser().parse_args(base + ["--random_steps", "450", "--epochs", "0", "--save_replay", p1]))
    head = sd.ReplayMemory.peek(p1)
    assert (head["size"], head["count"], head["current"]) == (600, 450, 450) == (600, st.mem.count, st.mem.current)
    st2 = M.run(M.build_parser().parse_args(base + ["--offline_replay", p1, "--train_steps", "20", "--epochs", "1"]))
    assert st2.mem.count == 450 and st2.net.train_iterations == 20
    for name in ("actions", "rewards", "terminals", "screens"):
        assert np.array_equal(np.asarray(getattr(st.mem, name))[:450], np.asarray(getattr(st2.mem, name))[:450]), name
    st3 = M.run(M.build_parser().parse_args(base + ["--play_games", "1", "--save_replay", p2]))
    assert sd.ReplayMemory.peek(p2)["count"] == st3.mem.count > 0


def test_a_dataset_of_another_size_is_refused(sd, dataset, tmp_path):
    from simple_dqn_amd import main as M
    argv = _argv(dataset, tmp_path / "x.csv")
    argv[argv.index("--replay_size") + 1] = "3000"
    with pytest.raises(ValueError) as ei:
        M.run(M.build_parser().parse_args(argv))
    assert "--replay_size" in str(ei.value) and "2000" in str(ei.value) and "3000" in str(ei.value)


def test_cql_holds_the_unseen_action_down(sd):
    """the dataset holds only actions 0 and 1 (a two-action random policy on catch, written through mem.add); 500 learns each with alpha 1
    and alpha 0 from the same seed; on 64 hold-out states mean(Q[:, 2] - max(Q[:, :2])) is lower with alpha 1.  Only the sign is asserted."""
    gaps = {}
    for alpha in (1.0, 0.0):
        args = _catch_args(cql_alpha=alpha, target_steps=100, random_seed=11)
        random.seed(11)
        env, mem, net = sd.CatchEnvironment(args, seed=11), sd.ReplayMemory(SIZE, args), sd.DeepQNetwork(3, args)
        rng = np.random.RandomState(11)
        env.restart()
        for _ in range(SIZE):
            a = int(rng.randint(2))
            r = env.act(a)
            term = env.isTerminal()
            mem.add(a, r, env.getScreen(), term)
            if term:
                env.restart()
        assert set(np.unique(np.asarray(mem.actions)[:mem.count]).tolist()) == {0, 1}
        agent = sd.Agent(env, mem, net, args)
        agent.train_offline(500)
        assert net.train_iterations == 500
        random.seed(99)
        hold = np.concatenate([np.array(mem.getMinibatch()[0]) for _ in range(2)])
        q = np.concatenate([net.predict(hold[:32]), net.predict(hold[32:])]).astype(np.float64)
        gaps[alpha] = float((q[:, 2] - q[:, :2].max(axis=1)).mean())
    print("mean(Q[:, 2] - max(Q[:, :2])): alpha 1: %.5f, alpha 0: %.5f" % (gaps[1.0], gaps[0.0]))
    assert gaps[1.0] < gaps[0.0]
