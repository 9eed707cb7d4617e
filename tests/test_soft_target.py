"""--target_tau without a device: the bindings, the command line, main.run's refusals, the oracle's ability to tell the
specified three-rounding blend from a contracted one, and the Agent's hard-update schedule on a stub network."""
import ctypes as C
import random

import numpy as np
import pytest

from soft_target_oracle import blend, blend32_through_fp64, hard_updates
from util import make_args


def test_bindings_are_declared_and_exported():
    import simple_dqn_amd as sd
    sig = sd._lib.SIGNATURES
    assert sig["sdqn_net_soft_update"] == (C.c_int, [C.c_void_p, C.c_double])
    assert sig["sdqn_net_set_target_tau"] == (C.c_int, [C.c_void_p, C.c_double])
    assert sig["sdqn_net_get_target_tau"][1][1] == C.POINTER(C.c_double)
    lib = sd.load()
    for name in ("sdqn_net_soft_update", "sdqn_net_set_target_tau", "sdqn_net_get_target_tau"):
        assert getattr(lib, name) is not None
    # the blend has a profile row of its own, appended after the last one
    n = C.c_int()
    assert lib.sdqn_net_profile_count(C.byref(n)) == 0 and n.value == 28
    header = open(sd._lib._HERE + "/../include/sdqn.h").read()
    for name in ("sdqn_net_soft_update", "sdqn_net_set_target_tau", "sdqn_net_get_target_tau"):
        assert "int %s(" % name in header


def test_parser_accepts_target_tau():
    from simple_dqn_amd import main
    assert main.build_parser().parse_args([]).target_tau == 0.0
    a = main.build_parser().parse_args(["--target_tau", "0.005"])
    assert a.target_tau == 0.005
    assert main.check_target_tau(a) == 0.005


@pytest.mark.parametrize("extra", [["--target_tau", "-0.1"], ["--target_tau", "1.5"], ["--target_tau", "nan"],
                                   ["--target_tau", "0.01", "--target_steps", "0"]])
def test_main_run_refuses_before_touching_the_device(extra, monkeypatch):
    from simple_dqn_amd import main
    import simple_dqn_amd
    def no_device(*a, **k):
        raise RuntimeError("a device object was constructed")
    for cls in ("DeepQNetwork", "ReplayMemory"):
        monkeypatch.setattr(simple_dqn_amd, cls, no_device)
    args = main.build_parser().parse_args(["--random_steps", "0", "--epochs", "0"] + extra)
    with pytest.raises(ValueError) as ei:
        main.run(args)
    assert "--target_tau" in str(ei.value)


def test_oracle_tells_three_roundings_from_one():
    rng = np.random.RandomState(2024)
    w, wt = rng.uniform(-1, 1, 100000).astype(np.float32), rng.uniform(-1, 1, 100000).astype(np.float32)
    a, b = blend(w, wt, 0.25), blend32_through_fp64(w, wt, 0.25)
    assert a.dtype == np.float32 and b.dtype == np.float32
    differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print("three roundings vs one: %d of %d values differ" % (differ, a.size))
    assert differ > 0
    assert np.abs(a.astype(np.float64) - b).max() < 1e-6                   # ... by round-off only
    # float64 form: same formula in double; tau = 1 need not reproduce theta (why the library special-cases it)
    assert blend(w, wt, 0.25, np.float64).dtype == np.float64
    assert (blend(w, wt, 1.0) != w).any()


class _StubNet:
    """records ('hard' | 'train', the agent's total_train_steps at the call)"""

    def __init__(self, A):
        self.A, self.calls, self.train_iterations, self.agent = A, [], 0, None

    def _note(self, what):
        self.calls.append((what, self.agent.total_train_steps))

    def update_target_network(self):
        self._note("hard")

    def predict(self, states):
        return np.zeros((states.shape[0], self.A), np.float32)

    def train(self, minibatch, epoch=0):
        self._note("train")
        self.train_iterations += 1


class _StubEnv:
    def __init__(self, A):
        self.A, self.t = A, 0

    def numActions(self):
        return self.A

    def restart(self):
        pass

    def act(self, action):
        self.t += 1
        return 0

    def getScreen(self):
        return np.full((84, 84), self.t & 255, np.uint8)

    def isTerminal(self):
        return False


class _StubMem:
    batch_size = 4

    def __init__(self):
        self.count = 0

    def add(self, action, reward, screen, terminal):
        self.count += 1

    def getMinibatch(self):
        return None


def _run_agent(target_tau, calls=2, train_steps=10, target_steps=4):
    from simple_dqn_amd.agent import Agent
    args = make_args(batch_size=4, train_frequency=1, target_steps=target_steps, target_tau=target_tau, exploration_decay_steps=10)
    net = _StubNet(3)
    agent = net.agent = Agent(_StubEnv(3), _StubMem(), net, args, fused=False)
    random.seed(1)
    for _ in range(calls):
        agent.train(train_steps, 0)
    assert agent.total_train_steps == calls * train_steps
    return net.calls


def test_agent_schedule_with_and_without_target_tau():
    trains = [("train", t) for t in range(4, 20)]                          # one per env step once the memory holds > batch_size transitions
    on = _run_agent(0.01)
    assert [c for c in on if c[0] == "hard"] == [("hard", 0)]              # exactly one hard update over two consecutive train calls
    assert on[0] == ("hard", 0)                                            # ... before anything trains
    assert [c for c in on if c[0] == "train"] == trains
    assert hard_updates(2, 10, 4, 0.01) == [0]
    # off: today's sequence, i % target_steps == 0 of every call -> steps 0, 4, 8 of each call, each before that step's train
    off = _run_agent(0.0)
    assert hard_updates(2, 10, 4, 0.0) == [0, 4, 8, 10, 14, 18]
    expected = []
    for t in range(20):
        expected += [("hard", t)] if t in (0, 4, 8, 10, 14, 18) else []
        expected += [("train", t)] if t >= 4 else []
    assert off == expected
    assert [t for what, t in off if what == "hard"] == hard_updates(2, 10, 4, 0.0)
    # a resumed run (start_epoch > 0) makes no hard update at all with the option on
    assert hard_updates(1, 10, 4, 0.01, start=100) == []
