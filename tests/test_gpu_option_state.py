"""The target options' state on the device, on both train paths: the smallest generic net that has every layer (36 x 36 x 2
screens, float64: conv outputs 8 x 8, 3 x 3, 1 x 1) and the tuned 84 x 84 x 4 float32 net, B = 4, 3 actions.

A refused setter call — an option the table pairs with one that is on, a value out of range, n_step beside the persistent form — answers
with its error and leaves every value the getters show as it was; a twin with the same seed that never made those calls then trains to the
same bits.  An option switched on and off between steps reaches the step it is on for and no other.  Every assertion is bit-equality
between two nets of one library, so the test asks the same of any layout of the state."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import make_args  # noqa: E402

pytestmark = pytest.mark.gpu
B, A = 4, 3
PATHS = {"generic": dict(screen_height=36, screen_width=36, history_length=2, datatype="float64"), "tuned": {}}
GETTERS = (("sdqn_net_get_munchausen", (C.c_int, C.c_double, C.c_double, C.c_double)), ("sdqn_net_get_advantage_learning", (C.c_double, C.c_int)),
           ("sdqn_net_get_cql", (C.c_double,)), ("sdqn_net_get_bootstrap", (C.c_int, C.c_double, C.c_uint64)), ("sdqn_net_get_quantiles", (C.c_int,)),
           ("sdqn_net_get_dueling", (C.c_int,)))


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def make_net(sd, path):
    return sd.DeepQNetwork(A, make_args(batch_size=B, random_seed=7, **PATHS[path]))


def minibatches(path, n):
    kw = PATHS[path]
    shape = (B, kw.get("history_length", 4), kw.get("screen_height", 84), kw.get("screen_width", 84))
    rng = np.random.RandomState(11)
    return [(rng.randint(0, 256, shape, dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8), rng.randint(-1, 2, B).astype(np.int64),
             rng.randint(0, 256, shape, dtype=np.uint8), np.array([False, True, False, False])) for _ in range(n)]


def state(lib, h):
    """every value the C ABI's getters show"""
    out = []
    for fn, types in GETTERS:
        vals = [t() for t in types]
        assert getattr(lib, fn)(h, *[C.byref(v) for v in vals]) == 0
        out.append((fn,) + tuple(v.value for v in vals))
    return out


def assert_same_bits(a, b):
    for which in (0, 1):
        for wa, wb in zip(a.get_weights(which), b.get_weights(which)):
            assert np.array_equal(wa, wb)
    for qa, qb in zip(a.last_q(), b.last_q()):
        assert np.array_equal(qa, qb)


# the option that is on -> (switch it on, [(refused call, a fragment of its error)])
SCENARIOS = {
    "double_dqn": (
        lambda net: net.set_option("double_dqn", 1),
        [(lambda lib, h: lib.sdqn_net_set_munchausen(h, 1, 0.9, 0.03, -1.0), b"munchausen cannot be combined with double_dqn"),
         (lambda lib, h: lib.sdqn_net_set_munchausen(h, 0, 0.5, -1.0, -1.0), b"munchausen_tau"),
         (lambda lib, h: lib.sdqn_net_set_advantage_learning(h, 0.5, 0), b"advantage_learning cannot be combined with double_dqn"),
         (lambda lib, h: lib.sdqn_net_set_cql(h, -1.0), b"cql_alpha -1"),
         (lambda lib, h: lib.sdqn_net_set_bootstrap(h, 3, 1.0, 5), b"bootstrap_heads 3 cannot be combined with double_dqn"),
         (lambda lib, h: lib.sdqn_net_set_quantiles(h, 3), b"quantiles 3 cannot be combined with double_dqn"),
         (lambda lib, h: lib.sdqn_net_set_dueling(h, 1), b"dueling cannot be combined with double_dqn"),
         (lambda lib, h: lib.sdqn_net_set_option(h, b"n_step", 0), b"n_step 0 out of range")]),
    "persistent_advantage": (
        lambda net: net.set_advantage_learning(0.5, True),
        [(lambda lib, h: lib.sdqn_net_set_option(h, b"n_step", 2), b"n_step 2 cannot be combined with persistent_advantage"),
         (lambda lib, h: lib.sdqn_net_set_option(h, b"double_dqn", 1), b"double_dqn cannot be combined with advantage_learning"),
         (lambda lib, h: lib.sdqn_net_set_munchausen(h, 1, 0.9, 0.03, -1.0), b"munchausen cannot be combined with advantage_learning"),
         (lambda lib, h: lib.sdqn_net_set_advantage_learning(h, 1.0, 1), b"advantage_learning 1 outside"),
         (lambda lib, h: lib.sdqn_net_set_cql(h, 1.0), b"cql_alpha cannot be combined with advantage_learning"),
         (lambda lib, h: lib.sdqn_net_set_bootstrap(h, 3, 1.5, 5), b"bootstrap_mask_probability 1.5"),
         (lambda lib, h: lib.sdqn_net_set_quantiles(h, 3), b"quantiles 3 cannot be combined with advantage_learning"),
         (lambda lib, h: lib.sdqn_net_set_dueling(h, 1), b"dueling cannot be combined with advantage_learning")]),
}


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("path", list(PATHS))
def test_refused_calls_change_nothing(sd, path, scenario):
    lib = sd.load()
    switch_on, refused = SCENARIOS[scenario]
    a, b = make_net(sd, path), make_net(sd, path)
    mbs = minibatches(path, 3)
    for net in (a, b):
        net.train(mbs[0])                                  # the option is switched between steps
        switch_on(net)
    before = state(lib, a._h)
    assert before == state(lib, b._h)
    for call, fragment in refused:
        assert call(lib, a._h) != 0
        assert fragment in lib.sdqn_last_error(), (fragment, lib.sdqn_last_error())
        assert state(lib, a._h) == before
    for mb in mbs[1:]:
        a.train(mb)
        b.train(mb)
    assert_same_bits(a, b)


@pytest.mark.parametrize("path", list(PATHS))
def test_an_option_switched_on_and_off_reaches_its_step_only(sd, path):
    lib = sd.load()
    a, b, plain = make_net(sd, path), make_net(sd, path), make_net(sd, path)
    mbs = minibatches(path, 2)
    off = state(lib, a._h)
    for net in (a, b):
        net.set_munchausen(True, 0.8, 0.05, -2.0)
        assert state(lib, net._h)[0] == ("sdqn_net_get_munchausen", 1, 0.8, 0.05, -2.0)
        assert state(lib, net._h)[1:] == off[1:]
        net.train(mbs[0])
        net.set_munchausen(False)
        assert state(lib, net._h)[0] == ("sdqn_net_get_munchausen", 0, 0.8, 0.05, -2.0)      # (the parameters stay for the next time)
    plain.train(mbs[0])
    assert_same_bits(a, b)
    # the committed option took part in that step: the Munchausen target is not the standard one (a soft value and a log-policy bonus)
    assert not all(np.array_equal(x, y) for x, y in zip(a.get_weights(0), plain.get_weights(0)))
    for net in (a, b):
        net.train(mbs[1])
    assert_same_bits(a, b)
