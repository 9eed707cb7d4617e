"""Which training options combine, on the device: one network per option that is on first, every other option's setter
attempted on it, against what the library answered before its refusals became a table (tests/golden/option_conflicts_lib.json).
Nothing trains."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import make_args  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_conflicts_lib.json")


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _get(lib, fn, h, types, pick=0):
    out = [t() for t in types]
    assert getattr(lib, fn)(h, *[C.byref(o) for o in out]) == 0
    return out[pick].value


# option -> (switch it on, switch it off, is it on); double_dqn has no getter in the C ABI (None: _double_dqn_is_on)
OPTIONS = {
    "double_dqn": (lambda lib, h: lib.sdqn_net_set_option(h, b"double_dqn", 1), lambda lib, h: lib.sdqn_net_set_option(h, b"double_dqn", 0), None),
    "munchausen": (lambda lib, h: lib.sdqn_net_set_munchausen(h, 1, 0.9, 0.03, -1.0), lambda lib, h: lib.sdqn_net_set_munchausen(h, 0, 0.9, 0.03, -1.0),
                   lambda lib, h: _get(lib, "sdqn_net_get_munchausen", h, [C.c_int, C.c_double, C.c_double, C.c_double]) == 1),
    "advantage_learning": (lambda lib, h: lib.sdqn_net_set_advantage_learning(h, 0.5, 0), lambda lib, h: lib.sdqn_net_set_advantage_learning(h, 0.0, 0),
                           lambda lib, h: _get(lib, "sdqn_net_get_advantage_learning", h, [C.c_double, C.c_int]) > 0.0),
    "cql_alpha": (lambda lib, h: lib.sdqn_net_set_cql(h, 1.0), lambda lib, h: lib.sdqn_net_set_cql(h, 0.0),
                  lambda lib, h: _get(lib, "sdqn_net_get_cql", h, [C.c_double]) > 0.0),
    "bootstrap_heads": (lambda lib, h: lib.sdqn_net_set_bootstrap(h, 2, 1.0, 0), lambda lib, h: lib.sdqn_net_set_bootstrap(h, 1, 1.0, 0),
                        lambda lib, h: _get(lib, "sdqn_net_get_bootstrap", h, [C.c_int, C.c_double, C.c_uint64]) > 1),
    "quantiles": (lambda lib, h: lib.sdqn_net_set_quantiles(h, 2), lambda lib, h: lib.sdqn_net_set_quantiles(h, 1),
                  lambda lib, h: _get(lib, "sdqn_net_get_quantiles", h, [C.c_int]) > 1),
    "dueling": (lambda lib, h: lib.sdqn_net_set_dueling(h, 1), lambda lib, h: lib.sdqn_net_set_dueling(h, 0),
                lambda lib, h: _get(lib, "sdqn_net_get_dueling", h, [C.c_int]) == 1),
    "noisy_nets": (lambda lib, h: lib.sdqn_net_set_noisy(h, 1, 0.5, 0), lambda lib, h: lib.sdqn_net_set_noisy(h, 0, 0.5, 0),
                   lambda lib, h: _get(lib, "sdqn_net_get_noisy", h, [C.c_int, C.c_double, C.c_uint64, C.c_int64]) == 1),
    "clip_grad_norm": (lambda lib, h: lib.sdqn_net_set_clip_grad_norm(h, 5.0), lambda lib, h: lib.sdqn_net_set_clip_grad_norm(h, 0.0),
                       lambda lib, h: _get(lib, "sdqn_net_get_clip_grad_norm", h, [C.c_double]) > 0.0),
    "target_tau": (lambda lib, h: lib.sdqn_net_set_target_tau(h, 0.1), lambda lib, h: lib.sdqn_net_set_target_tau(h, 0.0),
                   lambda lib, h: _get(lib, "sdqn_net_get_target_tau", h, [C.c_double]) > 0.0),
}
FIRSTS = list(OPTIONS) + ["batch_norm"]                    # batch_norm is a property of the network: on from its creation, no setter


def _double_dqn_is_on(lib, h):
    """Double DQN shows in what it refuses: --munchausen is refused beside it and, on a plain network, beside nothing else.  Only asked
    where munchausen itself is off and nothing else that excludes it is on."""
    if lib.sdqn_net_set_munchausen(h, 1, 0.9, 0.03, -1.0) == 0:
        assert lib.sdqn_net_set_munchausen(h, 0, 0.9, 0.03, -1.0) == 0
        return False
    return True


def enumerate_pairs(sd):
    """[{first, second, rc, message}] for every network and every setter attempted on it; asserts what holds whatever the table says"""
    lib, rows = sd.load(), []
    for first in FIRSTS:
        net = sd.DeepQNetwork(4, make_args(batch_size=32, batch_norm=first == "batch_norm"))
        h = net._h
        if first != "batch_norm":
            assert OPTIONS[first][0](lib, h) == 0, (first, lib.sdqn_last_error())
        for second, (on, off, is_on) in OPTIONS.items():
            if second == first:
                continue
            rc = on(lib, h)
            rows.append({"first": first, "second": second, "rc": 0 if rc == 0 else -1, "message": None if rc == 0 else lib.sdqn_last_error().decode()})
            if rc == 0:
                assert off(lib, h) == 0, (first, second, lib.sdqn_last_error())          # allowed: off again, one option beside the first at a time
            elif is_on is not None:
                assert not is_on(lib, h), (first, second)                                # refused: the handle is as it was
            if first == "batch_norm":
                assert net.batch_norm
            elif OPTIONS[first][2] is not None:
                assert OPTIONS[first][2](lib, h), (first, second)
            assert _get(lib, "sdqn_net_train_iterations", h, [C.c_int64]) == 0
        if first == "double_dqn":
            assert _double_dqn_is_on(lib, h)
    return rows


def test_every_pair_answers_as_recorded(sd):
    golden = json.load(open(GOLDEN))
    rows = enumerate_pairs(sd)
    assert len(rows) == len(golden) == 100
    for got, want in zip(rows, golden):
        assert got == want, (got, want)
    assert sum(r["rc"] != 0 for r in rows) == 2 * 36 - 7                                 # every refused pair both ways; batch_norm's 7 one way only


def test_a_refused_double_dqn_stays_off(sd):
    """the one option without a getter: refused beside --dueling, then --dueling off, --munchausen is welcome (it is not beside double_dqn)"""
    lib = sd.load()
    net = sd.DeepQNetwork(4, make_args(batch_size=32))
    assert lib.sdqn_net_set_dueling(net._h, 1) == 0
    assert lib.sdqn_net_set_option(net._h, b"double_dqn", 1) != 0
    assert lib.sdqn_net_set_dueling(net._h, 0) == 0
    assert not _double_dqn_is_on(lib, net._h)
