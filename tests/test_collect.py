"""--train_envs without a device: the lane sampler of the library against its numpy restatement
(tests/collect_oracle.py) index for index and draw for draw, its refusals, and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
from oracle.replay_numpy import MT19937  # noqa: E402
import collect_oracle as CO  # noqa: E402
from util import make_args  # noqa: E402

N, L, HIST, B = 3, 23, 4, 32
CASES = [(12, 12), (L, 0), (L, 5), (L, 22)]                # (fill, write position): not wrapped (p == f), and full at three positions


def _terminals():
    t = np.zeros(N * L, np.uint8)
    t[::11] = 1
    return t


def _native(seed, term, lanes, lane_len, f, p, n, batch=B, hist=HIST):
    lib = sd.load()
    mt = (C.c_uint32 * 625)()
    _lib.check(lib.sdqn_mt_seed(mt, seed))
    idx, draws = np.full(batch, -1, np.int64), C.c_int64()
    _lib.check(lib.sdqn_sample_indices_lanes(mt, _lib.ptr(term, C.c_uint8), lanes, lane_len, f, p, hist, n, batch,
                                             _lib.ptr(idx, C.c_int64), C.byref(draws)))
    return idx, draws.value, mt


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("f,p", CASES)
def test_lane_sampler_equals_the_oracle(f, p, n):
    term = _terminals()
    valid = CO.valid_indexes(term, N, L, f, p, HIST, n)
    assert len(valid) >= B // 2, (f, p, n, len(valid))     # on the oracle alone: the rejection loop cannot spin
    rng = MT19937(17 + n)
    mt = None
    for call in range(3):                                  # consecutive calls go on in the same stream
        o_idx, o_draws = CO.sample_indexes_lanes(rng, term, N, L, f, p, HIST, n, B)
        if mt is None:
            idx, draws, mt = _native(17 + n, term, N, L, f, p, n)
        else:
            d = C.c_int64()
            _lib.check(sd.load().sdqn_sample_indices_lanes(mt, _lib.ptr(term, C.c_uint8), N, L, f, p, HIST, n, B,
                                                           _lib.ptr(idx, C.c_int64), C.byref(d)))
            draws = d.value
        assert idx.tolist() == o_idx.tolist() and draws == o_draws, call
        assert draws > B or len(valid) == N * (f - n - HIST + 1)       # (rejections happened wherever something is rejectable)
        for i in idx:
            lane, l = divmod(int(i), L)
            assert 0 <= lane < N and l >= HIST and l + n - 1 < f   # the whole window [i - hist, i + n - 1] lies inside one lane
            assert (i - HIST) // L == (i + n - 1) // L == lane
            assert not (l + n - 1 >= p and l - HIST < p)           # ... avoids the write position
            assert not term[i - HIST:i].any()                      # ... and has a clean prestate
            assert int(i) in valid
    assert set(idx.tolist()) <= set(valid)


def test_lane_sampler_refusals():
    term = _terminals()
    for kw in (dict(f=HIST + 1 - 1, n=1),                  # span = f - n - hist + 1 = 0
               dict(f=HIST + 2, n=3),                      # span = 0 with n = 3
               dict(lanes=0), dict(lanes=-2),              # bad N
               dict(lane_len=HIST + 1 + 1),                # L < hist + n + 2
               dict(f=L + 1), dict(p=L), dict(p=-1), dict(n=0), dict(n=17), dict(batch=0)):
        a = dict(lanes=N, lane_len=L, f=12, p=12, n=1, batch=B)
        a.update(kw)
        if "p" not in kw and a["f"] < L:
            a["p"] = a["f"]
        with pytest.raises(AssertionError):
            _native(1, term, a["lanes"], a["lane_len"], a["f"], a["p"], a["n"], a["batch"])
    with pytest.raises(AssertionError):                    # every prestate holds a terminal: the loop would spin
        _native(1, np.ones(N * L, np.uint8), N, L, 12, 12, 1)
    idx, draws, _ = _native(1, term, N, L, 12, 12, 1)      # and the same arguments without a fault are served
    assert draws >= B and (idx >= 0).all()


def test_command_line_and_refusals_before_any_device_call():
    from simple_dqn_amd import main
    a = main.build_parser().parse_args(["--environment", "catch", "--train_envs", "32", "--replay_size", "20000"])
    assert a.train_envs == 32 and main.check_train_envs(a) == 32
    d = main.build_parser().parse_args([])
    assert d.train_envs == 0 and main.check_train_envs(d) == 0
    for name in ("sdqn_env_collect", "sdqn_replay_set_lanes", "sdqn_replay_get_lanes", "sdqn_sample_indices_lanes"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name)
    base = ["--environment", "catch", "--train_envs", "32", "--replay_size", "20000", "--random_steps", "0", "--epochs", "0"]
    for extra, word in ((["--train_envs", "33"], "--batch_size"),
                        (["--environment", "synthetic"], "--environment"),
                        (["--prioritized_replay", "true"], "--prioritized_replay"),
                        (["--replay_size", "20001"], "--replay_size"),
                        (["--replay_size", "160"], "--replay_size")):
        args = main.build_parser().parse_args(base + extra)
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never this ValueError
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert "--train_envs" in str(ei.value) and word in str(ei.value), (extra, str(ei.value))
    ns = make_args(environment="catch", train_envs=4, batch_size=2, replay_size=400)
    with pytest.raises(ValueError):
        main.check_train_envs(ns)


def test_isa_census_of_the_collect_kernel():
    """registers, LDS and scratch of the collect kernel as the compiler reports them (tools/isa_census.py): no scratch, the 16 bytes of
    LDS of the view hand-off, registers far below the 128 that would halve the residency of a 512-thread workgroup; no atomics in the text"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_env.hip")
    hit = [r for r in rows if "catch_collect_kernel" in r["name"]]
    assert len(hit) == 1, [r["name"] for r in rows]
    k = hit[0]
    print("catch_collect_kernel: vgpr %d agpr %d lds %d scratch %d" % (k["vgpr"], k["agpr"], k["lds"], k["scratch"]))
    assert k["scratch"] == 0 and k["lds"] <= 64 and k["vgpr"] + k["agpr"] <= 128
    assert not [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    src = open(os.path.join(isa_census.CSRC, "sdqn_env.hip")).read() + open(os.path.join(isa_census.CSRC, "env_catch.h")).read()
    assert "atomic" not in src.lower()
