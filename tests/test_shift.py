"""--random_shift without a device: the command line, the refusals, the draws restated exactly, the shift against numpy's own
padding, and the kernel's resource census."""
import os
import sys

import numpy as np
import pytest

import shift_oracle as S
from simple_dqn_amd import deepqnetwork as D
from simple_dqn_amd.main import build_parser, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdqn_net_set_random_shift", "sdqn_net_get_random_shift", "sdqn_random_shift_draw", "sdqn_net_last_shifts")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402


def test_flag_parses():
    assert build_parser().parse_args([]).random_shift == 0
    assert build_parser().parse_args(["--random_shift", "4"]).random_shift == 4
    for P in range(9):
        assert D.check_random_shift(build_parser().parse_args(["--random_shift", str(P)])) == P


REFUSED = [(["--random_shift", "9"], "9"), (["--random_shift", "-1"], "-1"), (["--random_shift", "4", "--batch_norm", "true"], "--batch_norm"),
           (["--random_shift", "8", "--screen_height", "8", "--screen_width", "20"], "--screen_height 8"),
           (["--random_shift", "5", "--screen_height", "20", "--screen_width", "5"], "--screen_width 5")]


@pytest.mark.parametrize("extra,named", REFUSED, ids=[" ".join(e) for e, _ in REFUSED])
def test_run_refuses_by_name_before_touching_a_device(extra, named):
    args = build_parser().parse_args(["--environment", "catch"] + extra)
    with pytest.raises(ValueError) as e:
        run(args)
    assert "--random_shift" in str(e.value) and named in str(e.value)


def test_flag_off_refuses_nothing():
    assert D.check_random_shift(build_parser().parse_args(["--batch_norm", "true", "--screen_height", "1"])) == 0


def test_symbols_in_header_signatures_and_library():
    import simple_dqn_amd as sd
    from simple_dqn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name in hdr, name


@pytest.mark.parametrize("P", [1, 4, 8])
def test_library_draw_equals_the_oracle(P):
    rng = np.random.RandomState(P)
    seen_lo = seen_hi = False
    for k in range(10000):
        if k < 64:                                            # the corners of the key space first
            seed = (0, 123, 2 ** 64 - 1, 2 ** 63)[k & 3]; step = (0, 1, 2 ** 40 + 3, 2 ** 64 - 2)[(k >> 2) & 3]; n = (0, 1, 255, 4095)[(k >> 4) & 3]
        else:
            seed = int(rng.randint(0, 2 ** 62)) * 4 + int(rng.randint(0, 4)); step = int(rng.randint(0, 2 ** 31)); n = int(rng.randint(0, 4096))
        s = k & 1
        got = D.random_shift_draw(seed, step, n, s, P)
        assert got == S.draw(seed, step, n, s, P), (seed, step, n, s)
        assert -P <= got[0] <= P and -P <= got[1] <= P
        seen_lo |= -P in got
        seen_hi |= P in got
    assert seen_lo and seen_hi


@pytest.mark.parametrize("P", [1, 2])
def test_every_pair_occurs(P):
    seen = {D.random_shift_draw(7, t, n, s, P) for t in range(8) for n in range(32) for s in (0, 1)}
    assert seen == {(a, b) for a in range(-P, P + 1) for b in range(-P, P + 1)}


def test_pre_and_post_draw_independently():
    d = S.draws(123, 0, 256, 4)
    assert (d[:, 0] != d[:, 1]).any(axis=1).mean() > 0.9       # equal by chance with probability 1 / 81
    assert not np.array_equal(S.draws(123, 0, 32, 4), S.draws(123, 1, 32, 4)) and not np.array_equal(S.draws(123, 0, 32, 4), S.draws(124, 0, 32, 4))


@pytest.mark.parametrize("H,W", [(84, 84), (36, 38), (9, 12)])
def test_oracle_shift_is_edge_padding_then_a_crop(H, W):
    rng = np.random.RandomState(H)
    st = rng.randint(0, 256, (3, H, W), dtype=np.uint8)
    for P in (1, 4, 8):
        pad = np.pad(st, ((0, 0), (P, P), (P, P)), mode="edge")
        for dy in (-P, 0, 1, P):
            for dx in (-P, -1, 0, P):
                assert np.array_equal(S.shift(st, dy, dx), pad[:, P + dy:P + dy + H, P + dx:P + dx + W]), (P, dy, dx)


def test_forced_corner_seed_is_found_within_1000():
    seed = S.forced_seed(8, 2)
    assert seed is not None and seed < 1000
    d = np.array([[D.random_shift_draw(seed, 0, n, s, 2) for s in (0, 1)] for n in range(8)])
    assert np.array_equal(d, S.draws(seed, 0, 8, 2))
    assert (d == -2).all(axis=2).any() and (d == 2).all(axis=2).any()


needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_census.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_isa_census_of_the_shift_kernel():
    """shift_gather_kernel: no scratch, no LDS, the register count of the build recorded in DESIGN.md §34 (16 VGPRs, no AGPRs)"""
    rows = [r for r in isa_census.census_rows("sdqn_shift.hip") if "shift_gather_kernel" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in rows]
    r = rows[0]
    print("shift_gather_kernel: vgpr %d agpr %d lds %d scratch %d" % (r["vgpr"], r["agpr"], r["lds"], r["scratch"]))
    assert r["scratch"] == 0 and r["lds"] == 0 and r["mfma"] == 0 and r["barriers"] == 0
    # (the figure of the compiler this tree was built with: a toolchain that allocates another register fails here with the code unchanged —
    #  then re-run the census, check that nothing else moved, and record the new figure here and in §34.2)
    assert r["vgpr"] + r["agpr"] <= 16, r
