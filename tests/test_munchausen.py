"""--munchausen without a device: the oracle's soft value and bonus against the naive formulas, the command line and its
refusals, the C ABI symbol, and the compiler's resource report of the Munchausen head kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
import munchausen_oracle as MO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _naive(q, actions, alpha, tau, clip):
    """V = sum_a pi (q - tau ln pi) and m = alpha clip(tau ln pi(a)), pi = softmax(q / tau) in np.longdouble"""
    ql = np.asarray(q, dtype=np.longdouble)
    z = (ql - ql.max(axis=1, keepdims=True)) / np.longdouble(tau)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    pi = e / s
    tlogpi = np.longdouble(tau) * (z - np.log(s))             # tau ln pi, finite where pi underflows to 0
    V = (pi * (ql - tlogpi)).sum(axis=1)
    n = np.arange(len(q))
    m = np.longdouble(alpha) * np.clip(tlogpi[n, actions], clip, 0.0)
    return np.asarray(V, dtype=np.float64), np.asarray(m, dtype=np.float64)


@pytest.mark.parametrize("tau", [1.0, 0.03, 1e-4])
@pytest.mark.parametrize("A", [1, 2, 4, 5, 18])
def test_soft_value_and_bonus_equal_the_naive_formulas(A, tau):
    rng = np.random.RandomState(100 * A + int(-np.log10(tau)))
    q = rng.randn(64, A) * rng.choice([0.01, 1.0, 30.0], size=(64, 1))
    q[0] = 0.0                                                 # an exact tie
    actions = rng.randint(0, A, 64)
    alpha, clip = 0.9, -1.0
    V, m = MO.soft_value(q, tau), MO.bonus(q, actions, alpha, tau, clip)
    assert np.isfinite(V).all() and np.isfinite(m).all()
    Vn, mn = _naive(q, actions, alpha, tau, clip)
    assert np.abs(V - Vn).max() <= 1e-12, np.abs(V - Vn).max()
    assert np.abs(m - mn).max() <= 1e-12, np.abs(m - mn).max()
    assert (m <= 0).all() and (m >= alpha * clip).all() and (V >= q.max(axis=1)).all()
    if A == 1:
        assert np.array_equal(V, q[:, 0]) and np.array_equal(m, np.zeros(64)) and not np.signbit(m).any()


def test_parser_defaults_and_refusals_before_any_device_call():
    from simple_dqn_amd import main
    d = main.build_parser().parse_args([])
    assert d.munchausen is False and d.munchausen_alpha == 0.9 and d.munchausen_tau == 0.03 and d.munchausen_clip == -1
    assert main.check_munchausen(d) is False
    on = main.build_parser().parse_args(["--munchausen", "true", "--munchausen_alpha", "0", "--munchausen_tau", "1e-4", "--munchausen_clip", "0"])
    assert main.check_munchausen(on) is True
    base = ["--munchausen", "true", "--random_steps", "0", "--epochs", "0"]
    for extra, words in ((["--munchausen_tau", "0"], ("--munchausen_tau",)),
                         (["--munchausen_tau", "-0.5"], ("--munchausen_tau",)),
                         (["--munchausen_tau", "nan"], ("--munchausen_tau",)),
                         (["--munchausen_alpha", "-0.1"], ("--munchausen_alpha",)),
                         (["--munchausen_alpha", "1.5"], ("--munchausen_alpha",)),
                         (["--munchausen_clip", "0.25"], ("--munchausen_clip",)),
                         (["--double_dqn", "true"], ("--munchausen", "--double_dqn")),
                         (["--batch_norm", "true"], ("--munchausen", "--batch_norm"))):
        args = main.build_parser().parse_args(base + extra)
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never this ValueError
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
    # the parameter ranges hold with the option off too; the two combinations are refused only when it is on
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true"])
    assert main.check_munchausen(off) is False
    with pytest.raises(ValueError):
        main.check_munchausen(main.build_parser().parse_args(["--munchausen_tau", "0"]))


def test_symbol_in_signatures_and_library():
    for name in ("sdqn_net_set_munchausen", "sdqn_net_get_munchausen"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name), name
    assert "sdqn_net_set_munchausen" in open(os.path.join(ROOT, "include", "sdqn.h")).read()


def test_isa_census_of_the_munchausen_heads():
    """every Munchausen head: no scratch, LDS no larger than head_kernel's for the same action bucket; the new translation unit left the
    default head's name alone (tests/test_kernarg_preload_census.py selects it by this fragment)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    mu = [r for r in isa_census.census_rows("sdqn_munchausen.hip") if "munchausen_head_kernel" in r["name"]]
    std = isa_census.census_rows("sdqn_kernels.hip")
    assert len([r for r in std if "head_kernelILi4ELb0ELb0ELb0ELb0ELb0E" in r["name"]]) == 1
    assert len(mu) == 12, [r["name"] for r in mu]           # 3 buckets x {plain, PER} x {one-step, n-step}
    for bucket in (4, 8, 18):
        ref = [r for r in std if "head_kernelILi%dELb0ELb0ELb0ELb0ELb0E" % bucket in r["name"]]
        assert len(ref) == 1, bucket
        mine = [r for r in mu if "munchausen_head_kernelILi%dE" % bucket in r["name"]]
        assert len(mine) == 4, (bucket, [r["name"] for r in mine])
        for r in mine:
            print("%s: vgpr %d lds %d scratch %d (head_kernel: lds %d)" % (r["name"][:60], r["vgpr"], r["lds"], r["scratch"], ref[0]["lds"]))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] <= ref[0]["lds"], (r["name"], r["lds"], ref[0]["lds"])
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])     # two 512-thread workgroups per CU, as the standard head
