"""--cql_alpha without a device: the command line and its refusals, the C ABI symbols, the oracle against autograd, the
host restatement sdqn_cql_loss against the oracle at its edges, and the compiler's resource report of the CQL head kernels."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
from simple_dqn_amd.deepqnetwork import cql_loss  # noqa: E402
import cql_oracle as CO  # noqa: E402
from oracle.dqn_numpy import OracleDQN, xavier_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = (2, 64, 48)                 # the smallest screen the tests of the generic path use


def test_parser_defaults_and_refusals_before_any_device_call():
    from simple_dqn_amd import deepqnetwork, main
    assert deepqnetwork.check_cql is not None and main.check_cql(main.build_parser().parse_args([])) == 0.0
    d = main.build_parser().parse_args([])
    assert d.cql_alpha == 0.0 and d.save_replay is None and d.offline_replay is None
    on = main.build_parser().parse_args(["--cql_alpha", "1", "--prioritized_replay", "true", "--n_step", "3", "--target_tau", "0.01",
                                         "--clip_grad_norm", "10", "--random_shift", "4", "--optimizer", "adam", "--datatype", "float16"])
    assert main.check_cql(on) == 1.0
    assert main.check_cql(main.build_parser().parse_args(["--cql_alpha", "5.5", "--datatype", "float64", "--screen_width", "48"])) == 5.5
    base = ["--random_steps", "0", "--epochs", "0"]
    cql = ["--cql_alpha", "1"]
    for extra, words in ((["--cql_alpha", "-0.1"], ("--cql_alpha",)),
                         (["--cql_alpha", "nan"], ("--cql_alpha",)),
                         (["--cql_alpha", "inf"], ("--cql_alpha",)),
                         (cql + ["--double_dqn", "true"], ("--cql_alpha", "--double_dqn")),
                         (cql + ["--munchausen", "true"], ("--cql_alpha", "--munchausen")),
                         (cql + ["--advantage_learning", "0.9"], ("--cql_alpha", "--advantage_learning")),
                         (cql + ["--bootstrap_heads", "2"], ("--cql_alpha", "--bootstrap_heads")),
                         (cql + ["--quantiles", "2"], ("--cql_alpha", "--quantiles")),
                         (cql + ["--dueling", "true"], ("--cql_alpha", "--dueling")),
                         (cql + ["--noisy_nets", "true"], ("--cql_alpha", "--noisy_nets")),
                         (cql + ["--batch_norm", "true"], ("--cql_alpha", "--batch_norm"))):
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:                    # check_cql itself names both flags
            main.check_cql(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never a ValueError
        with pytest.raises(ValueError):
            main.run(args)
        with pytest.raises(ValueError):                          # DeepQNetwork refuses too, before it loads the library
            sd.DeepQNetwork(4, args)
    # with alpha = 0 the other options are nobody's business
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true", "--dueling", "true"])
    assert main.check_cql(off) == 0.0


def test_symbols_in_signatures_header_and_library():
    header = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in ("sdqn_net_set_cql", "sdqn_net_get_cql", "sdqn_cql_loss"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name), name
        assert name + "(" in header, name


def _autograd(q, a, y, alpha):
    import torch
    t = torch.tensor(np.asarray(q, np.float64), requires_grad=True)
    loss = 0.5 * (t[a] - y) ** 2 + alpha * (torch.logsumexp(t, 0) - t[a])
    loss.backward()
    return t.grad.numpy(), float(loss.detach())


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 8, 9, 18])
def test_oracle_against_autograd(A):
    """dq and the cost term of cql_oracle in float64, without clip and weight, against torch.autograd of
    0.5 delta^2 + alpha (logsumexp(q) - q[a]) on the CPU: 1e-12"""
    rng = np.random.RandomState(A)
    for trial in range(20):
        q = rng.randn(A) * (1.0 if trial % 2 else 5.0)
        a, y, alpha = int(rng.randint(A)), float(rng.randn()), float(rng.choice([0.1, 1.0, 5.0]))
        dq, cost, d = CO.cql_sample(q, a, y, alpha, 0.0, 1.0, np.float64)
        g, loss = _autograd(q, a, y, alpha)
        assert np.abs(dq - g).max() <= 1e-12 * max(1.0, np.abs(g).max()), (q, a, y, dq, g)
        assert abs(float(cost) - loss) <= 1e-12 * max(1.0, abs(loss)), (cost, loss)
        assert d == q[a] - y


def _same(q, a, y, alpha, clip, w):
    """sdqn_cql_loss against the float32 oracle: the float operations are the same operations, so only the two libraries' exp and log (a few
    ulp in float64, below the one rounding to float32 but for ties) can differ — one float32 ulp of the larger magnitude in the row"""
    dq, cost = cql_loss(q, a, y, alpha, clip, w)
    odq, ocost, _ = CO.cql_sample(np.asarray(q, np.float32), a, y, alpha, clip, w, np.float32)
    assert np.isfinite(dq).all() and np.isfinite(cost)
    ulp = np.spacing(np.float32(max(np.abs(odq).max(), abs(float(ocost)), 1e-30)))
    assert np.abs(dq.astype(np.float64) - odq.astype(np.float64)).max() <= ulp, (q, a, dq, odq)
    assert abs(float(cost) - float(ocost)) <= ulp, (cost, ocost)
    return dq, cost


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("A", list(range(1, 19)))
def test_host_restatement_against_the_oracle_at_every_width(A, clip):
    rng = np.random.RandomState(100 + A)
    for trial in range(8):
        q = (rng.randn(A) * 3).astype(np.float32)
        a, y = int(rng.randint(A)), float(rng.randn() * 3)
        for w in (1.0, 0.37, 2.5):
            dq, cost = _same(q, a, y, 1.0, clip, w)
            d = np.float32(q[a] - np.float32(y))
            if clip:
                assert abs(float(dq[a])) <= w * (clip + 1.0) * (1 + 1e-6)       # the TD part is clipped, the regulariser lies in [-alpha, 0]
            if A == 1:                                           # pi = exp(0) = 1 exactly: dq == w dc bit for bit, the cost the standard head's
                dc = np.float32(min(max(d, np.float32(-clip)), np.float32(clip))) if clip else d
                assert dq[0].tobytes() == np.float32(np.float32(w) * dc).tobytes()
                assert np.float32(cost).tobytes() == np.float32(np.float32(w) * np.float32(np.float32(0.5) * np.float32(d * d))).tobytes()


def test_host_restatement_on_tied_rows_and_far_apart_rows():
    for A in (2, 3, 4, 7, 18):
        q = np.full(A, 1.25, np.float32)                         # exactly tied: pi = 1 / A
        dq, cost = _same(q, 0, 1.25, 1.0, 1.0, 1.0)
        assert np.allclose(dq[1:], 1.0 / A, rtol=1e-6) and np.isclose(dq[0], 1.0 / A - 1.0, rtol=1e-6)
        assert np.isclose(cost, math.log(A), rtol=1e-6)          # delta = 0: the cost is alpha log A
    for gap in (1e3, 1e4):
        for a in (0, 1, 2):
            q = np.array([gap, 0.0, -gap, 0.5], np.float32)      # pi underflows to 0 off the maximum: no NaN, no inf
            for clip in (0.0, 1.0):
                dq, cost = _same(q, a, 0.25, 1.0, clip, 1.7)
                assert all(dq[k] == 0.0 for k in (1, 2, 3) if k != a)
                if a != 0:
                    assert dq[0] == np.float32(1.7)              # w alpha (pi[0] - 0), pi[0] = 1


def test_oracle_alpha_zero_and_one_action_equal_the_parent_to_rounding():
    """(bit identity of the library's step is held on the GPU, tests/test_gpu_cql.py; the oracle hands dq to its parent as
    preq - (preq - dq), one rounding of |q| in float64 away)"""
    def small(cls, A, B, **attrs):
        ws, wt = xavier_weights(A, 3, np.float64, *GEOM), xavier_weights(A, 103, np.float64, *GEOM)
        o = cls(A, batch_size=B, history_length=GEOM[0], screen_height=GEOM[1], screen_width=GEOM[2], dtype=np.float64, weights=ws)
        o.Wt = [w.copy() for w in wt]
        for k, v in attrs.items():
            setattr(o, k, v)
        return o

    def mb(B, A, seed):
        rng = np.random.RandomState(seed)
        pre = rng.randint(0, 256, (B,) + GEOM, dtype=np.uint8)
        post = rng.randint(0, 256, (B,) + GEOM, dtype=np.uint8)
        return pre, rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64), post, rng.rand(B) < 0.25

    for A, alpha in ((4, 0.0), (1, 1.0)):
        m = mb(5, A, A)
        g0 = small(OracleDQN, A, 5).gradients(m)
        o = small(CO.CQLOracle, A, 5, cql_alpha=alpha)
        g1 = o.gradients(m)
        assert np.abs(g0[1] - g1[1]) <= 1e-15 * max(1.0, abs(g0[1]))
        for a, b in zip(g0[0], g1[0]):                           # (the oracle restates dq as preq - (preq - dq): one rounding of |q| in float64)
            assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(a).max())
    # and with alpha > 0 every fc5 row carries gradient
    o = small(CO.CQLOracle, 4, 5, cql_alpha=1.0)
    g = o.gradients(mb(5, 4, 9))[0]
    assert (np.abs(o.last_dq) > 0).all() and (np.abs(g[4]).max(axis=1) > 0).all()


def test_isa_census_of_the_cql_heads():
    """every CQL head: no scratch, 12 kernels (3 buckets x {plain, PER} x {one-step, n-step}), and registers that keep two 512-thread
    workgroups on a CU as the standard head's do; LDS and VGPRs per bucket are printed (DESIGN.md §35 records them)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = [r for r in isa_census.census_rows("sdqn_cql.hip") if "cql_head_kernel" in r["name"]]
    assert len(rows) == 12, [r["name"] for r in rows]
    for bucket in (4, 8, 18):
        mine = [r for r in rows if "cql_head_kernelILi%dE" % bucket in r["name"]]
        assert len(mine) == 4, (bucket, [r["name"] for r in mine])
        for r in mine:
            print("%s: vgpr %d agpr %d lds %d scratch %d" % (r["name"][:64], r["vgpr"], r["agpr"], r["lds"], r["scratch"]))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] == (2 * bucket * 512 + 3 * bucket) * 4, (r["name"], r["lds"])      # prod[][] + sh_q[2][] + sh_dq[]
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])
