"""--advantage_learning / --persistent_advantage without a device: the oracle's targets on hand-computed rows, one step's
gradients against finite differences of the loss, the command line and its refusals, the C ABI symbols, and the compiler's resource
report of the advantage-learning head kernels."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
import advantage_oracle as AO  # noqa: E402
from oracle.dqn_numpy import OracleDQN, xavier_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = (2, 64, 48)                 # the smallest screen the tests of the generic path use
GAMMA, ALPHA = 0.99, 0.9


class _Rows(AO._AdvantageLearning, OracleDQN):
    """td_targets on Q rows given by hand: no forward pass"""

    def __init__(self, A, qpre, qpost, **attrs):
        OracleDQN.__init__(self, A, batch_size=len(qpre), history_length=GEOM[0], screen_height=GEOM[1], screen_width=GEOM[2],
                           dtype=np.float64, discount_rate=GAMMA)
        self.last_pre_target_q, self.last_post_target_q = np.array(qpre, np.float64), np.array(qpost, np.float64)
        for k, v in attrs.items():
            setattr(self, k, v)

    def y(self, actions, rewards, terminals):
        n = len(actions)
        preq = np.zeros((n, self.num_actions))
        t = self.td_targets(preq, self.last_post_target_q.max(axis=1), np.array(actions), np.array(rewards), np.array(terminals))
        return t[np.arange(n), actions]


# qbar(s), qbar(s'), a, r, terminal
QPRE = [[1.0, 3.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.25, 0.0], [0.5, 0.25, 0.0], [2.0, 2.0, -1.0]]
QPOST = [[0.0, 4.0, 1.0], [4.0, 0.0, 1.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.0, 5.0, 3.0]]
ACT = [1, 0, 2, 1, 1]
REW = [1, 0, -3, 1, 2]             # clipped to [-1, 1]: 1, 0, -1, 1, 1
TERM = [False, False, False, True, False]


def test_gap_is_zero_on_a_maximiser_and_positive_elsewhere():
    g = AO.gap(QPRE, ACT)
    assert np.array_equal(g, np.array([0.0, 2.0, 0.5, 0.25, 0.0])) and not np.signbit(g).any()
    assert np.array_equal(AO.gap(QPOST, ACT), np.array([0.0, 0.0, 0.5, 0.0, 0.0]))


def test_al_targets_on_hand_computed_rows():
    y = _Rows(3, QPRE, QPOST, advantage_learning=ALPHA).y(ACT, REW, TERM)
    ystd = np.array([1 + GAMMA * 4.0, 0 + GAMMA * 4.0, -1 + GAMMA * 1.0, 1.0, 1 + GAMMA * 5.0])
    want = ystd - ALPHA * np.array([0.0, 2.0, 0.5, 0.25, 0.0])          # the terminal row loses its gap too
    assert np.abs(y - want).max() <= 1e-12, (y, want)


def test_pal_takes_each_branch_and_equals_al_on_terminal_rows():
    qpost = [[0.0, 4.0, 1.0], [4.0, 0.0, 1.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.0, 2.0, 3.0]]
    qpre = [[1.0, 3.0, 2.0], [1.0, 3.0, 2.0], [0.5, 0.25, 0.25], [0.5, 0.25, 0.0], [2.0, 2.0, -1.0]]
    o = _Rows(3, qpre, qpost, advantage_learning=ALPHA, persistent_advantage=True)
    y = o.y(ACT, REW, TERM)
    gpre, gpost = np.array([0.0, 2.0, 0.25, 0.25, 0.0]), np.array([0.0, 0.0, 0.5, 0.0, 1.0])
    ystd = np.array([1 + GAMMA * 4.0, 0 + GAMMA * 4.0, -1 + GAMMA * 1.0, 1.0, 1 + GAMMA * 3.0])
    al = ystd - ALPHA * gpre
    # row 0: both gaps 0 (either branch, same value); row 1: the poststate's gap is smaller -> that branch; rows 2 and 4: the prestate's gap
    # is smaller -> y_AL; row 3: terminal -> y_AL although the poststate's gap (0) is smaller
    want = np.array([al[0], ystd[1] - ALPHA * gpost[1], al[2], al[3], al[4]])
    assert np.abs(y - want).max() <= 1e-12, (y, want)
    assert list(o.last_pal_took_post) == [False, True, False, False, False]
    assert np.array_equal(o.last_gap_pre, gpre) and np.array_equal(o.last_gap_post, gpost)
    assert np.abs(o.last_y - want).max() <= 1e-12 and np.abs(o.last_y_std - ystd).max() <= 1e-12
    # PAL never lies below AL, and equals it on every terminal row
    o2 = _Rows(3, qpre, qpost, advantage_learning=ALPHA, persistent_advantage=True)
    yt = o2.y(ACT, REW, [True] * 5)
    at = _Rows(3, qpre, qpost, advantage_learning=ALPHA).y(ACT, REW, [True] * 5)
    assert np.array_equal(yt, at) and not o2.last_pal_took_post.any()
    assert (y >= al - 1e-15).all()


def _mb(B, A, seed, p_term=0.25):
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, (B,) + GEOM, dtype=np.uint8)
    post = rng.randint(0, 256, (B,) + GEOM, dtype=np.uint8)
    return pre, rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64), post, rng.rand(B) < p_term


def _small(cls, A, B, **attrs):
    ws, wt = xavier_weights(A, 3, np.float64, *GEOM), xavier_weights(A, 103, np.float64, *GEOM)
    o = cls(A, batch_size=B, history_length=GEOM[0], screen_height=GEOM[1], screen_width=GEOM[2], dtype=np.float64, weights=ws)
    o.Wt = [w.copy() for w in wt]
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("pal", [False, True])
def test_alpha_zero_and_one_action_equal_the_parent_bit_for_bit(pal):
    mb = _mb(5, 4, 1)
    g0 = _small(OracleDQN, 4, 5).gradients(mb)
    g1 = _small(AO.AdvantageOracle, 4, 5, advantage_learning=0.0, persistent_advantage=pal).gradients(mb)
    for a, b in zip(g0[0], g1[0]):
        assert np.array_equal(a, b)
    assert g0[1] == g1[1] and np.array_equal(g0[2], g1[2])
    mb1 = _mb(5, 1, 2)
    g0 = _small(OracleDQN, 1, 5).gradients(mb1)
    o = _small(AO.AdvantageOracle, 1, 5, advantage_learning=ALPHA, persistent_advantage=pal)
    g1 = o.gradients(mb1)
    assert np.array_equal(o.last_gap_pre, np.zeros(5)) and np.array_equal(o.last_y, o.last_y_std)
    for a, b in zip(g0[0], g1[0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("pal", [False, True])
def test_gradients_equal_finite_differences_of_the_loss(pal):
    """L(W) = sum_n 0.5 (Q(W, s_n)[a_n] - y_n)^2 with y held fixed (the targets are constants of the step), no error clip: central differences
    in float64 on the largest-gradient entries of every layer"""
    A, B = 4, 5
    mb = _mb(B, A, 4)
    o = _small(AO.AdvantageOracle, A, B, advantage_learning=ALPHA, persistent_advantage=pal, clip_error=0)
    g = o.gradients(mb)[0]
    y, x, n, a = o.last_y.copy(), o._normalize(mb[0]), np.arange(B), mb[1].astype(np.int64)
    assert (np.abs(y - o.last_y_std) > 1e-3).any()               # the targets are not the parent's

    def loss():
        q = o.fprop(o.W, x)
        return float((0.5 * (q[n, a] - y) ** 2).sum())

    for li in range(5):
        flat, gf = o.W[li].reshape(-1), np.asarray(g[li]).reshape(-1)
        for i in np.argsort(-np.abs(gf))[:3]:
            w0, h = flat[i], 1e-6
            flat[i] = w0 + h; lp = loss()
            flat[i] = w0 - h; lm = loss()
            flat[i] = w0
            fd = (lp - lm) / (2 * h)
            assert abs(fd - gf[i]) <= 1e-6 * max(1.0, abs(gf[i])), (li, i, fd, gf[i])


def test_parser_defaults_and_refusals_before_any_device_call():
    from simple_dqn_amd import main
    d = main.build_parser().parse_args([])
    assert d.advantage_learning == 0.0 and d.persistent_advantage is False
    assert main.check_advantage_learning(d) == (0.0, False)
    on = main.build_parser().parse_args(["--advantage_learning", "0.9", "--persistent_advantage", "true", "--prioritized_replay", "true",
                                         "--target_tau", "0.01", "--clip_grad_norm", "10"])
    assert main.check_advantage_learning(on) == (0.9, True)
    assert main.check_advantage_learning(main.build_parser().parse_args(["--advantage_learning", "0.5", "--n_step", "3"])) == (0.5, False)
    base = ["--random_steps", "0", "--epochs", "0"]
    al = ["--advantage_learning", "0.9"]
    for extra, words in ((["--advantage_learning", "1"], ("--advantage_learning",)),
                         (["--advantage_learning", "-0.1"], ("--advantage_learning",)),
                         (["--advantage_learning", "nan"], ("--advantage_learning",)),
                         (["--persistent_advantage", "true"], ("--persistent_advantage", "--advantage_learning")),
                         (al + ["--persistent_advantage", "true", "--n_step", "2"], ("--persistent_advantage", "--n_step")),
                         (al + ["--double_dqn", "true"], ("--advantage_learning", "--double_dqn")),
                         (al + ["--munchausen", "true"], ("--advantage_learning", "--munchausen")),
                         (al + ["--bootstrap_heads", "2"], ("--advantage_learning", "--bootstrap_heads")),
                         (al + ["--batch_norm", "true"], ("--advantage_learning", "--batch_norm"))):
        args = main.build_parser().parse_args(base + extra)
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never this ValueError
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
        with pytest.raises(ValueError) as ei:                    # DeepQNetwork refuses by the same words, before it loads the library
            sd.DeepQNetwork(4, args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
    # with alpha = 0 the other options are nobody's business
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true", "--n_step", "3"])
    assert main.check_advantage_learning(off) == (0.0, False)


def test_symbols_in_signatures_and_library():
    for name in ("sdqn_net_set_advantage_learning", "sdqn_net_get_advantage_learning"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name), name
        assert name in open(os.path.join(ROOT, "include", "sdqn.h")).read()


def test_isa_census_of_the_advantage_heads():
    """every advantage-learning head: no scratch, and per action bucket no more LDS and no more VGPRs than the Munchausen heads of that
    bucket (the largest of its four), so the 512-thread workgroup's residency is theirs; the PAL choice is a run-time branch: 12 kernels"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    al = [r for r in isa_census.census_rows("sdqn_advantage.hip") if "advantage_head_kernel" in r["name"]]
    mu = [r for r in isa_census.census_rows("sdqn_munchausen.hip") if "munchausen_head_kernel" in r["name"]]
    assert len(al) == 12, [r["name"] for r in al]           # 3 buckets x {plain, PER} x {one-step, n-step}
    for bucket in (4, 8, 18):
        ref = [r for r in mu if "munchausen_head_kernelILi%dE" % bucket in r["name"]]
        mine = [r for r in al if "advantage_head_kernelILi%dE" % bucket in r["name"]]
        assert len(ref) == 4 and len(mine) == 4, (bucket, [r["name"] for r in mine])
        for r in mine:
            frag = re.search(r"head_kernelILi\d+ELb[01]ELb[01]E", r["name"]).group(0)
            twin = [m for m in ref if frag in m["name"]]        # the Munchausen head of the same (bucket, PER, NSTEP)
            assert len(twin) == 1, (frag, [m["name"] for m in ref])
            lds, vgpr = twin[0]["lds"], twin[0]["vgpr"] + twin[0]["agpr"]
            print("%s: vgpr %d lds %d scratch %d (munchausen: vgpr %d lds %d)" % (r["name"][:60], r["vgpr"], r["lds"], r["scratch"], vgpr, lds))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] <= lds, (r["name"], r["lds"], lds)
            assert r["vgpr"] + r["agpr"] <= vgpr, (r["name"], r["vgpr"], vgpr)
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])     # two 512-thread workgroups per CU, as the standard head
