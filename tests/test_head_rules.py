"""The TD head's rule headers (td_rule.h, munchausen.h, advantage.h, bootstrap.h) on the CPU, against the Python oracles.
tests/emul/head_rules.cpp includes the headers and runs each rule on float and double rows, composed as generic_net.hip's head_kernel
composes them; the oracles' td_targets methods run on the same rows (the oracle classes without a network: only the attributes td_targets
reads).  The bootstrap oracle computes its targets inside gradients(), behind a forward pass, so its lines (bootstrap_oracle.py:101-121) are
restated here over bootstrap_oracle.mask.
Tolerances are the project's for the generic path against these oracles: 1e-9 for double rows (test_gpu_double_dqn.py f64_b8,
test_gpu_per.py, test_gpu_generic.py), 1e-5 for float rows (test_gpu_generic.py's float32 bound on Q).  Every branch the inputs are meant to
reach is asserted on the oracle's side before anything is compared."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import bootstrap_oracle as BO
from advantage_oracle import _AdvantageLearning
from double_dqn_oracle import _DoubleDQN
from munchausen_oracle import _Munchausen
from nstep_oracle import _NStep, gamma_n
from oracle.dqn_numpy import OracleDQN
from per_oracle import _PER, new_priority

B, GAMMA, MINR, MAXR = 8, 0.99, -1.0, 1.0
ALPHA_PER, EPS_PER = 0.6, 1e-6
TOL = {np.float64: 1e-9, np.float32: 1e-5}
SUF = {np.float64: "d", np.float32: "f"}


@pytest.fixture(scope="module")
def rules():
    so = os.path.join(HERE, "emul", "libsdqn_head_rules.so")
    src = os.path.join(HERE, "emul", "head_rules.cpp")
    hdrs = [os.path.join(HERE, "..", "simple_dqn_amd", "csrc", h) for h in ("td_rule.h", "munchausen.h", "advantage.h", "bootstrap.h", "env_catch.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _common(act, rew, term, n):
    """the arguments every entry point takes behind its rows: metadata, n_step, discount, gamma^n, reward clip"""
    return [_p(act), _p(rew), _p(term), C.c_int(n), C.c_double(GAMMA), C.c_double(gamma_n(n, GAMMA)), C.c_double(MINR), C.c_double(MAXR)]


def _inputs(A, dt, n, seed=20):
    """B samples: rows, actions, rewards (ints outside the clip range too, or n-step returns as float64 bits), terminals 0 and 3"""
    rng = np.random.RandomState(seed + A)
    pre, post, sel, mu = [(rng.standard_normal((B, A)) * 0.3).astype(dt) for _ in range(4)]
    act = rng.randint(0, A, B).astype(np.int32)
    term = np.zeros(B, np.int32); term[[0, 3]] = 1
    if n > 1:
        R = rng.uniform(-0.8, 0.8, B)
        rew = np.array([struct.unpack("<q", struct.pack("<d", float(x)))[0] for x in R], np.int64)
        return pre, post, sel, mu, act, rew, R, term
    rew = rng.randint(-3, 4, B).astype(np.int64)
    return pre, post, sel, mu, act, rew, rew, term


def _stub(cls, dt, n):
    o = object.__new__(cls)
    o.dtype, o.discount_rate, o.min_reward, o.max_reward, o.n_step = dt, GAMMA, MINR, MAXR, n
    return o


class _TD(_PER, _DoubleDQN, _NStep, OracleDQN):
    pass


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("A", [1, 2, 4, 18])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_standard_double_per_tail(rules, dt, A, n, double, clip):
    pre, post, sel, _, act, rew, r_oracle, term = _inputs(A, dt, n)
    pre[1, act[1]] += dt(5)                                   # an error outside the clip
    w = np.linspace(0.25, 1.0, B).astype(np.float32)           # PER weights != 1
    assert (w != 1).sum() >= B - 1 and term.any() and not term.all()
    o = _stub(_TD, dt, n)
    o._clip, o.weights = clip, w
    o.last_online_postq, o.last_target_postq = (sel, post) if double else (None, None)
    t = o.td_targets(pre, post.max(axis=1), act, r_oracle, term.astype(bool))
    rows = np.arange(B)
    dq_ref = pre[rows, act] - t[rows, act]
    absd = o.last_abs_delta.astype(np.float64)
    if clip:
        assert (absd > clip).any() and (absd < clip).any()   # inside and outside the clip
    dq, cost, maxq, prio, y = np.zeros((B, A), dt), np.zeros(B, dt), np.zeros(B, dt), np.zeros(B, np.float32), np.zeros(B)
    getattr(rules, "hr_td_" + SUF[dt])(_p(pre), _p(post), _p(sel) if double else None, B, A, *_common(act, rew, term, n), C.c_double(clip), _p(w),
                                       C.c_double(ALPHA_PER), C.c_double(EPS_PER), _p(dq), _p(cost), _p(maxq), _p(prio), _p(y))
    tol = TOL[dt]
    assert np.abs(maxq - o.last_maxpostq).max() == 0
    assert np.abs(dq[rows, act] - dq_ref).max() <= tol
    off = dq.copy(); off[rows, act] = 0
    assert not off.any()
    assert abs(float(cost.astype(np.float64).mean()) - float(o._per_cost)) <= tol
    np.testing.assert_allclose(prio, new_priority(absd, ALPHA_PER, EPS_PER), rtol=1e-6)       # (test_gpu_per.py's bound on a float32 priority)
    # without PER: the parent's rule, deltas and cost before the weight
    o2 = _stub(_TD, dt, n)
    o2._clip, o2.weights = clip, None
    o2.last_online_postq, o2.last_target_postq = o.last_online_postq, o.last_target_postq
    t2 = o2.td_targets(pre, post.max(axis=1), act, r_oracle, term.astype(bool))
    getattr(rules, "hr_td_" + SUF[dt])(_p(pre), _p(post), _p(sel) if double else None, B, A, *_common(act, rew, term, n), C.c_double(clip), None,
                                       C.c_double(0.0), C.c_double(0.0), _p(dq), _p(cost), _p(maxq), _p(prio), _p(y))
    assert np.abs(dq[rows, act] - (pre[rows, act] - t2[rows, act])).max() <= tol
    assert abs(float(cost.astype(np.float64).mean()) - float(o2._per_cost)) <= tol


class _Mu(_Munchausen, OracleDQN):
    pass


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("A", [1, 2, 4, 18])
@pytest.mark.parametrize("n", [1, 3])
def test_munchausen_target(rules, dt, A, n):
    alpha, tau, l0 = 0.9, 0.03, -0.05
    pre, post, _, mu, act, rew, r_oracle, term = _inputs(A, dt, n)
    if A >= 2:
        a1, a2 = int(act[1]), int(act[2])
        mu[1, :] = dt(-3); mu[1, a1] = dt(10)                 # the unique maximiser far above the rest: the log-policy term is exactly 0
        mu[2, :] = dt(-3); mu[2, a2] = dt(0.48); mu[2, (a2 + 1) % A] = dt(0.5)      # a near-maximiser: strictly between l0 and 0
        a4 = int(act[4])
        mu[4, :] = dt(0); mu[4, (a4 + 1) % A] = dt(1)         # far below the maximum: clipped at l0
    o = _stub(_Mu, dt, n)
    o.munchausen_alpha, o.munchausen_tau, o.munchausen_clip = alpha, tau, l0
    o.last_pre_target_q, o.last_post_target_q = mu, post
    o.td_targets(pre, None, act, r_oracle, term.astype(bool))
    lp = o.last_bonus / alpha
    if A >= 2:
        assert lp[1] == 0.0 and l0 < lp[2] < 0.0 and o.last_bonus[4] == alpha * l0
    else:
        assert (lp == 0.0).all()                              # A = 1: lse == q[0] exactly
    assert term.any() and not term.all()
    y, V, bonus = np.zeros(B), np.zeros(B), np.zeros(B)
    getattr(rules, "hr_munchausen_" + SUF[dt])(_p(mu), _p(post), B, A, *_common(act, rew, term, n), C.c_double(alpha), C.c_double(tau), C.c_double(l0),
                                               _p(y), _p(V), _p(bonus))
    tol = TOL[dt]
    assert np.abs(V - o.last_V).max() <= tol and np.abs(bonus - o.last_bonus).max() <= tol and np.abs(y - o.last_y).max() <= tol


class _AL(_AdvantageLearning, OracleDQN):
    pass


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("A", [1, 2, 4, 18])
@pytest.mark.parametrize("n,persistent", [(1, False), (3, False), (1, True)])
def test_advantage_target(rules, dt, A, n, persistent):
    alpha = 0.9
    pre, post, _, mu, act, rew, r_oracle, term = _inputs(A, dt, n)
    if A >= 2:
        a1, a2 = int(act[1]), int(act[2])
        mu[1, :] = dt(0); mu[1, (a1 + 1) % A] = dt(2); post[1, :] = dt(0.1)       # large gap now, none in s': PAL takes the poststate's target
        mu[2, :] = dt(0); mu[2, a2] = dt(1); post[2, :] = dt(0); post[2, (a2 + 1) % A] = dt(2)      # no gap now, a large one in s': PAL keeps y_AL
        mu[0, :] = dt(0); mu[0, (int(act[0]) + 1) % A] = dt(2); post[0, :] = dt(0.1)                 # as sample 1, but terminal
    o = _stub(_AL, dt, n)
    o.advantage_learning, o.persistent_advantage = alpha, persistent
    o.last_pre_target_q, o.last_post_target_q = mu, post
    o.td_targets(pre, post.max(axis=1), act, r_oracle, term.astype(bool))
    took = o.last_pal_took_post
    if persistent and A >= 2:
        assert took[1] and not took[2] and term[0] and not took[0]      # each of PAL's two targets, and PAL on a terminal sample
    else:
        assert not took.any()
    y, maxq = np.zeros(B), np.zeros(B, dt)
    getattr(rules, "hr_advantage_" + SUF[dt])(_p(mu), _p(post), B, A, *_common(act, rew, term, n), C.c_double(alpha), int(persistent), _p(y), _p(maxq))
    assert np.abs(maxq - post.max(axis=1)).max() == 0
    assert np.abs(y - o.last_y).max() <= TOL[dt]


def _bootstrap_reference(pre, post, K, A, act, r, term, gam, clip, masks, dt):
    """bootstrap_oracle.py:101-121 on given rows"""
    N = len(act)
    targets, live, maxq = pre.copy(), np.zeros(pre.shape, bool), np.zeros(N)
    for s in range(N):
        for k in range(K):
            mk = float(post[s, k * A:(k + 1) * A].max())
            maxq[s] += mk
            targets[s, k * A + int(act[s])] = r[s] if term[s] else r[s] + gam * mk
            live[s, k * A + int(act[s])] = bool(masks[s, k])
        maxq[s] /= K
    deltas = pre - targets.astype(dt)
    terms = (0.5 * (np.where(live, deltas, dt(0)) ** 2).sum(axis=1) / dt(K)).astype(dt)
    if clip:
        deltas = np.clip(deltas, -clip, clip).astype(dt)
    return (np.where(live, deltas, dt(0)) / dt(K)).astype(dt), terms, maxq, np.abs(pre - targets.astype(dt))[live]


@pytest.mark.parametrize("dt,fn", [(np.float64, "hr_bootstrap_d"), (np.float32, "hr_bootstrap_f"), (np.float32, "hr_bootstrap_fminmax_f")])
@pytest.mark.parametrize("K,A,P", [(1, 4, 1.0), (6, 3, 0.5), (2, 1, 0.5), (1, 18, 1.0)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_bootstrap_sample(rules, dt, fn, K, A, P, n, clip):
    seed = 5
    _, _, _, _, act, rew, r_oracle, term = _inputs(A, dt, n)
    rng = np.random.RandomState(31 + K)
    pre, post = [(rng.standard_normal((B, K * A)) * 0.3).astype(dt) for _ in range(2)]
    pre[1, np.arange(K) * A + act[1]] += dt(5)               # errors outside the clip
    all_masks = {i: BO.mask(seed, P, K, i) for i in range(400)}
    dead = [i for i, m in all_masks.items() if not m.any()]
    full = [i for i, m in all_masks.items() if m.all()]
    if P < 1.0:
        assert dead and full                                  # a sample whose masks are all dead, one whose masks are all live
        idx = np.array([dead[0], full[0]] + list(range(10, 10 + B - 2)), np.int64)
    else:
        idx = np.arange(B, dtype=np.int64)
    masks = np.stack([all_masks[int(i)] for i in idx])
    r = [float(x) for x in (r_oracle if n > 1 else np.clip(r_oracle, MINR, MAXR))]
    dq_ref, terms_ref, maxq_ref, absd = _bootstrap_reference(pre, post, K, A, act, r, term, gamma_n(n, GAMMA) if n > 1 else GAMMA, clip, masks, dt)
    if clip:
        assert (absd > clip).any() and (absd < clip).any()
    assert term.any() and not term.all()
    dq, cost, maxq, rows = np.zeros((B, K * A), dt), np.zeros(B, dt), np.zeros(B, dt), np.zeros(B, np.int32)
    getattr(rules, fn)(_p(pre), _p(post), B, K, A, *_common(act, rew, term, n), C.c_double(clip), C.c_uint64(seed), C.c_uint64(BO.threshold(P)), _p(idx),
                       _p(dq), _p(cost), _p(maxq), _p(rows))
    tol = TOL[dt]
    assert np.abs(dq - dq_ref).max() <= tol and np.abs(cost - terms_ref).max() <= tol and np.abs(maxq - maxq_ref.astype(dt)).max() <= tol
    for s in range(B):                                        # the row mask names exactly the live taken-action rows
        assert int(rows[s]) == sum(1 << (k * A + int(act[s])) for k in range(K) if masks[s, k])
    if P < 1.0:
        assert not dq[0].any() and cost[0] == 0 and rows[0] == 0
