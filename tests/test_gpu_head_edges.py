"""The head kernel (fc5 of both nets, bootstrap value, TD target, clip, fc5 dgrad) and the fc5 part of the optimizer pass at the inputs
where they branch, against the numpy oracles.

  A. action counts: A = 1 (legal, never run before), 7 | 8 | 9 (the A <= 8 bucket edge), 17 — one whole plain step, every head variant
     (--double_dqn, --n_step, --prioritized_replay, float16, --batch_norm), the generic path and the one-launch acting forward;
  B. exact ties in the Double DQN action choice: the rule is numpy argmax's FIRST maximum, which no test with random weights can see;
  C. degenerate minibatches: all / no terminals, one action throughout, every reward clipped on one side, clip_error = 0 with |delta| ~ 5,
     all-zero prestates (every gradient exactly zero) and the sparse frames of the library's own game.

Everything is at the smallest shape that enters the branch (B = 8 unless the regime is the point) and at the bound the existing one-step
test of the same configuration uses."""
import random

import numpy as np
import pytest

import nstep_oracle as N
import per_oracle as P
from catch_oracle import CatchOracle
from double_dqn_oracle import DoubleDQNOracle, DoubleDQNOracleBN
from oracle.dqn_numpy import OracleDQN, _im2col, xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4          # tests/test_gpu_dqn.py
H_TOL = 3e-3          # tests/test_gpu_dqn.py, float16 mode


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


class _Capture:
    """keeps the bootstrap values the step used (last_maxpostq)"""
    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        self.last_maxpostq = np.array(maxpostq)
        return super().td_targets(preq, maxpostq, actions, rewards, terminals)


class _Oracle(_Capture, OracleDQN):
    pass


def _costs(net):
    costs = []
    net.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
    return costs


def _pair(sd, A, B, seed, half=False, **kw):
    """a net and its oracle (float32, or float16 with the half oracle) from the same two Xavier draws"""
    args = make_args(batch_size=B, datatype="float16" if half else "float32", **kw)
    net = sd.DeepQNetwork(A, args)
    ws, wt = xavier_weights(A, seed), xavier_weights(A, seed + 1)
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    o = _Oracle(A, batch_size=B, weights=ws, clip_error=args.clip_error, min_reward=args.min_reward, max_reward=args.max_reward,
                half_activations=half)
    o.Wt = [w.copy() for w in wt]
    return net, o


def _step_check(net, o, mb, half=False, update=True):
    """One whole step against the oracle.  float32: the bounds of test_one_step_gradients_and_update (Q and max-Q 1e-4, cost 1e-5, every
    gradient element 1e-4 of the layer's largest, weights 2e-5 where the gradient is not round-off-small, RMSProp state 1e-3);
    float16: those of test_fp16_one_step_gradients (Q 3e-3, cost 5e-3, gradients 5e-2 in relative norm and 1.5e-1 of the largest)."""
    B = mb[0].shape[0]
    net.set_option("keep_gradients", 1)
    costs = _costs(net)
    g, cost, _, preq = o.gradients(mb)
    net.train(mb)
    q, mq = net.last_q()
    qtol = H_TOL if half else Q_TOL
    assert q.shape == preq.shape
    eq, em = np.abs(q - preq).max(), np.abs(mq - o.last_maxpostq).max()
    ec = abs(costs[0] - float(cost)) / max(1.0, float(cost))
    print("Q max abs err %.3e, max-Q %.3e, cost rel err %.3e" % (eq, em, ec))
    assert eq < qtol and em < qtol
    assert ec < (5e-3 if half else 1e-5)
    for i in range(5):
        gg = net.get_layer(i, which=3)
        mx = np.abs(gg - g[i]).max()
        fro = float(np.linalg.norm(gg - g[i]) / max(1e-12, np.linalg.norm(g[i])))
        print("layer %d: grad max abs err %.3e (max |g| %.3e), rel norm %.3e" % (i, mx, np.abs(g[i]).max(), fro))
        if half:
            assert fro < 5e-2 and mx / max(1e-6, np.abs(g[i]).max()) < 1.5e-1, i
        else:
            assert mx < 1e-4 * max(1e-3, np.abs(g[i]).max()), "grad layer %d" % i
    if update and not half:
        o.rmsprop(g, B)
        for i in range(5):
            big = np.abs(g[i]) / B > 1e-6
            if big.any():
                assert np.abs(net.get_layer(i, 0) - o.W[i])[big].max() < 2e-5, "weights layer %d" % i
            assert np.abs(net.get_layer(i, 2) - o.S[i]).max() < 1e-6 + 1e-3 * np.abs(o.S[i]).max(), "state layer %d" % i
    assert net.train_iterations == 1


# ---- A. action counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", [(1, 8), (7, 8), (8, 8), (9, 8), (17, 8), (1, 32), (9, 32)])
def test_plain_step_action_counts(sd, A, B):
    """Q of the prestates, max-Q, cost, the five gradients and the weights and RMSProp state after the update: A = 1 (the action loops
    run once, fc5's optimizer workgroups are 4), 7 / 8 (last of the A <= 8 head) and 9 (first of the A <= 18 head), 17."""
    net, o = _pair(sd, A, B, 700 + A)
    _step_check(net, o, random_minibatch(B, A, 710 + A, reward_range=(-3, 4)))


@pytest.mark.parametrize("A", [1, 8, 9])
def test_float16_step_action_counts(sd, A):
    net, o = _pair(sd, A, 8, 720 + A, half=True)
    _step_check(net, o, random_minibatch(8, A, 730 + A, reward_range=(-2, 3)), half=True)


@pytest.mark.parametrize("A", [1, 8, 9, 17])
def test_double_dqn_step_action_counts(sd, A):
    """--double_dqn: the third net slot of the head (108 KB of LDS at A = 17 / 18) — Q, the bootstrap value and the gradients at the
    bounds of tests/test_gpu_double_dqn.py's one-step test.  With one action the choice is trivial and the step is the standard one."""
    from test_gpu_double_dqn import _check_maxpostq, _follow
    B = 8
    mb = random_minibatch(B, A, 740 + A)
    ws, wt = xavier_weights(A, 741 + A), xavier_weights(A, 841 + A)
    net = sd.DeepQNetwork(A, make_args(batch_size=B, double_dqn=True))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.set_option("keep_gradients", 1)
    o = DoubleDQNOracle(A, batch_size=B, weights=ws)
    o.Wt = [w.copy() for w in wt]
    net.train(mb)
    q, mq = net.last_q()
    o.choose = _follow(mq, Q_TOL) if A > 1 else None                   # (a top-2 gap within round-off may go either way: as the device went)
    g, _, _, preq = o.gradients(mb)
    if A > 1:
        differ = o.last_online_postq.argmax(1) != o.last_target_postq.argmax(1)
        assert differ.any()                                            # a library that ignored the option would fail below
        assert np.abs(o.last_maxpostq - o.last_target_postq.max(1)).max() > Q_TOL
    assert np.abs(q - preq).max() < Q_TOL * max(1.0, float(np.abs(preq).max()))
    if A > 1:
        _check_maxpostq(mq, o, Q_TOL)
    else:                                                              # (no second candidate to accept)
        assert np.abs(mq - o.last_maxpostq).max() <= Q_TOL * max(1.0, float(np.abs(o.last_target_postq).max()))
    for i in range(5):
        assert np.abs(net.get_layer(i, 3) - g[i]).max() < 1e-4 * max(1e-3, np.abs(g[i]).max()), i


@pytest.mark.parametrize("A", [1, 8, 9])
def test_n_step_action_counts(sd, A):
    """--n_step 3 through the tuple API: float64 returns R, done flags, bootstrap factor gamma^3 — the bounds of tests/test_gpu_nstep.py"""
    B, n = 8, 3
    pre, act, _, post, done = random_minibatch(B, A, 750 + A)
    r = np.random.RandomState(751 + A).randint(-1, 2, (B, n)).astype(np.float64)
    R = r[:, 0] + 0.99 * r[:, 1] + (0.99 * 0.99) * r[:, 2]
    mb = (pre, act, R, post, done)
    ws, wt = xavier_weights(A, 752 + A), xavier_weights(A, 852 + A)
    net = sd.DeepQNetwork(A, make_args(batch_size=B, n_step=n))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.set_option("keep_gradients", 1)
    o = N.NStepOracle(A, batch_size=B, weights=ws)
    o.Wt = [w.copy() for w in wt]
    o.n_step = n
    g, _, _, preq = o.gradients(mb)
    net.train(mb)
    q, mq = net.last_q()
    ref = o.fprop(o.Wt, o._normalize(post)).max(1)
    assert np.abs(q - preq).max() < Q_TOL * max(1.0, float(np.abs(preq).max()))
    assert np.abs(mq - ref).max() < Q_TOL * max(1.0, float(np.abs(ref).max()))
    for i in range(5):
        assert np.abs(net.get_layer(i, 3) - g[i]).max() < 1e-4 * max(1e-3, np.abs(g[i]).max()), i


def _per_fixture(size, A, seed=3):
    """the ring content and raw priorities of tests/test_gpu_per.py's step tests, for any action count"""
    omem = ReplayOracle(size, batch_size=8)
    synthetic_fill(omem, seed, num_actions=A, current=None)
    omem.terminals[np.arange(7, size, 97)] = True
    raw = (10.0 ** np.random.RandomState(seed).uniform(-2, 1, size)).astype(np.float32)
    return omem, raw


@pytest.mark.parametrize("A", [1, 8, 9])
def test_prioritized_step_action_counts(sd, A):
    """--prioritized_replay through the library's loop: the stratified draw, the importance weights, the weighted gradients, the update
    and the new priorities — the checks and bounds of tests/test_gpu_per.py's test_one_step"""
    from test_gpu_per import ALPHA, EPS, _check_update, _mem
    B, size = 8, 3000
    mem = _mem(sd, size, B, A=A)
    omem, raw = _per_fixture(size, A)
    mem.set_priorities(0, raw)
    ws = xavier_weights(A, 760 + A)
    net = sd.DeepQNetwork(A, make_args(batch_size=B))
    net.set_weights(ws, 0)
    net.update_target_network()
    net.set_option("keep_gradients", 1)
    o = P.PEROracle(A, batch_size=B, weights=ws)
    o.Wt = [w.copy() for w in ws]
    leaf = mem.priorities()
    random.seed(21)
    st = random.getstate()
    net.train_from_memory(mem, 1)
    idx, w = mem.last_sample()
    r = random.Random(); r.setstate(st)
    assert np.array_equal(idx, P.sample(leaf, P.uniforms(r, B)))
    np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)
    assert w.min() < 0.5                                               # (the weights are spread: ignoring them fails below)
    o.weights = w
    g, _, _, preq = o.gradients(omem.gather(idx))
    q, _ = net.last_q()
    assert np.abs(q - preq).max() < Q_TOL * max(1.0, float(np.abs(preq).max()))
    for i in range(5):
        assert np.abs(net.get_layer(i, 3) - g[i]).max() < 1e-4 * max(1e-3, np.abs(g[i]).max()), i
    _check_update(net, o, g, B, {})
    newp = P.new_priority(o.last_abs_delta, ALPHA, EPS)
    pr = mem.priorities()
    last = {int(i): k for k, i in enumerate(idx)}
    np.testing.assert_allclose(np.array([pr[i] for i in last]), np.array([newp[k] for k in last.values()]), rtol=1e-5)


@pytest.mark.parametrize("A", [1, 8, 9])
def test_batch_norm_step_action_counts(sd, A):
    """--batch_norm (its own head form): the checks and bounds of tests/test_gpu_bn.py's train-step test"""
    from test_gpu_bn import _check_state, _pair as bn_pair
    B = 8
    net, o = bn_pair(sd, A, B, 770 + A)
    net.set_option("keep_gradients", 1)
    mb = random_minibatch(B, A, 771 + A)
    g, _, _, preq = o.gradients(mb)
    o.optimize(g, B)
    net.train(mb)
    q, _ = net.last_q()
    assert np.abs(q - preq).max() < Q_TOL
    for i in range(5):
        assert np.abs(net.get_layer(i, 3) - g[i]).max() < 5e-4 * max(1e-3, np.abs(g[i]).max()), i
    gb, gg = o._bn_grads
    for l in range(4):
        b_, g_ = net.get_bn(l, 3)
        assert np.abs(b_ - gb[l]).max() < 5e-4 * max(1e-3, np.abs(gb[l]).max()), l
        assert np.abs(g_ - gg[l]).max() < 5e-4 * max(1e-3, np.abs(gg[l]).max()), l
    _check_state(net, o, 2e-5)


@pytest.mark.parametrize("A", [1, 9])
@pytest.mark.parametrize("dtype,geom", [("float64", (4, 84, 84)), ("float32", (2, 64, 48))])
def test_generic_path_action_counts(sd, dtype, geom, A):
    """float64 and a non-84 x 84 geometry (generic_net.hip, its own head): tests/test_gpu_generic.py's one-step test and tolerances"""
    from test_gpu_generic import _minibatch, _pair as gen_pair, _rel
    hist, H, W = geom
    B = 7
    net, o = gen_pair(sd, A, B, hist, H, W, dtype, 780 + A)
    mb = _minibatch(B, A, hist, H, W, 781 + A)
    tol_g, tol_w, tol_q = (1e-11, 1e-12, 1e-10) if dtype == "float64" else (2e-5, 2e-6, 1e-5)
    costs = _costs(net)
    g_o, cost_o, _, preq = o.gradients(mb)
    net.train(mb, 0)
    o.train(mb, 0)
    assert np.abs(net.last_q()[0] - preq).max() < max(tol_q, 1e-6)              # (last_q returns float32)
    assert abs(costs[0] - float(cost_o)) <= 1e-6 * max(1.0, abs(float(cost_o)))
    for l in range(5):
        assert _rel(net.get_layer(l, 3), g_o[l]) < tol_g, ("gradient", l)
        assert _rel(net.get_layer(l, 0), o.W[l]) < tol_w, ("weights", l)
        assert _rel(net.get_layer(l, 2), o.S[l]) < max(tol_g * 4, 1e-10), ("rmsprop state", l)
    assert np.abs(net.predict(mb[0]) - o.predict(mb[0])).max() < tol_q


@pytest.mark.parametrize("A", [1, 7, 8, 9, 17])
def test_acting_calls_action_counts(sd, A):
    """predict_state on a DeviceStateBuffer fed through act_step (with and without the speculative forward) and act_greedy: the
    one-launch forward's eight partial Q-vectors of length A against the oracle and the five-launch forward, at the bounds of
    tests/test_gpu_act.py; act_greedy is the first maximum of those Q-values."""
    net = sd.DeepQNetwork(A, make_args(batch_size=32))
    ws = xavier_weights(A, 790 + A)
    net.set_weights(ws, 0)
    net.update_target_network()
    orc = OracleDQN(A, batch_size=1, weights=ws)
    buf = sd.DeviceStateBuffer(make_args(batch_size=32))
    rng = np.random.RandomState(791 + A)
    for i in range(6):
        net.set_option("act_kernel", 1)
        net.act_step(buf, None, rng.randint(0, 256, (84, 84), dtype=np.uint8), speculate=bool(i % 2))
        q1 = net.predict_state(buf)
        a = net.act_greedy(buf)
        net.set_option("act_kernel", 0)
        q5 = net.predict_state(buf)
        qo = orc.predict(buf.getState()[None])[0]
        scale = max(1e-3, float(np.abs(qo).max()))
        assert q1.shape == (A,)
        assert np.abs(q1 - q5).max() <= 2e-6 * scale + 1e-7, (i, q1, q5)
        assert np.abs(q1 - qo).max() <= 2e-5 * scale + 1e-6, (i, q1, qo)
        assert a == int(np.argmax(q1)), (i, a, q1)


@pytest.mark.parametrize("A", [0, 19])
def test_action_counts_outside_1_to_18_are_refused(sd, A):
    with pytest.raises(Exception, match=r"num_actions must be in 1\.\.18 \(got %d\)" % A):
        sd.DeepQNetwork(A, make_args(batch_size=8))


# ---- B. exact ties in the Double DQN choice ----------------------------------------------------------------------------------------------
# name: (A, B, screen (hist, H, W), make_args keywords, Q tolerance of the configuration (tests/test_gpu_double_dqn.py), (k1, k2),
#        offset between the target net's rows k2 and k1)
TIES = {
    "fp32_b32": (6, 32, (4, 84, 84), {}, 1e-4, (1, 4), 0.02),
    "fp32_b256": (6, 256, (4, 84, 84), {}, 1e-4, (1, 4), 0.02),
    "fp16_b32": (6, 32, (4, 84, 84), dict(datatype="float16"), 3e-3, (1, 4), 0.05),
    "bn_b32": (6, 32, (4, 84, 84), dict(batch_norm=True), 1e-4, (1, 4), 0.02),
    "f64_b8": (6, 8, (4, 84, 84), dict(datatype="float64"), 1e-9, (1, 4), 0.02),
    "f32_generic": (6, 7, (2, 64, 48), {}, 1e-5, (1, 4), 0.02),
    "fp32_a18": (18, 32, (4, 84, 84), {}, 1e-4, (0, 17), 0.02),
}


def _tie_setup(sd, name, seed, top):
    """Online fc5 rows k1 < k2 bit-identical: |a Xavier row| x 3 (a4 >= 0, so that row is the maximum almost everywhere) or x -3 (never
    the maximum).  Target row k2 = target row k1 + c on every weight, so Qt[:, k2] - Qt[:, k1] = c sum(a4) > 0: the LAST maximum (and the
    standard step's max) gives a different, larger bootstrap value than the first."""
    A, B, geom, kw, tol, (k1, k2), c = TIES[name]
    dt = np.float64 if kw.get("datatype") == "float64" else np.float32
    ws, wt = xavier_weights(A, seed, dt, *geom), xavier_weights(A, seed + 100, dt, *geom)
    ws[4][k1] = np.abs(ws[4][k1]) * dt(3 if top else -3)
    ws[4][k2] = ws[4][k1]
    wt[4][k2] = wt[4][k1] + dt(c)
    assert ws[4][k1].tobytes() == ws[4][k2].tobytes()
    cls = DoubleDQNOracleBN if kw.get("batch_norm") else DoubleDQNOracle
    o = cls(A, batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2], dtype=dt, weights=ws,
            half_activations=kw.get("datatype") == "float16")
    o.Wt = [w.copy() for w in wt]
    net = sd.DeepQNetwork(A, make_args(batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2],
                                       double_dqn=True, **kw))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    if kw.get("batch_norm"):                 # non-trivial BatchNorm parameters and running statistics in both nets (tests/test_gpu_bn.py)
        rng = np.random.RandomState(seed + 7)
        for l in range(4):
            for tgt, (be, ga, gm, gv) in enumerate(((o.beta, o.gamma, o.gmean, o.gvar), (o.beta_t, o.gamma_t, o.gmean_t, o.gvar_t))):
                be[l][:] = rng.uniform(-0.3, 0.3, be[l].shape); ga[l][:] = rng.uniform(0.5, 1.5, ga[l].shape)
                gm[l][:] = rng.uniform(-0.2, 0.2, gm[l].shape); gv[l][:] = rng.uniform(0.5, 2.0, gv[l].shape)
                net.set_bn(l, be[l], ga[l], which=tgt); net.set_bn(l, gm[l], gv[l], which=tgt, running=True)
    return net, o


def _tie_minibatch(name, seed):
    from test_gpu_double_dqn import _minibatch
    A, B, geom = TIES[name][:3]
    return _minibatch(B, A, geom, seed)


def tied_samples(o, mb, k1, k2, tol):
    """(online Q, target Q on the poststates, samples on which the tied pair is the online maximum by more than 3 tol) on the oracle"""
    x = o._normalize(mb[3])
    qo, qt = o.fprop(o.W, x), o.fprop(o.Wt, x)
    others = np.delete(qo, [k1, k2], axis=1).max(1)
    scale = max(1.0, float(np.abs(qt).max()))
    return qo, qt, np.minimum(qo[:, k1], qo[:, k2]) - others > 3 * tol * scale


@pytest.mark.parametrize("name", list(TIES))
def test_double_dqn_takes_the_first_of_two_exactly_tied_maxima(sd, name):
    A, B, geom, kw, tol, (k1, k2), _ = TIES[name]
    tol = max(tol, 1e-6)                                               # (last_q returns float32)
    mb = _tie_minibatch(name, 15)
    net, o = _tie_setup(sd, name, 31, top=True)
    qo, qt, tied = tied_samples(o, mb, k1, k2, tol)
    scale = max(1.0, float(np.abs(qt).max()))
    live = tied & ~mb[4]
    print("%s: tied pair is the online maximum on %d of %d samples; target gap min %.3e (100 tol = %.3e)" % (
        name, int(tied.sum()), B, float((qt[:, k2] - qt[:, k1])[tied].min()), 100 * tol * scale))
    assert tied.sum() * 2 >= B
    assert np.abs(qt[:, k2] - qt[:, k1])[tied].min() >= 100 * tol * scale
    # the tie is exact on the device, not merely near
    qd = net.predict(mb[3])
    assert np.array_equal(qd[:, k1], qd[:, k2])
    net.train(mb)
    _, mq = net.last_q()
    assert live.any()
    assert np.abs(mq - qt[:, k1])[tied].max() <= tol * scale, np.nonzero(np.abs(mq - qt[:, k1]) > tol * scale)[0]


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_tied_rows_below_the_maximum_change_nothing(sd, name):
    """the mirror case: rows k1, k2 bit-identical but never the maximum — the step is the untied oracle's (numpy argmax)"""
    from test_gpu_double_dqn import _check_grads, _check_maxpostq, _follow
    A, B, geom, kw, tol, (k1, k2), _ = TIES[name]
    mb = _tie_minibatch(name, 16)
    net, o = _tie_setup(sd, name, 41, top=False)
    net.set_option("keep_gradients", 1)
    qd = net.predict(mb[3])
    assert np.array_equal(qd[:, k1], qd[:, k2])
    net.train(mb)
    q, mq = net.last_q()
    o.choose = _follow(mq, tol)
    g, _, _, preq = o.gradients(mb)
    best = o.last_online_postq.argmax(1)
    assert not np.isin(best, (k1, k2)).any()
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    _check_maxpostq(mq, o, tol)
    _check_grads(net, "fp32_b32" if name == "fp32_b32" else "f64_b8", g)


# ---- C. degenerate minibatches -----------------------------------------------------------------------------------------------------------
def _degenerate(kind, B, A, seed):
    pre, act, rew, post, term = random_minibatch(B, A, seed, reward_range=(-3, 4))
    if kind == "all_terminal":
        term[:] = True
    elif kind == "none_terminal":
        term[:] = False
    elif kind == "action_0":
        act[:] = 0
    elif kind == "action_last":
        act[:] = A - 1
    elif kind == "rewards_plus_7":
        rew[:] = 7
    elif kind == "rewards_minus_7":
        rew[:] = -7
    elif kind == "clip0":
        rew[:] = np.where(np.random.RandomState(seed + 1).rand(B) < 0.5, -5, 5)
    else:
        raise KeyError(kind)
    return pre, act, rew, post, term


KINDS = ["all_terminal", "none_terminal", "action_0", "action_last", "rewards_plus_7", "rewards_minus_7"]


@pytest.mark.parametrize("kind", KINDS + ["clip0"])
def test_degenerate_minibatch_float32(sd, kind):
    """clip0: clip_error = 0 with min_reward / max_reward = -5 / 5 and rewards +-5 — |delta| ~ 5 reaches the backward pass unclipped"""
    A, B = 4, 32
    kw = dict(clip_error=0.0, min_reward=-5.0, max_reward=5.0) if kind == "clip0" else {}
    net, o = _pair(sd, A, B, 900, **kw)
    mb = _degenerate(kind, B, A, 901)
    _step_check(net, o, mb)
    if kind == "clip0":
        assert np.abs(net.last_q()[0][np.arange(B), mb[1]] - mb[2]).min() > 3          # every |delta| well above 1


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_minibatch_float16(sd, kind):
    """float16 stores delta4 as half(delta4 x 1024).  With clip_error = 1 (every case here) |delta4| <= max |W5| = sqrt(3 / 512) = 0.077,
    so the scaled half is at most 79: far inside half's range (65504) whatever the rewards — they are clipped to +-1 before the TD
    error and the error to +-1 after it."""
    A, B = 4, 32
    net, o = _pair(sd, A, B, 910, half=True)
    _step_check(net, o, _degenerate(kind, B, A, 911), half=True)
    assert all(np.isfinite(net.get_layer(i, 0)).all() for i in range(5))


@pytest.mark.parametrize("datatype", ["float32", "float16"])
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam", "adadelta"])
def test_all_zero_prestates_leave_exact_zero_gradients(sd, optimizer, datatype):
    """All-zero prestates, random poststates.  Without biases a4 of the prestates is exactly 0, so the a4 > 0 gate closes every path
    into fc4 and the convolutions, and fc5's own weight gradient delta x a4 is exactly 0 too (the taken rows included): every gradient
    sum is exactly zero although delta is not.  From a non-zero optimizer state (set through which = 2 and 4):
      * the first state comes back as exactly rho S (RMSProp, Adadelta) / beta_1 m (Adam), the second as rho S2 / beta_2 v;
      * RMSProp and Adadelta leave every weight bit-identical (their update is a multiple of the gradient);
      * Adam moves a weight by lr_t m' / (sqrt(v') + eps) whatever the gradient: bit-identical where m is zero (half of the elements
        here), and elsewhere the formula within one spacing of the weight (its final rounding) + 1e-6 of the update (a few float32
        ulp for the multiply, square root and divide)."""
    A, B = 4, 32
    f32 = np.float32
    mb = list(random_minibatch(B, A, 921))
    mb[0] = np.zeros_like(mb[0])
    rng = np.random.RandomState(922)
    ws = xavier_weights(A, 923)
    s1 = [rng.uniform(1e-7, 1e-4, w.shape).astype(f32) for w in ws]
    s2 = [rng.uniform(1e-9, 1e-6, w.shape).astype(f32) for w in ws]
    if optimizer == "adam":
        s1 = [(rng.uniform(-1e-3, 1e-3, w.shape) * (rng.rand(*w.shape) < 0.5)).astype(f32) for w in ws]
    for keep in ((0, 1) if optimizer == "rmsprop" else (1,)):              # (rmsprop: the fused fc4 update and the unfused one)
        net = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=optimizer, datatype=datatype))
        net.set_weights(xavier_weights(A, 924), 1)
        net.set_weights(ws, 0)
        net.set_weights(s1, 2)
        if optimizer != "rmsprop":
            net.set_weights(s2, 4)
        net.set_option("keep_gradients", keep)
        net.train(tuple(mb), 0)
        q, mq = net.last_q()
        assert np.all(q == 0) and np.abs(mq).max() > 0
        for i in range(5):
            w, a = net.get_layer(i, 0), net.get_layer(i, 2)
            if keep:
                assert np.all(net.get_layer(i, 3) == 0), i
            decay = f32(0.9) if optimizer == "adam" else f32(0.95)
            assert np.array_equal(a, s1[i] * decay), (i, "first state")
            if optimizer != "rmsprop":
                assert np.array_equal(net.get_layer(i, 4), s2[i] * (f32(0.999) if optimizer == "adam" else f32(0.95))), (i, "second state")
            if optimizer != "adam":
                assert np.array_equal(w, ws[i]), (i, "weights")
            else:
                still = s1[i] == 0
                assert still.any() and (~still).any()
                assert np.array_equal(w[still], ws[i][still]), (i, "weights without momentum")
                lr_t = 0.00025 * np.sqrt(1 - 0.999) / (1 - 0.9)
                m, v = (s1[i] * f32(0.9)).astype(np.float64), (s2[i] * f32(0.999)).astype(np.float64)
                upd = lr_t * m / (np.sqrt(v) + 1e-8)
                err = np.abs(w - (ws[i].astype(np.float64) - upd))
                assert (err <= np.spacing(np.abs(ws[i])) + 1e-6 * np.abs(upd)).all(), (i, float(err.max()))
        if datatype == "float16":                                          # the half copies follow: same forward as a net given these weights
            twin = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=optimizer, datatype=datatype))
            twin.set_weights(net.get_weights(0), 0)
            assert np.array_equal(twin.predict(mb[3]), net.predict(mb[3]))


def catch_minibatch(B, seed=5, steps=48):
    """B consecutive transitions of a scripted random play of the game catch (the host definition, tests/catch_oracle.py) at 84 x 84,
    two balls per episode so that the play holds terminals; states are the last four frames, zero before an episode's first"""
    env = CatchOracle(84, 84, seed=seed, balls_per_episode=2)
    rng = np.random.RandomState(seed)
    state = np.zeros((4, 84, 84), np.uint8)
    state[-1] = env.screen()
    pre, act, rew, post, term = [], [], [], [], []
    for _ in range(steps):
        a = int(rng.randint(0, 3))
        r = env.act(a)
        t = env.terminal
        pre.append(state.copy())
        if t:
            env.restart()
            state[:] = 0
        else:
            state[:-1] = state[1:]
        state[-1] = env.screen()
        post.append(state.copy()); act.append(a); rew.append(r); term.append(t)
    k = steps - B
    return (np.stack(pre[k:]), np.array(act[k:], np.uint8), np.array(rew[k:], np.int64), np.stack(post[k:]), np.array(term[k:], bool))


def conv1_zero_share(o, states):
    """share of conv1's pre-activations that are exactly zero on the oracle"""
    cols, _, _ = _im2col(o._normalize(states), 8, 8, 4)
    return float(((cols @ o.W[0]) == 0).mean())


@pytest.mark.parametrize("half", [False, True])
def test_game_frames_step(sd, half):
    """Frames of the catch renderer: a 21 x 7 paddle and a 7 x 7 ball on black, so most 8 x 8 patches are all zero — exact-zero
    pre-activations (gates exactly at their threshold), dead fc4 units and exact-zero gradient elements, none of which uniform random
    bytes produce."""
    A, B = 4, 32
    mb = catch_minibatch(B)
    assert mb[4].any() and not mb[4].all() and (mb[2] != 0).any() and len(set(mb[1].tolist())) == 3
    net, o = _pair(sd, A, B, 930, half=half)
    assert conv1_zero_share(o, mb[0]) > 0.5
    _step_check(net, o, mb, half=half)
