"""--quantiles on the GPU against tests/quantile_oracle.py.

Train steps are fed from tests/test_gpu_bootstrap.py's 300-slot ring through train_indexes (sdqn_net_train_replay); online and target
weights come from different Xavier draws of an N A-action net.  The forward and the backward are the launches of an N A-action net, so the
bounds are the ones tests/test_gpu_bootstrap.py holds the bootstrap head to in the same regime: Q(pre) within tol, the bootstrap value
(maxq, and here each of the N targets: r + gamma times one stored Q) within 3 tol, gradients by _check_grads, the hold-out Q after
free-running steps within the regime's free-running bound.  Two bounds follow from those by the loss's shape (kappa = clip_error = 1):
  * g = w clip(delta) / kappa is continuous in delta (it passes through 0 where the indicator steps) with slope <= 1 / kappa, so an error
    e_delta <= tol scale + 3 tol scale_T in a pair's delta moves dq = (sum_j' g_jj') / N^2 by at most e_delta / (N kappa);
  * rho = w L_kappa(delta) / kappa has slope w |clip(delta)| / kappa <= 1, so the mean over the pairs — a cost term — moves by at most
    e_delta, and so does the cost, their mean.
In the oracle alone every sample's best and second-best m(a) differ by more than 1e-4 (asserted, not filtered: the seeds were chosen on
the CPU), so no a* of a comparison is decided by rounding."""
import numpy as np
import pytest

import bootstrap_oracle as BO
import nstep_oracle as NO
import quantile_oracle as QO
from clip_oracle import clip_gradients
from collect_oracle import CollectOracle
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle
from soft_target_oracle import blend
from test_gpu_bootstrap import REGIMES as _BR, SIZE, _batch, _cargs, _check_grads, _dt
from test_gpu_double_dqn import _counts
from test_gpu_munchausen import CONFIGS as _MU
from util import make_args

pytestmark = pytest.mark.gpu

GAMMA = 0.99
# tests/test_gpu_bootstrap.py's regimes, and float64 on the generic path at tests/test_gpu_generic.py's small geometry with that file's batch
REGIMES = dict(_BR, f64_small=(7, (3, 60, 52), dict(datatype="float64")) + _MU["f64_b8"][4:])
# (regime, A, N, batch seed): the seed is the first from 5 on whose batch meets the gap condition in the oracle (searched on the CPU)
CASES = [("fp32_b32", 2, 2, 5), ("fp32_b32", 3, 6, 5), ("fp32_b32", 2, 9, 5), ("fp32_b128", 2, 2, 5), ("fp32_b128", 3, 6, 6), ("fp32_b128", 2, 9, 8),
         ("fp16_b32", 3, 6, 5), ("f64_small", 3, 6, 5)]
COLLECT = "catch_collect(lockstep)"              # the lockstep's name in the launch profile (tests/test_gpu_collect.py)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _regime(regime):
    """a key of REGIMES, or a regime of its form itself (as tests/test_gpu_bootstrap.py's helpers take one)"""
    return REGIMES[regime] if isinstance(regime, str) else regime


def _setup(sd, regime, A, N, seed=11, n=1, **extra):
    """(net, oracle, product ring, oracle ring, valid indexes); sd = None: the oracle's side alone (net and product ring None)"""
    B, (hist, H, W), kw = _regime(regime)[:3]
    args = make_args(batch_size=B, history_length=hist, screen_height=H, screen_width=W, **dict(kw, quantiles=N, n_step=n, **extra))
    om = ReplayOracle(SIZE, H, W, hist, B)
    BO.fill_ring(om, A)
    ws, wt = xavier_weights(N * A, seed, _dt(kw), hist, H, W), xavier_weights(N * A, seed + 100, _dt(kw), hist, H, W)
    net = mem = None
    if sd is not None:
        mem = sd.ReplayMemory(SIZE, args)
        BO.fill_ring(mem, A)
        mem.sync_mirror()
        net = sd.DeepQNetwork(A, args)
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        assert net.quantiles == N and net.num_actions == A
    o = QO.QuantileOracle(A, N, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=_dt(kw), weights=ws,
                          half_activations=kw.get("datatype") == "float16", n_step=n)
    o.Wt = [w.copy() for w in wt]
    return net, o, mem, om, BO.valid_slots(om, n)


def _gaps_clear(o):
    assert o.last_gaps.min() > QO.GAP, "sample %d: best and second-best m(a) differ by %.3e" % (int(o.last_gaps.argmin()), o.last_gaps.min())


def _check_step(net, o, regime, g, cost_ref, preq, cost, mb):
    B, geom, kw = _regime(regime)[:3]
    tol = max(_regime(regime)[3], 1e-6)
    N, A = o.quantiles, o.game_actions
    _gaps_clear(o)
    q, mq = net.last_q()
    scale = max(1.0, float(np.abs(preq).max()))
    scale_t = max(1.0, float(np.abs(o.last_targets).max()), float(np.abs(o.last_maxq).max()))
    eq, em = np.abs(q - preq).max(), np.abs(mq - o.last_maxq).max()
    e_delta = tol * scale + 3 * tol * scale_t
    ec = abs(float(cost) - float(cost_ref))
    label = regime if isinstance(regime, str) else "B=%d %s" % (B, kw or "float32")
    print("%s A=%d N=%d: Q(pre) err %.3e (bound %.1e), maxq err %.3e (%.1e), cost %.6g vs %.6g (err %.3e, bound %.1e)"
          % (label, A, N, eq, tol * scale, em, 3 * tol * scale_t, cost, cost_ref, ec, e_delta))
    assert q.shape == (o.batch_size, N * A)
    assert eq < tol * scale
    assert em < 3 * tol * scale_t
    assert ec < e_delta
    # the N targets and the dq rows, on every path (sdqn_net_last_quantile_step: the generic path's too)
    T64, dq64 = net.last_quantile_step()
    et, ed = np.abs(T64 - o.last_targets).max(), np.abs(dq64 - o.gradients_dq).max()
    print("   targets err %.3e (bound %.1e), dq err %.3e (%.1e)" % (et, 3 * tol * scale_t, ed, e_delta / N))
    assert T64.shape == (B, N) and dq64.shape == (B, N * A)
    assert et < 3 * tol * scale_t
    assert ed < e_delta / N
    live = np.zeros((B, N, A), bool)
    live[np.arange(B), :, np.asarray(mb[1], np.int64)] = True
    assert (dq64.reshape(B, N, A)[~live] == 0).all() and (dq64 != 0).sum() > B     # zero off the taken action's N rows
    if kw.get("datatype") != "float64" and geom == (4, 84, 84):                    # the tuned path's own buffers
        T = net.debug_read("quantile_targets", B * N).reshape(B, N)
        dq = net.debug_read("dq", B * N * A).reshape(B, N * A)
        terms = net.debug_read("cost_terms", B)
        qq = net.debug_read("q", 2 * B * N * A).reshape(2, B, N * A)
        ect = np.abs(terms - o.last_cost_terms).max()
        print("   cost term err %.3e (%.1e)" % (ect, e_delta))
        assert ect < e_delta
        assert np.array_equal(T.astype(np.float64), T64) and np.array_equal(dq.astype(np.float64), dq64)
        assert np.array_equal(qq[0], q)
        # the device restates the host function on its own stored rows, bit for bit (float32 and float16 alike: the head is fp32)
        r = [float(x) for x in mb[2]] if o.n_step > 1 else [float(x) for x in np.clip(mb[2], -1.0, 1.0)]
        gam = NO.gamma_n(o.n_step, GAMMA) if o.n_step > 1 else GAMMA
        same = 0
        for n in range(B):
            ref = QO.sample(qq[0, n], qq[1, n], N, A, int(mb[1][n]), r[n], bool(mb[4][n]), gam, 1.0)
            same += int(np.array_equal(ref["dq"].view(np.uint32), dq[n].view(np.uint32)) and ref["cost"].view(np.uint32) == terms[n].view(np.uint32)
                        and np.array_equal(ref["targets"].view(np.uint32), T[n].view(np.uint32)) and ref["maxq"].view(np.uint32) == mq[n].view(np.uint32))
        print("   %d of %d samples bit-identical to the host restatement on the device's own Q rows" % (same, B))
        assert same == B
    _check_grads(net, _regime(regime), g)


def _gradients(o, mb):
    g, cost_ref, deltas, preq = o.gradients(mb)
    o.gradients_dq = deltas
    return g, cost_ref, preq


@pytest.mark.parametrize("regime,A,N,bseed", CASES)
def test_one_step_parity(sd, regime, A, N, bseed):
    B = REGIMES[regime][0]
    net, o, mem, om, valid = _setup(sd, regime, A, N)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, bseed)
    g, cost_ref, preq = _gradients(o, mb)
    # the N targets of a sample differ (one per quantile of the target net): a library that used one target for all of them fails below
    assert (np.ptp(o.last_targets[~np.asarray(mb[4])], axis=1) > 1e-2).mean() > 0.5
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, regime, g, cost_ref, preq, cost, mb)


def test_three_free_running_ring_steps_b32(sd):
    """float32 B = 32: hold-out quantiles and every layer's weights after three free-running ring-fed steps, within the regime's free-running bound"""
    regime, A, N = "fp32_b32", 3, 6
    B, geom, kw, tol, tol10 = REGIMES[regime]
    net, o, mem, om, valid = _setup(sd, regime, A, N, seed=21)
    for s in range(3):
        idx, mb = _batch(om, valid, B, 30 + s)
        net.train_indexes(mem, idx)
        o.train(mb)
        _gaps_clear(o)
    hold = om.gather(_batch(om, valid, B, 99)[0])[0]
    ref, got = o.predict_quantiles(hold), net.predict_quantiles(hold)
    assert got.shape == (B, N, A)
    err, qmax = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s A=%d N=%d: hold-out Q max abs err after 3 steps %.3e (bound %.1e)" % (regime, A, N, err, tol10 * max(1.0, qmax)))
    assert err < tol10 * max(1.0, qmax)
    for i in range(5):
        we = float(np.abs(np.asarray(net.get_layer(i), np.float64) - o.W[i]).max())
        print("   layer %d weight max abs err %.3e" % (i, we))
        assert we < tol10 * max(1.0, float(np.abs(o.W[i]).max())), i
    assert np.abs(net.predict(hold) - o.predict_mean(hold)).max() < tol10 * max(1.0, qmax)      # predict: the mean over the quantiles [B][A]


def test_three_teacher_forced_ring_steps_b128(sd):
    """float32 B = 128 fed from the ring, held step by step (why: DESIGN.md §27.3): before every step the net takes the oracle's weights
    and optimizer state, and each step's quantities are held to the one-step rules"""
    regime, B, A, N = "fp32_b128", 128, 3, 6
    net, o, mem, om, valid = _setup(sd, regime, A, N, seed=21)
    net.set_option("keep_gradients", 1)
    for s in range(3):
        net.set_weights(o.W, 0)
        for i in range(5):
            net.set_layer(i, o.S[i], 2)
        idx, mb = _batch(om, valid, B, 30 + s)
        g, cost_ref, preq = _gradients(o, mb)
        cost = net.train_indexes(mem, idx, want_cost=True)
        _check_step(net, o, regime, g, cost_ref, preq, cost, mb)
        o.optimize(g, B)


@pytest.mark.parametrize("B,bseed", [(33, 5), (127, 6)])
def test_batch_edges(sd, B, bseed):
    """float32 B = 33 and B = 127 at (3, 6): one workgroup per sample at a ragged batch, both sides of the B = 128 regime change"""
    regime = (B,) + REGIMES["fp32_b32"][1:]
    net, o, mem, om, valid = _setup(sd, regime, 3, 6)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, bseed)
    g, cost_ref, preq = _gradients(o, mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, regime, g, cost_ref, preq, cost, mb)


def test_n_step_3(sd):
    A, N, B = 3, 6, 32
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, N, n=3)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 8, n=3)
    assert np.asarray(mb[4]).any() and not np.asarray(mb[4]).all()
    g, cost_ref, preq = _gradients(o, mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)


@pytest.mark.parametrize("what", ["clip_grad_norm", "target_tau"])
def test_one_step_composed(sd, what):
    """--clip_grad_norm 10 / --target_tau 0.01 at (3, 6), B = 32: the step's quantities by the one-step rules, then the applied update.
    G = 10 is the issue's figure; no row of dq exceeds 1 / N here, so the mean gradient's norm stays far below it and the scale is 1 on
    both sides: what this holds of the clip is its norm (the two launches ran between the gradient and the update) and an update left
    unscaled.  A clip that bites is tests/test_gpu_clip_grad_norm.py's and tests/test_gpu_bootstrap.py's ground."""
    A, N, B = 3, 6, 32
    G, TAU = 10.0, 0.01
    extra = dict(clip_grad_norm=G) if what == "clip_grad_norm" else dict(target_tau=TAU)
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, N, seed=31, **extra)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 40)
    g, cost_ref, preq = _gradients(o, mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    tol10 = REGIMES["fp32_b32"][4]
    if what == "clip_grad_norm":
        gc, norm, scale = clip_gradients(g, B, G, np.float32)
        n_lib, s_lib = net.last_grad_norm()
        print("clip_grad_norm: norm %.6g vs %.6g, scale %.6g vs %.6g" % (n_lib, norm, s_lib, float(scale)))
        assert abs(n_lib - norm) < 1e-3 * max(norm, 1e-3) and abs(s_lib - float(scale)) < 1e-3
        _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)      # (keep_gradients: g holds the sums as reduced; scale 1 left them)
        o.optimize(gc, B)
    else:
        _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)
        o.optimize(g, B)
        o.Wt = [blend(w, wt, TAU, np.float32) for w, wt in zip(o.W, o.Wt)]
    for which, ow in ((0, o.W), (1, o.Wt)):
        for i in (0, 4):
            err = np.abs(np.asarray(net.get_layer(i, which), np.float64) - ow[i]).max()
            assert err < tol10 * max(1.0, float(np.abs(ow[i]).max())), (which, i, err)


@pytest.mark.parametrize("kw", [{}, dict(datatype="float16")])
def test_one_quantile_is_inert(sd, kw):
    """--quantiles 1: three steps leave the weights and the optimizer state of a net built without the flag bit for bit, from the same launches"""
    A, B = 4, 32
    ws, wt = xavier_weights(A, 81), xavier_weights(A, 181)
    rng = np.random.RandomState(80)
    mbs = [(rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64),
            rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.rand(B) < 0.1) for _ in range(3)]
    nets = [sd.DeepQNetwork(A, make_args(batch_size=B, quantiles=1, **kw)), sd.DeepQNetwork(A, make_args(batch_size=B, **kw))]
    counts = []
    for net in nets:
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        counts.append(_counts(net, lambda: [net.train(mb) for mb in mbs], n=1))
    assert counts[0] == counts[1]
    for which in (0, 2):
        for i in range(5):
            assert np.array_equal(np.array(nets[0].get_layer(i, which)), np.array(nets[1].get_layer(i, which))), (which, i)
    assert np.array_equal(nets[0].predict(mbs[0][0]), nets[1].predict(mbs[0][0]))
    assert np.array_equal(nets[0].predict_quantiles(mbs[0][0])[:, 0], nets[1].predict(mbs[0][0]))


def test_refusals_in_the_library_in_either_order(sd):
    lib, C = sd.load(), __import__("ctypes")
    net = sd.DeepQNetwork(3, make_args(quantiles=6))
    n = C.c_int()
    sd._lib.check(lib.sdqn_net_get_quantiles(net._h, C.byref(n)))
    assert n.value == 6
    for call, word in ((lambda: net.set_option("double_dqn", 1), "double_dqn"), (lambda: net.set_munchausen(True), "munchausen"),
                       (lambda: net.set_advantage_learning(0.5, False), "advantage_learning"),
                       (lambda: sd._lib.check(lib.sdqn_net_set_bootstrap(net._h, 2, 1.0, 0)), "bootstrap_heads")):
        with pytest.raises(Exception) as ei:
            call()
        assert "quantiles" in str(ei.value) and word in str(ei.value), str(ei.value)
    pmem = sd.ReplayMemory(SIZE, make_args(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000))
    BO.fill_ring(pmem, 3)
    pmem.sync_mirror()
    with pytest.raises(Exception) as ei:
        net.train_from_memory(pmem, 1)
    assert "quantiles" in str(ei.value) and "prioritized_replay" in str(ei.value)
    plain = sd.DeepQNetwork(3, make_args(quantiles=6))
    for arm, word in ((lambda h: h.set_option("double_dqn", 1), "double_dqn"), (lambda h: h.set_munchausen(True), "munchausen"),
                      (lambda h: h.set_advantage_learning(0.5, False), "advantage_learning"),
                      (lambda h: sd._lib.check(lib.sdqn_net_set_bootstrap(h._h, 2, 1.0, 0)), "bootstrap_heads")):
        other = sd.DeepQNetwork(18, make_args())
        arm(other)
        with pytest.raises(Exception) as ei:
            sd._lib.check(lib.sdqn_net_set_quantiles(other._h, 6))
        assert "quantiles" in str(ei.value) and word in str(ei.value), str(ei.value)
    zero = sd.DeepQNetwork(18, make_args(clip_error=0.0))
    with pytest.raises(Exception) as ei:
        sd._lib.check(lib.sdqn_net_set_quantiles(zero._h, 6))
    assert "clip_error" in str(ei.value)
    assert lib.sdqn_net_set_quantiles(plain._h, 5) != 0              # 5 does not divide 18


# ---- acting ---------------------------------------------------------------------------------------------------------------------
def _spread_quantiles(net, N, A, seed=3):
    """Xavier torso and a Xavier fc5 scaled up, so that the quantile means of the three actions differ visibly on the game's frames"""
    ws = xavier_weights(N * A, seed)
    ws[4] = (ws[4] * 8).astype(np.float32)
    net.set_weights(ws, 0)
    return ws


def test_collect_acts_on_the_quantile_mean(sd):
    Nenv, steps, N, A = 4, 40, 6, 3
    args = _cargs(quantiles=N, random_seed=9)
    net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(Nenv * 40, args)
    mem.set_lanes(Nenv)
    _spread_quantiles(net, N, A)
    out = net.collect(env, mem, Nenv, steps, 0.0, seed=77, trace=True)
    o = CollectOracle(Nenv, Nenv * 40, 4, 84, 84, 77, env.balls_per_episode)
    seen = set()
    for t in range(steps):
        if t % 10 == 0 or t == steps - 1:
            states = np.zeros((32, 4, 84, 84), np.uint8); states[:Nenv] = o.games.states
            raw = net.predict_quantiles(states)[:Nenv].reshape(Nenv, N * A)
            for e in range(Nenv):
                want = QO.action_values(raw[e], N, A)
                assert np.array_equal(want, out["q"][t][e]), (t, e)              # tr_q holds the mean row, the oracle's float sum exactly
                assert QO.act(raw[e], N, A) == out["actions"][t][e], (t, e)
        a, r, term = o.lockstep(0.0, out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(term, out["terminals"][t]), t
        seen.update(int(x) for x in a)
    assert len(seen) >= 2
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k


def test_evaluate_acts_on_the_quantile_mean(sd):
    """evaluate on catch, 4 copies, N = 6, epsilon 0: an oracle game loop seeded like evaluate (tests/catch_oracle.py: EvalOracle) holds
    the states each lockstep acts on; their raw [N A] rows come from predict_quantiles, and the traced row has to be the oracle's mean of
    that raw row bit for bit, the action the oracle's rule on it"""
    from catch_oracle import EvalOracle
    Nenv, steps, N, A = 4, 30, 6, 3
    args = _cargs(quantiles=N, random_seed=9)
    net, env = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1)
    _spread_quantiles(net, N, A)
    out = net.evaluate(env, Nenv, steps, epsilon=0.0, seed=5, trace=True)
    assert out["q"].shape == (steps, Nenv, A)
    o = EvalOracle(Nenv, net.history_length, env.dims[0], env.dims[1], 0.0, 5, env.balls_per_episode)
    seen, spread = set(), 0
    for t in range(steps):
        states = np.zeros((32, 4, 84, 84), np.uint8); states[:Nenv] = o.states
        raw = net.predict_quantiles(states)[:Nenv].reshape(Nenv, N * A)
        for e in range(Nenv):
            assert np.array_equal(QO.action_values(raw[e], N, A), out["q"][t][e]), (t, e)
            assert QO.act(raw[e], N, A) == out["actions"][t][e], (t, e)
            spread += int(np.ptp(raw[e].reshape(N, A), axis=0).max() > 0)          # the quantiles of an action differ: a mean, not a copy
        a, r, term = o.step(out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(term, out["terminals"][t]), t
        seen.update(int(x) for x in a)
    assert len(seen) >= 2 and spread > steps
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k


def test_predict_is_the_mean_of_predict_quantiles(sd):
    N, A = 6, 3
    net = sd.DeepQNetwork(A, _cargs(quantiles=N, random_seed=9))
    _spread_quantiles(net, N, A)
    hold = np.random.RandomState(5).randint(0, 256, (32, 4, 84, 84), dtype=np.uint8)
    raw = net.predict_quantiles(hold)
    mean = net.predict(hold)
    assert raw.shape == (32, N, A) and mean.shape == (32, A)
    assert np.array_equal(mean, np.stack([QO.action_values(r.reshape(-1), N, A) for r in raw]))


def test_collect_with_one_quantile_is_the_parent_and_more_add_one_launch(sd):
    Nenv, steps, A = 4, 25, 3
    res, counts = [], []
    for kw in (dict(quantiles=1), {}, dict(quantiles=6)):
        args = _cargs(random_seed=4, **kw)
        net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(Nenv * 40, args)
        mem.set_lanes(Nenv)
        if kw.get("quantiles", 1) == 1:
            net.set_weights(xavier_weights(A, 5), 0)
        out = net.collect(env, mem, Nenv, steps, 0.3, seed=77, trace=True)
        res.append((out, np.array(mem.screens), np.array(mem.actions), np.array(mem.rewards), np.array(mem.terminals)))
        counts.append(_counts(net, lambda: net.collect(env, mem, Nenv, 5, 0.3), n=1))
    (o1, *r1), (o0, *r0) = res[0], res[1]
    for a, b in zip(r1, r0):
        assert np.array_equal(a, b)
    for k in o0:
        assert np.array_equal(o1[k], o0[k]), k
    assert counts[0] == counts[1]
    assert sum(counts[2].values()) == sum(counts[1].values()) + 5, (counts[2], counts[1])
    assert counts[2][COLLECT] == counts[1][COLLECT] + 5


def test_single_environment_acting(sd):
    """sdqn_net_act_greedy and DeepQNetwork.acting_action on one environment: the first maximum of the quantile means, training and testing alike"""
    N, A = 6, 3
    args = _cargs(quantiles=N, random_seed=9, replay_size=400, random_starts=4, exploration_rate_test=0.0)
    net = sd.DeepQNetwork(A, args)
    _spread_quantiles(net, N, A)
    buf = sd.DeviceStateBuffer(args)
    rng = np.random.RandomState(1)
    for k in range(6):
        buf.add(rng.randint(1, 256, (84, 84), dtype=np.uint8))
        raw = net.predict_state(buf)
        assert raw.shape == (N * A,)
        assert net.act_greedy(buf) == QO.act(raw, N, A) == net.acting_action(raw), k
    env, mem = sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(400, args)
    agent = sd.Agent(env, mem, net, args)
    log = []
    agent.callback = type("CB", (), dict(on_step=lambda self, a, r, t, s, e: log.append(a)))()
    agent.test(12)
    assert len(log) == 12 and all(0 <= a < A for a in log)
