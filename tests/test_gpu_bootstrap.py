"""--bootstrap_heads on the GPU against tests/bootstrap_oracle.py.

Train steps are fed from a 300-slot ring through train_indexes (sdqn_net_train_replay), so every sample has the ring index its mask is a
function of.  Online and target weights come from different Xavier draws of a K A-action net, so the K targets of a sample differ.
Bounds: those tests/test_gpu_munchausen.py holds the same regime to (its CONFIGS and _check_grads) — Q(pre) within tol, the bootstrap
value within 3 tol, gradients by the regime's rule, the hold-out Q after free-running steps within the regime's 10-step bound.  The cost
bound is NOT from that file (it asserts no cost); it is derived here: the cost is 0.5 delta^2 averaged, and an error e <= 3 tol scale in
delta moves a term by at most |delta| e + e^2 / 2.  That is loose at float32; the tight cost check is test_masks' per-term 1e-3."""
import numpy as np
import pytest

import bootstrap_oracle as BO
import nstep_oracle as NO
from clip_oracle import clip_gradients
from collect_oracle import CollectOracle
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle
from soft_target_oracle import blend
from test_gpu_double_dqn import _counts
from test_gpu_munchausen import CONFIGS as _MU
from util import make_args

pytestmark = pytest.mark.gpu

GAMMA, MINR, MAXR = 0.99, -1.0, 1.0
SIZE = 300
# regime: (batch, screen, make_args keywords, Q tolerance, 10-step Q tolerance) from tests/test_gpu_munchausen.py
REGIMES = {
    "fp32_b32": (32, (4, 84, 84), {}) + _MU["fp32_b32"][4:],
    "fp32_b128": (128, (4, 84, 84), {}) + _MU["fp32_b128"][4:],
    "fp16_b32": (32, (4, 84, 84), dict(datatype="float16")) + _MU["fp16_b32"][4:],
    "fp16_b128": (128, (4, 84, 84), dict(datatype="float16")) + _MU["fp16_b128"][4:],
    "f64_b32": (32, (4, 84, 84), dict(datatype="float64")) + _MU["f64_b8"][4:],
    "f32_generic": (7, (2, 64, 48), {}) + _MU["f32_generic"][4:],
}
CASES = [("fp32_b32", 2, 2), ("fp32_b32", 4, 2), ("fp32_b32", 3, 6), ("fp32_b128", 2, 2), ("fp32_b128", 4, 2), ("fp32_b128", 3, 6),
         ("fp16_b32", 3, 6), ("fp16_b128", 3, 6), ("f64_b32", 3, 6), ("f32_generic", 2, 2)]


def _regime(regime):
    """a key of REGIMES, or a regime of its form itself (tests/test_gpu_option_head_edges.py passes its own)"""
    return REGIMES[regime] if isinstance(regime, str) else regime


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _dt(kw):
    return np.float64 if kw.get("datatype") == "float64" else np.float32


def _args(regime, **extra):
    B, (hist, H, W), kw = _regime(regime)[:3]
    return make_args(batch_size=B, history_length=hist, screen_height=H, screen_width=W, **dict(kw, **extra))


def _setup(sd, regime, A, K, seed=11, n=1, **extra):
    """(net, oracle, product ring, oracle ring, valid indexes): a full, wrapped 300-slot ring with terminals; different draws for theta / theta-"""
    B, (hist, H, W), kw = _regime(regime)[:3]
    args = _args(regime, bootstrap_heads=K, n_step=n, **extra)
    mem, om = sd.ReplayMemory(SIZE, args), ReplayOracle(SIZE, H, W, hist, B)
    for m in (mem, om):
        BO.fill_ring(m, A)
    mem.sync_mirror()
    ws, wt = xavier_weights(K * A, seed, _dt(kw), hist, H, W), xavier_weights(K * A, seed + 100, _dt(kw), hist, H, W)
    net = sd.DeepQNetwork(A, args)
    net.set_weights(wt, 1); net.set_weights(ws, 0)
    assert net.bootstrap_heads == K and net.num_actions == A
    o = BO.BootstrapOracle(A, K, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=_dt(kw), weights=ws,
                           half_activations=kw.get("datatype") == "float16", n_step=n,
                           mask_probability=getattr(args, "bootstrap_mask_probability", 1.0), mask_seed=args.random_seed)
    o.Wt = [w.copy() for w in wt]
    valid = BO.valid_slots(om, n)
    return net, o, mem, om, valid


def _batch(om, valid, B, seed, n=1, must=None):
    idx = np.random.RandomState(seed).choice(valid, B, replace=len(valid) < B).astype(np.int64)
    if must is not None:
        idx[B // 2] = must
    mb = NO.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
    return idx, mb


def _check_grads(net, regime, g):
    """the rules of tests/test_gpu_munchausen.py::_check_grads"""
    B, _, kw = _regime(regime)[:3]
    for i in range(5):
        gg, ref = np.asarray(net.get_layer(i, 3), np.float64), np.asarray(g[i], np.float64)
        rel = np.linalg.norm(gg - ref) / max(np.linalg.norm(ref), 1e-300)
        print("%s layer %d: grad max abs err %.3e of %.3e, rel norm %.3e" % (regime, i, np.abs(gg - ref).max(), np.abs(ref).max(), rel))
        if kw.get("datatype") == "float64":
            assert rel < 1e-11, i
        elif kw.get("datatype") == "float16":
            assert rel < 5e-2, i
        elif B >= 128:
            assert rel < 1e-2, i
        else:
            assert np.abs(gg - ref).max() < 1e-4 * max(1e-3, np.abs(ref).max()), i


def _check_step(net, o, regime, g, cost_ref, preq, cost):
    tol = max(_regime(regime)[3], 1e-6)
    K, A = o.heads, o.game_actions
    q, mq = net.last_q()
    scale = max(1.0, float(np.abs(preq).max()))
    eq, em = np.abs(q - preq).max(), np.abs(mq - o.last_maxq).max()
    dmax = 1.0 + scale + max(1.0, float(np.abs(o.last_maxq).max()))      # |delta| <= |Q| + |r_c| + gamma |Q'|
    ec = abs(float(cost) - float(cost_ref))
    print("%s A=%d K=%d: Q(pre) err %.3e, maxq err %.3e, cost %.6g vs %.6g (err %.3e)" % (regime, A, K, eq, em, cost, cost_ref, ec))
    assert q.shape == (o.batch_size, K * A)
    assert eq < tol * scale
    assert em < 3 * tol * max(1.0, float(np.abs(o.last_maxq).max()))
    e = 3 * tol * scale
    assert ec < dmax * e + 0.5 * e * e
    _check_grads(net, regime, g)


@pytest.mark.parametrize("regime,A,K", CASES)
def test_one_step_parity(sd, regime, A, K):
    B = REGIMES[regime][0]
    net, o, mem, om, valid = _setup(sd, regime, A, K)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 5)
    o.indexes = idx
    g, cost_ref, deltas, preq = o.gradients(mb)
    # the K targets of a sample differ (different draws per head): a library that used one target for all heads fails below
    spread = np.ptp(o.fprop(o.Wt, o._normalize(mb[3])).reshape(B, K, A).max(2), axis=1)
    assert (spread > 1e-2).mean() > 0.5
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, regime, g, cost_ref, preq, cost)


def _random_minibatch(B, A, geom, seed, p_term=0.05):
    """a minibatch as tests/test_gpu_double_dqn.py::_minibatch draws it (uniform pixels, rewards -2 .. 2)"""
    hist, H, W = geom
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, (B, hist, H, W), dtype=np.uint8)
    post = rng.randint(0, 256, (B, hist, H, W), dtype=np.uint8)
    return pre, rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64), post, rng.rand(B) < p_term


@pytest.mark.parametrize("regime,A,K", CASES)
def test_three_free_running_steps(sd, regime, A, K):
    """Hold-out Q rows and every layer's weights after three free-running steps, within the regime's free-running bound of
    tests/test_gpu_munchausen.py's CONFIGS (float32 B = 128: 2e-3, the figure tests/test_gpu_double_dqn.py holds fp32_b256 to).
    Every regime is fed from the ring but float32 B = 128, which takes the minibatches tests/test_gpu_double_dqn.py's free-running
    test takes (uniform-pixel tuples through train(), mask probability 1); its ring-fed steps are held step by step in
    test_three_teacher_forced_ring_steps_b128 below (why: DESIGN.md §27.3)."""
    B, geom, kw, tol, tol10 = REGIMES[regime]
    net, o, mem, om, valid = _setup(sd, regime, A, K, seed=21)
    for s in range(3):
        if regime == "fp32_b128":
            mb = _random_minibatch(B, A, geom, 100 + s)
            o.indexes = None
            net.train(mb)
        else:
            idx, mb = _batch(om, valid, B, 30 + s)
            o.indexes = idx
            net.train_indexes(mem, idx)
        o.train(mb)
    hold = _random_minibatch(B, A, geom, 99)[0] if regime == "fp32_b128" else om.gather(_batch(om, valid, B, 99)[0])[0]
    ref, got = o.predict_heads(hold), net.predict_heads(hold)
    assert got.shape == (B, K, A)
    err, qmax = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s A=%d K=%d: hold-out Q max abs err after 3 steps %.3e" % (regime, A, K, err))
    assert err < tol10 * max(1.0, qmax)
    for i in range(5):
        we = float(np.abs(np.asarray(net.get_layer(i), np.float64) - o.W[i]).max())
        print("   layer %d weight max abs err %.3e" % (i, we))
        assert we < tol10 * max(1.0, float(np.abs(o.W[i]).max())), i
    assert np.abs(net.predict(hold) - ref.mean(axis=1)).max() < tol10 * max(1.0, qmax)      # predict: the head-mean [B][A]


@pytest.mark.parametrize("A,K", [(2, 2), (4, 2), (3, 6)])
def test_three_teacher_forced_ring_steps_b128(sd, A, K):
    """float32 B = 128 fed from the ring, as tests/test_gpu_double_dqn.py::test_ten_teacher_forced_steps holds its B = 256: before every
    step the net takes the oracle's weights and optimizer state, and each step's Q rows, bootstrap value, cost and gradients are held to
    the one-step rules"""
    regime, B = "fp32_b128", 128
    net, o, mem, om, valid = _setup(sd, regime, A, K, seed=21)
    net.set_option("keep_gradients", 1)
    for s in range(3):
        net.set_weights(o.W, 0)
        for i in range(5):
            net.set_layer(i, o.S[i], 2)
        idx, mb = _batch(om, valid, B, 30 + s)
        o.indexes = idx
        g, cost_ref, _, preq = o.gradients(mb)
        cost = net.train_indexes(mem, idx, want_cost=True)
        _check_step(net, o, regime, g, cost_ref, preq, cost)
        o.optimize(g, B)


def _layers(net):
    return [np.array(net.get_layer(i, w)) for w in (0, 2) for i in range(5)]


@pytest.mark.parametrize("kw", [{}, dict(datatype="float16")])
def test_one_head_is_inert(sd, kw):
    """K = 1: three steps leave the weights and the optimizer state of a net built without the flag, from the same launches"""
    A, B = 4, 32
    ws, wt = xavier_weights(A, 81), xavier_weights(A, 181)
    rng = np.random.RandomState(80)
    mbs = [(rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64),
            rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.rand(B) < 0.1) for _ in range(3)]
    nets = [sd.DeepQNetwork(A, make_args(batch_size=B, bootstrap_heads=1, bootstrap_mask_probability=1.0, **kw)), sd.DeepQNetwork(A, make_args(batch_size=B, **kw))]
    counts = []
    for net in nets:
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        counts.append(_counts(net, lambda: [net.train(mb) for mb in mbs], n=1))
    assert counts[0] == counts[1]
    for a, b in zip(_layers(nets[0]), _layers(nets[1])):
        assert np.array_equal(a, b)
    assert np.array_equal(nets[0].predict(mbs[0][0]), nets[1].predict(mbs[0][0]))


def test_masks(sd):
    """P = 0.5, (A = 3, K = 6), B = 32: dq is non-zero exactly where the mask is 1; a sampled slot with an all-zero mask (seed and slot found on
    the CPU: tests/test_bootstrap.py asserts the search) has an all-zero dq row, an all-zero d4 row and a zero cost term"""
    A, K, B = 3, 6, 32
    seed, slot = BO.empty_mask_case()
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, K, bootstrap_mask_probability=0.5, random_seed=seed)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 6, must=slot)
    o.indexes = idx
    g, cost_ref, deltas, preq = o.gradients(mb)
    assert not o.last_masks[B // 2].any() and 0.3 < o.last_masks.mean() < 0.7
    cost = net.train_indexes(mem, idx, want_cost=True)
    dq = net.debug_read("dq", B * K * A).reshape(B, K * A)
    d4 = net.debug_read("d4", B * 512).reshape(B, 512)
    terms = net.debug_read("cost_terms", B)
    want = np.zeros((B, K * A), bool)
    for n in range(B):
        for k in range(K):
            want[n, k * A + int(mb[1][n])] = bool(o.last_masks[n, k])
    assert np.array_equal(dq != 0, want & (deltas != 0)) and (want & (deltas != 0)).sum() > B
    assert np.abs(dq - deltas).max() < 1e-4
    assert not dq[B // 2].any() and not d4[B // 2].any() and terms[B // 2] == 0.0
    assert np.abs(d4).max() > 0 and np.abs(d4 - o.last_d4).max() < 1e-4 * max(1.0, np.abs(o.last_d4).max())
    assert np.abs(terms - o.last_cost_terms).max() < 1e-3 * max(1.0, float(o.last_cost_terms.max()))
    _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost)
    # the tuple path has no ring index: refused by name with P < 1, served with P = 1
    with pytest.raises(Exception) as ei:
        net.train(mb)
    assert "sdqn_net_train_host" in str(ei.value) and "bootstrap_mask_probability" in str(ei.value)
    net1, o1, _, _, _ = _setup(sd, "fp32_b32", A, K)
    net1.set_option("keep_gradients", 1)
    g1, c1, _, preq1 = o1.gradients(mb)
    net1.callback = type("CB", (), dict(on_train=lambda self, c: setattr(self, "cost", c)))()
    net1.train(mb)
    _check_step(net1, o1, "fp32_b32", g1, c1, preq1, net1.callback.cost)


def test_n_step_3(sd):
    A, K, B = 3, 2, 32
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, K, n=3)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 7, n=3)
    assert np.asarray(mb[4]).any() and not np.asarray(mb[4]).all()
    o.indexes = idx
    g, cost_ref, _, preq = o.gradients(mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost)


@pytest.mark.parametrize("what", ["clip_grad_norm", "target_tau"])
def test_three_steps_composed(sd, what):
    A, K, B = 3, 2, 32
    G, TAU = 0.02, 0.25
    extra = dict(clip_grad_norm=G) if what == "clip_grad_norm" else dict(target_tau=TAU)
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, K, seed=31, **extra)
    clipped = 0
    for s in range(3):
        idx, mb = _batch(om, valid, B, 40 + s)
        o.indexes = idx
        net.train_indexes(mem, idx)
        g, _, _, _ = o.gradients(mb)
        if what == "clip_grad_norm":
            g, norm, scale = clip_gradients(g, B, G, np.float32)
            clipped += int(scale < 1)
            n_lib, s_lib = net.last_grad_norm()
            assert abs(n_lib - norm) < 1e-3 * max(norm, 1e-3) and abs(s_lib - float(scale)) < 1e-3
        o.optimize(g, B)
        if what == "target_tau":
            o.Wt = [blend(w, wt, TAU, np.float32) for w, wt in zip(o.W, o.Wt)]
    assert what != "clip_grad_norm" or clipped > 0
    tol10 = REGIMES["fp32_b32"][4]
    hold = om.gather(_batch(om, valid, B, 98)[0])[0]
    for which, ow in ((0, o.W), (1, o.Wt)):
        err = np.abs(np.asarray(net.get_layer(4, which), np.float64) - ow[4]).max()
        assert err < tol10 * max(1.0, float(np.abs(ow[4]).max())), (which, err)
    ref = o.predict_heads(hold)
    assert np.abs(net.predict_heads(hold) - ref).max() < tol10 * max(1.0, float(np.abs(ref).max()))


# ---- acting ---------------------------------------------------------------------------------------------------------------------
def _cargs(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=2, eval_envs=0, train_envs=0, batch_size=32)
    d.update(kw)
    return make_args(**d)


def _disagreeing_heads(net, K, A, prefer, seed=3):
    """Xavier torso; fc5 row k A + a = c / 512 with c = 2 for head k's preferred action and 1 otherwise: Q_k[a] = c mean(a4), so head k's
    greedy action is prefer[k] wherever a4 is not all zero"""
    ws = xavier_weights(K * A, seed)
    w5 = np.ones((K * A, 512), np.float32) / 512
    for k in range(K):
        w5[k * A + prefer[k]] *= 2
    ws[4] = w5
    net.set_weights(ws, 0)
    return ws


def test_collect_follows_one_head_per_episode(sd):
    N, steps, K, A = 4, 70, 3, 3
    args = _cargs(bootstrap_heads=K, random_seed=9)
    net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(N * 40, args)
    mem.set_lanes(N)
    prefer = [2, 0, 1]
    _disagreeing_heads(net, K, A, prefer)
    out = net.collect(env, mem, N, steps, 0.0, seed=77, trace=True)
    o = CollectOracle(N, N * 40, 4, 84, 84, 77, env.balls_per_episode)
    heads_seen = set()
    for t in range(steps):
        ks = [BO.head_of(9, K, e, int(o.tally["episodes"][e])) for e in range(N)]
        heads_seen.update(ks)
        if t % 10 == 0 or t == steps - 1:
            states = np.zeros((32, 4, 84, 84), np.uint8); states[:N] = o.games.states
            raw = net.predict_heads(states)[:N]
            for e in range(N):
                assert np.abs(raw[e, ks[e]] - out["q"][t][e]).max() < 1e-5, (t, e)       # tr_q holds the selected row (test_gpu_dqn.Q_TOL's order)
                assert raw[e, ks[e]].max() == 0 or int(np.argmax(raw[e, ks[e]])) == prefer[ks[e]]
        a, r, term = o.lockstep(0.0, out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(term, out["terminals"][t]), t
        for e in range(N):
            if out["q"][t][e].max() > 0:
                assert a[e] == prefer[ks[e]], (t, e)
    assert out["episodes"].min() >= 2 and len(heads_seen) >= 2 and out["q"].max() > 0
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k


def test_evaluate_votes_and_breaks_ties_low(sd):
    N, steps, A = 4, 30, 3
    args = _cargs(bootstrap_heads=2, random_seed=9)
    net, env = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1)
    _disagreeing_heads(net, 2, A, [2, 1])                  # one vote each for actions 2 and 1: the tie goes to action 1
    out = net.evaluate(env, N, steps, epsilon=0.0, seed=5, trace=True)
    live = out["q"].max(axis=2) > 0
    assert live.any()
    assert (out["actions"][live] == 1).all()
    assert np.array_equal(out["q"][live], np.tile(np.array([0, 1, 1], np.float32), (int(live.sum()), 1)))      # the vote counts
    net3 = sd.DeepQNetwork(A, _cargs(bootstrap_heads=3, random_seed=9))
    _disagreeing_heads(net3, 3, A, [2, 0, 2])
    out = net3.evaluate(env, N, steps, epsilon=0.0, seed=5, trace=True)
    live = out["q"].max(axis=2) > 0
    assert live.any() and (out["actions"][live] == 2).all()


def test_collect_with_one_head_is_the_parent_and_more_heads_add_one_launch(sd):
    N, steps, A = 4, 25, 3
    res, counts = [], []
    for kw in (dict(bootstrap_heads=1), {}, dict(bootstrap_heads=2)):
        args = _cargs(random_seed=4, **kw)
        net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(N * 40, args)
        mem.set_lanes(N)
        if "bootstrap_heads" not in kw or kw["bootstrap_heads"] == 1:
            net.set_weights(xavier_weights(A, 5), 0)
        out = net.collect(env, mem, N, steps, 0.3, seed=77, trace=True)
        res.append((out, np.array(mem.screens), np.array(mem.actions), np.array(mem.rewards), np.array(mem.terminals)))
        counts.append(_counts(net, lambda: net.collect(env, mem, N, 5, 0.3), n=1))
    (o1, *r1), (o0, *r0) = res[0], res[1]
    for a, b in zip(r1, r0):
        assert np.array_equal(a, b)
    for k in o0:
        assert np.array_equal(o1[k], o0[k]), k
    assert counts[0] == counts[1]
    assert sum(counts[2].values()) == sum(counts[1].values()) + 5, (counts[2], counts[1])


def test_single_environment_acting(sd):
    """sdqn_net_act_greedy and the Agent on one environment: while collecting, the Q-head of copy 0's episode number (advanced by every
    fresh episode, in the library and in DeepQNetwork alike); while testing, the vote"""
    K, A, seed = 3, 3, 9
    prefer = [2, 0, 1]
    args = _cargs(bootstrap_heads=K, random_seed=seed, replay_size=400, random_starts=4, exploration_rate_test=0.0)
    net = sd.DeepQNetwork(A, args)
    _disagreeing_heads(net, K, A, prefer)
    buf = sd.DeviceStateBuffer(args)
    rng = np.random.RandomState(1)
    for _ in range(4):
        buf.add(rng.randint(1, 256, (84, 84), dtype=np.uint8))
    raw = net.predict_state(buf)
    assert raw.shape == (K * A,) and raw.max() > 0
    net.set_acting(False)
    net.next_episode(reset=True)
    seen = set()
    for ep in range(10):
        k = BO.head_of(seed, K, 0, ep)
        seen.add(k)
        assert net.act_greedy(buf) == prefer[k] == net.acting_action(raw), ep      # the library's counter and Python's agree
        net.next_episode()
    assert len(seen) >= 2
    net.set_acting(True)
    assert net.act_greedy(buf) == 0 == net.acting_action(raw)                      # one vote each for 2, 0, 1: the lowest action
    # the Agent: test() votes, train() follows the episode's head and starts a new episode at every terminal
    env, mem = sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(400, args)
    agent = sd.Agent(env, mem, net, args)
    log = []
    agent.callback = type("CB", (), dict(on_step=lambda self, a, r, t, s, e: log.append((a, t))))()
    agent.test(12)
    assert [a for a, _ in log] == [0] * 12
    del log[:]
    net.next_episode(reset=True)
    agent._epsilon = type("E", (), dict(at=lambda self, t: 0.0))()
    agent.train_frequency = 10 ** 9                                                 # acting only
    agent._acting_mode(False)
    agent._fresh_episode()
    ep = net._boot_episode
    for _ in range(60):
        want = prefer[BO.head_of(seed, K, 0, ep)]
        a, _, _, term = agent._advance(0.0)
        assert a == want
        if term:
            assert net._boot_episode == ep + 1
            ep += 1
    assert ep >= 3
