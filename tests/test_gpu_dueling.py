"""--dueling on the GPU against tests/dueling_oracle.py.

Train steps are fed from a 600-slot ring with terminals through train_indexes; online and target weights come from different dense Xavier
draws of an (A + 1)-output net, which the library and the oracle both mask.  The forward and the backward are the launches of an
(A + 1)-action net, so the bounds are the ones tests/test_gpu_quantile.py holds the quantile head to in the same regime: a stored row
within tol of the oracle's, what is read off the target net within 3 tol, gradients by _check_grads, free-running weights and hold-out rows
within the regime's free-running bound.  What follows from those by the rule's shape:
  * Q = V + Adv_a - mean(Adv) is a sum of three quantities that each carry at most tol scale: 3 tol scale (e_q; e_qt on the target's rows);
  * y = r + gamma max Q(theta-, s', .): e_qt;  delta = Q(theta, s, a_n) - y: e_delta = e_q + e_qt;
  * c = clip(delta) is 1-Lipschitz and |1[b = a_n] - 1 / A| <= 1: every dq entry within e_delta; the cost term 0.5 delta^2 has slope
    |delta|: e_delta max(1, max |delta|), and so has the cost, their mean.
In the oracle alone every sample's best and second-best Q(theta-, s', .) differ by more than 1e-4 and no |delta| lies within 1e-4 of the
clip (asserted, not filtered: the seeds were chosen on the CPU), so no maximum and no clip edge of a comparison is decided by rounding."""
import random

import numpy as np
import pytest

import bootstrap_oracle as BO
import dueling_oracle as DO
import nstep_oracle as NO
import per_oracle as P
from clip_oracle import clip_gradients
from collect_oracle import CollectOracle
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle
from soft_target_oracle import blend
from test_gpu_bootstrap import REGIMES as _BR, _batch, _cargs, _check_grads, _dt
from test_gpu_double_dqn import _counts
from util import make_args

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SIZE = 600
# tests/test_gpu_bootstrap.py's regimes (their tolerances at other batch sizes of the same datatype), and float64 on the generic path at the
# smallest screen the layer stack accepts, held to the float64 bounds of DESIGN.md §4c (tests/test_gpu_bootstrap.py: f64_b32)
REGIMES = dict(_BR, f64_small=(5, (4, 36, 38), dict(datatype="float64")) + _BR["f64_b32"][3:])
for _B in (33, 127):
    REGIMES["fp32_b%d" % _B] = (_B,) + _BR["fp32_b32"][1:]
REGIMES["fp32_b257"] = (257,) + _BR["fp32_b128"][1:]
# (regime, A, batch seed): the seed is the first from 5 on whose batch meets the gap conditions in the oracle (searched on the CPU)
CASES = [("fp32_b32", 3, 5), ("fp32_b32", 4, 5), ("fp32_b32", 17, 5), ("fp32_b32", 1, 5), ("fp32_b33", 3, 5), ("fp32_b127", 3, 5),
         ("fp32_b128", 3, 5), ("fp32_b257", 3, 5), ("fp16_b32", 3, 5), ("fp16_b128", 3, 5), ("f64_small", 3, 5)]
TEN_SEEDS = (30, 31, 32, 33, 34, 35, 36, 37, 38, 40)     # of the ten free-running steps' batches: 39 puts a |delta| 8.7e-5 from the clip
COLLECT = "catch_collect(lockstep)"              # the lockstep's name in the launch profile (tests/test_gpu_collect.py)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _regime(regime):
    return REGIMES[regime] if isinstance(regime, str) else regime


def _setup(sd, regime, A, seed=11, n=1, oracle_dtype=None, **extra):
    """(net, oracle, product ring, oracle ring, valid indexes); sd = None: the oracle's side alone (net and product ring None);
    oracle_dtype: the oracle's precision where it is not the net's (the float64 oracle of a float32 net, on the same float32 draws)"""
    B, (hist, H, W), kw = _regime(regime)[:3]
    args = make_args(batch_size=B, history_length=hist, screen_height=H, screen_width=W, **dict(kw, dueling=True, n_step=n, **extra))
    om = ReplayOracle(SIZE, H, W, hist, B)
    BO.fill_ring(om, A)
    ws, wt = xavier_weights(A + 1, seed, _dt(kw), hist, H, W), xavier_weights(A + 1, seed + 100, _dt(kw), hist, H, W)
    net = mem = None
    if sd is not None:
        mem = sd.ReplayMemory(SIZE, args)
        BO.fill_ring(mem, A)
        mem.sync_mirror()
        net = sd.DeepQNetwork(A, args)
        net.set_weights(wt, 1); net.set_weights(ws, 0)                       # dense: the library masks them
        assert net.dueling and net.num_actions == A
    o = DO.DuelingOracle(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=oracle_dtype or _dt(kw), weights=ws,
                         half_activations=kw.get("datatype") == "float16", n_step=n, optimizer=extra.get("optimizer", "rmsprop"))
    o.set_target(wt)
    return net, o, mem, om, BO.valid_slots(om, n)


def _gaps_clear(o):
    assert o.last["gaps"].min() > DO.GAP, "sample %d: best and second-best Q(theta-, s', .) differ by %.3e" % (int(o.last["gaps"].argmin()), o.last["gaps"].min())
    assert o.last["edges"].min() > DO.GAP, "sample %d: |delta| within %.3e of the clip" % (int(o.last["edges"].argmin()), o.last["edges"].min())


def _check_step(net, o, regime, g, cost_ref, preq, cost, mb):
    B, geom, kw = _regime(regime)[:3]
    tol = max(_regime(regime)[3], 1e-6)
    A, L = o.game_actions, o.last
    _gaps_clear(o)
    raw, mq = net.last_q()
    scale = max(1.0, float(np.abs(preq).max()))
    scale_t = max(1.0, float(np.abs(L["postq"]).max()))
    e_q, e_qt = 3 * tol * scale, 3 * tol * scale_t
    e_delta = e_q + e_qt
    dmax = max(1.0, float(np.abs(L["delta"]).max()))
    er, em, ec = np.abs(raw - preq).max(), np.abs(mq - L["maxq"]).max(), abs(float(cost) - float(cost_ref))
    print("%s A=%d: rows err %.3e (bound %.1e), maxq err %.3e (%.1e), cost %.6g vs %.6g (err %.3e, bound %.1e)"
          % (regime, A, er, tol * scale, em, e_qt, cost, cost_ref, ec, e_delta * dmax))
    assert raw.shape == (B, A + 1)
    assert er < tol * scale
    assert em < e_qt
    assert ec < e_delta * dmax
    y64, d64, dq64 = net.last_dueling_step()
    ey, ed, edq = np.abs(y64 - L["y"]).max(), np.abs(d64 - L["delta"]).max(), np.abs(dq64 - L["dq"]).max()
    print("   y err %.3e (%.1e), delta err %.3e (%.1e), dq err %.3e (%.1e)" % (ey, e_qt, ed, e_delta, edq, e_delta))
    assert y64.shape == (B,) and dq64.shape == (B, A + 1)
    assert ey < e_qt and ed < e_delta and edq < e_delta
    # the shape of the rows' gradient, exactly: row 0 carries c, the advantages c (1[b = a_n] - 1 / A) — a plain (A + 1)-action net
    # leaves one non-zero entry per row, a head without the -1 / A term zeros off the taken action
    c = dq64[:, 0]
    act = np.asarray(mb[1], np.int64)
    t = _dt(kw)
    on, off = float(t(1.0 - 1.0 / A)), float(t(-1.0 / A))
    for n in range(B):
        for b in range(A):
            assert dq64[n, 1 + b] == float(t(t(c[n]) * t(on if b == act[n] else off))), (n, b)
    assert (np.abs(c) > 0).sum() > B // 2
    if A > 1:
        assert (dq64[:, 1:] != 0).sum() == A * (c != 0).sum()
    if kw.get("datatype") != "float64" and geom == (4, 84, 84):                    # the tuned path's own buffers
        step = net.debug_read("dueling_step", 2 * B).reshape(2, B)
        dq = net.debug_read("dq", B * (A + 1)).reshape(B, A + 1)
        terms = net.debug_read("cost_terms", B)
        qq = net.debug_read("q", 2 * B * (A + 1)).reshape(2, B, A + 1)
        ect = np.abs(terms - L["cost_terms"]).max()
        print("   cost term err %.3e (%.1e)" % (ect, e_delta * dmax))
        assert ect < e_delta * dmax
        assert np.array_equal(step[0].astype(np.float64), y64) and np.array_equal(step[1].astype(np.float64), d64)
        assert np.array_equal(dq.astype(np.float64), dq64) and np.array_equal(qq[0], raw)
        # the device restates the host function on its own stored rows, bit for bit (float32 and float16 alike: the head is fp32)
        r = [float(x) for x in mb[2]] if o.n_step > 1 else [float(x) for x in np.clip(mb[2], -1.0, 1.0)]
        gam = NO.gamma_n(o.n_step, GAMMA) if o.n_step > 1 else GAMMA
        w = o.per_weights
        same = 0
        for n in range(B):
            ref = DO.sample(qq[0, n], qq[1, n], A, int(mb[1][n]), r[n], bool(mb[4][n]), gam, 1.0, np.float32,
                            None if w is None else w[n], o.per_alpha, o.per_eps)
            same += int(np.array_equal(ref["dq"].view(np.uint32), dq[n].view(np.uint32)) and ref["cost"].view(np.uint32) == terms[n].view(np.uint32)
                        and ref["y"].view(np.uint32) == step[0, n].view(np.uint32) and ref["delta"].view(np.uint32) == step[1, n].view(np.uint32)
                        and ref["maxq"].view(np.uint32) == mq[n].view(np.uint32))
        print("   %d of %d samples bit-identical to the host restatement on the device's own rows" % (same, B))
        assert same == B
    _check_grads(net, _regime(regime), g)
    g5 = np.asarray(net.get_layer(4, 3))
    assert (g5[~DO.mask(A)] == 0).all() and not np.signbit(g5[~DO.mask(A)]).any()     # the masked gradient: +0.0


def _masked_is_plus_zero(net, A, which=(0, 1)):
    m = DO.mask(A)
    for w in which:
        w5 = np.asarray(net.get_layer(4, w))
        assert (w5[~m] == 0).all() and not np.signbit(w5[~m]).any(), w
        assert (w5[m] != 0).mean() > 0.99


@pytest.mark.parametrize("regime,A,bseed", CASES)
def test_one_step_parity(sd, regime, A, bseed):
    B = REGIMES[regime][0]
    net, o, mem, om, valid = _setup(sd, regime, A)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, bseed)
    g, cost_ref, deltas, preq = o.gradients(mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, regime, g, cost_ref, preq, cost, mb)
    _masked_is_plus_zero(net, A)
    v, adv = net.predict_streams(mb[0])
    assert v.shape == (B,) and adv.shape == (B, A)
    assert np.array_equal(net.predict(mb[0]), np.stack([DO.q_values(np.concatenate([[v[n]], adv[n]]), A, _dt(REGIMES[regime][2])) for n in range(B)]))


def test_ten_free_running_ring_steps_b32(sd):
    """float32 B = 32, A = 3: hold-out rows, Q and every layer's weights after ten free-running ring-fed steps, within the regime's
    free-running bound.  The reference runs in float64 on the same float32 draws, as the other option heads' free-running tests do
    (DESIGN.md §28.3): the rule is continuous, a Rectlin gate is not, and a float32 reference contributes gate flips of its own — with a
    float32 oracle this comparison stood 2.1e-2 apart after ten steps while every one-step quantity agreed to 4e-7"""
    regime, A = "fp32_b32", 3
    B, geom, kw, tol, tol10 = REGIMES[regime]
    net, o, mem, om, valid = _setup(sd, regime, A, seed=21, oracle_dtype=np.float64)
    for bseed in TEN_SEEDS:
        idx, mb = _batch(om, valid, B, bseed)
        net.train_indexes(mem, idx)
        o.train(mb)
        _gaps_clear(o)
    hold = om.gather(_batch(om, valid, B, 99)[0])[0]
    ref, got = o.predict(hold), np.concatenate([net.predict_streams(hold)[0][:, None], net.predict_streams(hold)[1]], axis=1)
    err, qmax = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s A=%d: hold-out rows max abs err after 10 steps %.3e (bound %.1e)" % (regime, A, err, tol10 * max(1.0, qmax)))
    assert err < tol10 * max(1.0, qmax)
    for i in range(5):
        we = float(np.abs(np.asarray(net.get_layer(i), np.float64) - o.W[i]).max())
        print("   layer %d weight max abs err %.3e" % (i, we))
        assert we < tol10 * max(1.0, float(np.abs(o.W[i]).max())), i
    assert np.abs(net.predict(hold) - o.predict_q(hold)).max() < 3 * tol10 * max(1.0, qmax)
    _masked_is_plus_zero(net, A)


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam", "adadelta"])
def test_masked_entries_stay_plus_zero(sd, optimizer):
    """ten steps under each optimizer, then a dense set_weights, a hard target copy and ten more steps under --target_tau 0.01: every
    masked W5 entry of theta and of the target is +0.0 to the bit throughout"""
    regime, A, B = "fp32_b32", 3, 32
    net, o, mem, om, valid = _setup(sd, regime, A, seed=41, optimizer=optimizer)
    _masked_is_plus_zero(net, A)                                             # after initialisation and the dense set_weights of _setup
    w0 = np.asarray(net.get_layer(4, 0)).copy()
    for s in range(10):
        net.train_indexes(mem, _batch(om, valid, B, 50 + s)[0])
    _masked_is_plus_zero(net, A)
    assert (np.asarray(net.get_layer(4, 0))[DO.mask(A)] != w0[DO.mask(A)]).mean() > 0.5          # (the live entries did move)
    dense = np.random.RandomState(3).uniform(-1, 1, (A + 1, 512)).astype(np.float32)
    net.set_layer(4, dense, 0)
    assert np.array_equal(np.asarray(net.get_layer(4, 0)), DO.masked(dense))
    _masked_is_plus_zero(net, A, (0,))
    net.update_target_network()
    _masked_is_plus_zero(net, A)
    assert np.array_equal(np.asarray(net.get_layer(4, 1)), DO.masked(dense))
    net.set_target_tau(0.01)
    for s in range(10):
        net.train_indexes(mem, _batch(om, valid, B, 70 + s)[0])
    _masked_is_plus_zero(net, A)
    assert not np.array_equal(np.asarray(net.get_layer(4, 1)), DO.masked(dense))


@pytest.mark.parametrize("what", ["clip_grad_norm", "target_tau"])
def test_one_step_composed(sd, what):
    """--clip_grad_norm 10: last_grad_norm() is the oracle's norm of the MASKED gradient (the dense one is asserted to differ from it by
    more than the bound); --target_tau 0.01: the blend behind the step"""
    A, B, G, TAU = 3, 32, 10.0, 0.01
    extra = dict(clip_grad_norm=G) if what == "clip_grad_norm" else dict(target_tau=TAU)
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, seed=31, **extra)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 40)
    g, cost_ref, deltas, preq = o.gradients(mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    tol10 = REGIMES["fp32_b32"][4]
    if what == "clip_grad_norm":
        gc, norm, scale = clip_gradients(g, B, G, np.float32)
        dense = [x.copy() for x in g]
        dense[4] = (deltas.T @ o.last["a4"]).astype(np.float32)
        norm_dense = clip_gradients(dense, B, G, np.float32)[1]
        n_lib, s_lib = net.last_grad_norm()
        print("clip_grad_norm: norm %.6g vs %.6g (unmasked: %.6g), scale %.6g vs %.6g" % (n_lib, norm, norm_dense, s_lib, float(scale)))
        assert abs(n_lib - norm) < 1e-3 * max(norm, 1e-3) and abs(s_lib - float(scale)) < 1e-3
        assert abs(norm_dense - norm) > 1e-2 * norm
        _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)
        o.optimize(gc, B)
    else:
        _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)
        o.optimize(g, B)
        o.Wt = [blend(w, wt, TAU, np.float32) for w, wt in zip(o.W, o.Wt)]
    for which, ow in ((0, o.W), (1, o.Wt)):
        for i in (0, 4):
            err = np.abs(np.asarray(net.get_layer(i, which), np.float64) - ow[i]).max()
            assert err < tol10 * max(1.0, float(np.abs(ow[i]).max())), (which, i, err)
    _masked_is_plus_zero(net, A)


def test_n_step_3(sd):
    A, B = 3, 32
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, n=3)
    net.set_option("keep_gradients", 1)
    idx, mb = _batch(om, valid, B, 8, n=3)
    assert np.asarray(mb[4]).any() and not np.asarray(mb[4]).all()
    g, cost_ref, deltas, preq = o.gradients(mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost, mb)


def test_prioritized_replay(sd):
    """--prioritized_replay: the sampled indexes and the importance weights against per_oracle's sampler on the memory's own leaves, the
    step against the oracle fed those weights, the priorities written back against (|delta| + eps)^alpha of the oracle's delta"""
    A, B, ALPHA, EPS = 3, 32, 0.6, 1e-6
    per = dict(prioritized_replay=True, priority_alpha=ALPHA, priority_beta=0.4, priority_epsilon=EPS, priority_beta_steps=1000)
    net, o, mem, om, valid = _setup(sd, "fp32_b32", A, seed=61, **per)
    mem.set_priorities(0, np.random.RandomState(5).uniform(0.05, 2.0, SIZE).astype(np.float32))      # (slots that cannot be sampled keep leaf 0)
    net.set_option("keep_gradients", 1)
    leaf = mem.priorities()
    random.seed(21)
    st = random.getstate()
    cost = net.train_from_memory(mem, 1, want_cost=True)
    idx, w = mem.last_sample()
    r = random.Random(); r.setstate(st)
    assert np.array_equal(idx, P.sample(leaf, P.uniforms(r, B)))
    np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)
    assert np.ptp(w) > 0.2                                                   # (the weights do differ across the batch: a weighted step)
    o.per_weights, o.per_alpha, o.per_eps = w, ALPHA, EPS
    mb = om.gather(idx)
    g, cost_ref, deltas, preq = o.gradients(mb)
    _check_step(net, o, "fp32_b32", g, cost_ref, preq, cost if cost is not None else cost_ref, mb)
    newp = P.new_priority(np.abs(o.last["delta"]), ALPHA, EPS)
    pr = mem.priorities()
    last = {int(i): k for k, i in enumerate(idx)}
    np.testing.assert_allclose(np.array([pr[i] for i in last]), np.array([newp[k] for k in last.values()]), rtol=1e-4)


def test_launches_per_step_and_flag_off_is_the_parent(sd):
    """flag off: three steps leave the weights and the optimizer state of a net built without the flag bit for bit, from the same launches
    and the same step structure (the route and step-trace goldens, which tests/test_dueling.py regenerates, hold the rest).  Flag on: a
    step is the clipped step's split tail with one mask launch and without the two clip launches — two launches more than the default step"""
    A, B = 4, 32
    ws, wt = xavier_weights(A, 81), xavier_weights(A, 181)
    rng = np.random.RandomState(80)
    mbs = [(rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.randint(0, A - 1, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64),
            rng.randint(0, 256, (B, 4, 84, 84), dtype=np.uint8), rng.rand(B) < 0.1) for _ in range(3)]
    nets = [sd.DeepQNetwork(A, make_args(batch_size=B, dueling=False)), sd.DeepQNetwork(A, make_args(batch_size=B)),
            sd.DeepQNetwork(A - 1, make_args(batch_size=B, dueling=True)), sd.DeepQNetwork(A, make_args(batch_size=B, clip_grad_norm=10.0))]
    counts = []
    for net in nets:
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        counts.append(_counts(net, lambda: [net.train(mb) for mb in mbs], n=1))
    on = C_int(sd, nets[0])
    assert on == 0 and C_int(sd, nets[2]) == 1
    assert counts[0] == counts[1] and nets[0].step_structure() == nets[1].step_structure()
    for which in (0, 1, 2):
        for i in range(5):
            assert np.array_equal(np.array(nets[0].get_layer(i, which)), np.array(nets[1].get_layer(i, which))), (which, i)
    assert np.array_equal(nets[0].predict(mbs[0][0]), nets[1].predict(mbs[0][0]))
    total = [sum(c.values()) for c in counts]
    print("launches per three steps: default %d, dueling %d, clipped %d" % (total[1], total[2], total[3]))
    assert total[2] == total[1] + 3 * 2                                      # mode 1 + mask + mode 2 in the place of the one update launch
    assert total[2] == total[3] - 3 * 1                                      # the clipped step's tail, one launch where it has two


def C_int(sd, net):
    import ctypes
    v = ctypes.c_int(-1)
    sd._lib.check(sd.load().sdqn_net_get_dueling(net._h, ctypes.byref(v)))
    return v.value


def test_refusals_in_the_library_in_either_order(sd):
    lib = sd.load()
    net = sd.DeepQNetwork(3, make_args(dueling=True))
    for call, word in ((lambda: net.set_option("double_dqn", 1), "double_dqn"), (lambda: net.set_munchausen(True), "munchausen"),
                       (lambda: net.set_advantage_learning(0.5, False), "advantage_learning"),
                       (lambda: sd._lib.check(lib.sdqn_net_set_bootstrap(net._h, 2, 1.0, 0)), "bootstrap_heads"),
                       (lambda: sd._lib.check(lib.sdqn_net_set_quantiles(net._h, 2)), "quantiles")):
        with pytest.raises(Exception) as ei:
            call()
        assert "dueling" in str(ei.value) and word in str(ei.value), str(ei.value)
    for arm, word in ((lambda h: h.set_option("double_dqn", 1), "double_dqn"), (lambda h: h.set_munchausen(True), "munchausen"),
                      (lambda h: h.set_advantage_learning(0.5, False), "advantage_learning"),
                      (lambda h: sd._lib.check(lib.sdqn_net_set_bootstrap(h._h, 2, 1.0, 0)), "bootstrap_heads"),
                      (lambda h: sd._lib.check(lib.sdqn_net_set_quantiles(h._h, 2)), "quantiles")):
        other = sd.DeepQNetwork(4, make_args())
        arm(other)
        with pytest.raises(Exception) as ei:
            sd._lib.check(lib.sdqn_net_set_dueling(other._h, 1))
        assert "dueling" in str(ei.value) and word in str(ei.value), str(ei.value)
    bn = sd.DeepQNetwork(4, make_args(batch_norm=True))
    with pytest.raises(Exception) as ei:
        sd._lib.check(lib.sdqn_net_set_dueling(bn._h, 1))
    assert "dueling" in str(ei.value) and "batch_norm" in str(ei.value)


# ---- acting ---------------------------------------------------------------------------------------------------------------------
def _spread(net, A, seed=3):
    """Xavier torso and a Xavier fc5 scaled up, so that the action values differ visibly on the game's frames"""
    ws = xavier_weights(A + 1, seed)
    ws[4] = (ws[4] * 8).astype(np.float32)
    net.set_weights(ws, 0)


def _raw_rows(net, states, Nenv):
    st = np.zeros((32, 4, 84, 84), np.uint8); st[:Nenv] = states
    v, adv = net.predict_streams(st)
    return np.concatenate([v[:Nenv, None], adv[:Nenv]], axis=1)


def test_collect_acts_on_the_dueling_rule(sd):
    Nenv, steps, A = 32, 50, 3
    args = _cargs(dueling=True, random_seed=9)
    net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(Nenv * 60, args)
    mem.set_lanes(Nenv)
    _spread(net, A)
    out = net.collect(env, mem, Nenv, steps, 0.0, seed=77, trace=True)
    o = CollectOracle(Nenv, Nenv * 60, 4, 84, 84, 77, env.balls_per_episode)
    seen = set()
    for t in range(steps):
        raw = _raw_rows(net, o.games.states, Nenv)
        for e in range(Nenv):
            assert np.array_equal(DO.q_values(raw[e], A), out["q"][t][e]), (t, e)          # tr_q holds the Q row, the oracle's to the bit
            assert DO.act(raw[e], A) == out["actions"][t][e], (t, e)
        a, r, term = o.lockstep(0.0, out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(term, out["terminals"][t]), t
        seen.update(int(x) for x in a)
    assert len(seen) >= 2
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k


def test_evaluate_acts_on_the_dueling_rule(sd):
    from catch_oracle import EvalOracle
    Nenv, steps, A = 32, 50, 3
    args = _cargs(dueling=True, random_seed=9)
    net, env = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1)
    _spread(net, A)
    out = net.evaluate(env, Nenv, steps, epsilon=0.0, seed=5, trace=True)
    assert out["q"].shape == (steps, Nenv, A)
    o = EvalOracle(Nenv, net.history_length, env.dims[0], env.dims[1], 0.0, 5, env.balls_per_episode)
    seen = set()
    for t in range(steps):
        raw = _raw_rows(net, o.states, Nenv)
        for e in range(Nenv):
            assert np.array_equal(DO.q_values(raw[e], A), out["q"][t][e]), (t, e)
            assert DO.act(raw[e], A) == out["actions"][t][e], (t, e)
        a, r, term = o.step(out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(term, out["terminals"][t]), t
        seen.update(int(x) for x in a)
    assert len(seen) >= 2
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k


def test_launches_per_lockstep(sd):
    """a dueling lockstep is the forward's launches plus two: dueling_q_kernel and the game's kernel (a standard lockstep: plus one)"""
    Nenv, A = 32, 3
    counts = []
    for kw in ({}, dict(dueling=True)):
        args = _cargs(random_seed=4, **kw)
        net, env, mem = sd.DeepQNetwork(A, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(Nenv * 40, args)
        mem.set_lanes(Nenv)
        net.collect(env, mem, Nenv, 2, 0.3, seed=77)
        counts.append(_counts(net, lambda: net.collect(env, mem, Nenv, 5, 0.3), n=1))
    fwd = sum(counts[0].values()) - counts[0][COLLECT]
    assert counts[0][COLLECT] == 5 and fwd % 5 == 0
    assert sum(counts[1].values()) == fwd + 2 * 5, (counts[1], counts[0])
    assert counts[1][COLLECT] == 10


def test_single_environment_acting(sd):
    """sdqn_net_act_greedy and DeepQNetwork.acting_action on one environment, and Agent's loop through them"""
    A = 3
    args = _cargs(dueling=True, random_seed=9, replay_size=400, random_starts=4, exploration_rate_test=0.0)
    net = sd.DeepQNetwork(A, args)
    _spread(net, A)
    buf = sd.DeviceStateBuffer(args)
    rng = np.random.RandomState(1)
    for k in range(6):
        buf.add(rng.randint(1, 256, (84, 84), dtype=np.uint8))
        raw = net.predict_state(buf)
        assert raw.shape == (A + 1,)
        assert net.act_greedy(buf) == DO.act(raw, A) == net.acting_action(raw), k
    env, mem = sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(400, args)
    agent = sd.Agent(env, mem, net, args)
    log = []
    agent.callback = type("CB", (), dict(on_step=lambda self, a, r, t, s, e: log.append(a)))()
    agent.test(12)
    assert len(log) == 12 and all(0 <= a < A for a in log)
