"""--random_shift on the GPU against its numpy restatement (tests/shift_oracle.py).

The oracles of the step itself are the ones the other options' tests use (OracleDQN and its Double DQN / n-step / prioritized / dueling
restatements), fed the oracle-shifted minibatch: a library that ignores the option, shifts by other offsets, shifts the two states alike
or hands one of the step's forwards an unshifted state misses the byte comparison or the parity bounds."""
import random

import numpy as np
import pytest

import dueling_oracle as DO
import nstep_oracle as N
import per_oracle as P
import shift_oracle as S
import test_gpu_dueling as TD
import test_gpu_nstep as NS
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill
from test_gpu_bootstrap import REGIMES as _BR
from test_gpu_bootstrap import _batch
from test_gpu_double_dqn import _check_maxpostq
from util import make_args

pytestmark = pytest.mark.gpu

SEED = 123                     # make_args' --random_seed: the stream of every default test net's shifts
GAMMA, MINR, MAXR = NS.GAMMA, NS.MINR, NS.MAXR
SHIFT = "shift_gather(random_shift)"      # the launch's own row in the profile (kernel id 20)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _cfg(B, dt=None, geom=(4, 84, 84), A=4):
    """a configuration of tests/test_gpu_nstep.py's form, with that file's (= tests/test_gpu_dqn.py's) bounds per datatype"""
    kw = {} if dt is None else dict(datatype=dt)
    tol = {None: 1e-4, "float16": 3e-3, "float64": 1e-9}[dt]
    return (A, B, geom, kw, tol, tol)


def _shifted(mb, seed, step, Pad):
    spre, spost, d = S.shift_minibatch(np.asarray(mb[0]), np.asarray(mb[3]), seed, step, Pad)
    return (spre, mb[1], mb[2], spost, mb[4]), d


# ---- 1. kernel exactness ---------------------------------------------------------------------------------------------------------------
EXACT = [("84x84x4 P=4", _cfg(8), 4, SEED), ("84x84x4 P=8", _cfg(8), 8, SEED), ("36x38x4 float64 P=3", _cfg(8, "float64", (4, 36, 38)), 3, SEED),
         ("84x84x4 P=2 forced corners", _cfg(8), 2, None)]


@pytest.mark.parametrize("name,cfg,Pad,seed", EXACT, ids=[e[0] for e in EXACT])
def test_kernel_bytes_equal_the_oracle(sd, name, cfg, Pad, seed):
    A, B, (hist, H, W), kw, _, _ = cfg
    if seed is None:
        seed = S.forced_seed(B, Pad)
        assert seed is not None and seed < 1000
    mem, om = NS._mems(sd, cfg, 1, size=200)
    net = sd.DeepQNetwork(A, NS._args(cfg, 1))
    net.set_random_shift(Pad, seed)
    idx = NS._sample(mem, 1, 5)
    assert len(set(idx.tolist())) > 1
    net.train_indexes(mem, idx)
    pre, post = mem.device_minibatch()
    opre, _, _, opost, _ = om.gather(idx)
    (spre, _, _, spost, _), d = _shifted((opre, None, None, opost, None), seed, 0, Pad)
    assert np.array_equal(net.last_shifts(), d)
    assert np.array_equal(pre, spre) and np.array_equal(post, spost)
    assert not np.array_equal(pre, opre) and not np.array_equal(post, opost)
    assert (d[:, 0] != d[:, 1]).any()                          # the two states of a sample draw their own offsets
    if Pad == 8:                                               # every clamp edge: some state is pushed past each of the four borders
        assert d[..., 0].min() < 0 < d[..., 0].max() and d[..., 1].min() < 0 < d[..., 1].max()
    if name.endswith("forced corners"):
        flat = d.reshape(-1, 2)
        assert (flat == -Pad).all(axis=1).any() and (flat == Pad).all(axis=1).any()
    assert net.random_shift_steps() == 1
    # the next step draws under the next counter value
    net.train_indexes(mem, idx)
    assert np.array_equal(net.last_shifts(), S.draws(seed, 1, B, Pad)) and not np.array_equal(net.last_shifts(), d)


# ---- 2. step parity --------------------------------------------------------------------------------------------------------------------
def _sync_from_oracle(net, o):
    net.set_weights(o.W, 0); net.set_weights(o.Wt, 1); net.set_weights(o.S, 2)


PARITY = [("fp32_b2", _cfg(2)), ("fp32_b32", _cfg(32)), ("fp32_b33", _cfg(33)), ("fp32_b128", _cfg(128)), ("fp16_b32", _cfg(32, "float16"))]


@pytest.mark.parametrize("name,cfg", PARITY, ids=[p[0] for p in PARITY])
def test_one_step_and_three_teacher_forced_steps(sd, name, cfg):
    """every step restarted from the oracle's (theta, theta-, s): Q, max Q', the cost and every gradient at tests/test_gpu_dqn.py's bounds for
    the regime, on the oracle-shifted minibatch of that step's counter value"""
    A, B, geom, kw, tol, _ = cfg
    Pad = 4
    mem, om = NS._mems(sd, cfg, 1, size=600)
    ws, wt = NS._weights(cfg, 11)
    net = NS._net(sd, cfg, 1, ws, wt, random_shift=Pad)
    assert net.random_shift == Pad
    net.set_option("keep_gradients", 1)
    o = NS._oracle(cfg, 1, ws, wt)
    ctol = 5e-3 if kw.get("datatype") == "float16" else 1e-5
    for s in range(4):                                         # the one step, then three teacher-forced ones
        idx = NS._sample(mem, 1, 5 + s)
        assert net.random_shift_steps() == s
        mb, d = _shifted(om.gather(idx), SEED, s, Pad)
        mb = tuple(np.array(x) for x in mb)
        if s:
            _sync_from_oracle(net, o)
        g, cost_ref, _, preq = NS._grads(o, mb)
        cost = net.train_indexes(mem, idx, want_cost=True)
        assert np.array_equal(net.last_shifts(), d), s
        print("%s step %d: cost %.6g vs %.6g" % (name, s, cost, float(cost_ref)))
        assert abs(cost - float(cost_ref)) < ctol * max(1.0, float(cost_ref)), s
        NS._check_q(net, o, preq, tol)
        NS._check_grads(net, cfg, g)
        o.train(mb)


COMPOSED = ["double_dqn", "n_step_3", "prioritized_replay", "dueling", "bootstrap_heads", "munchausen"]


@pytest.mark.parametrize("what", COMPOSED)
def test_one_step_composed(sd, what):
    B, Pad = 8, 4
    cfg = _cfg(B)
    A, _, geom, kw, tol, _ = cfg
    if what == "dueling":
        regime = (B, geom, {}) + _BR["fp32_b32"][3:]
        A = 3
        net, o, mem, om, valid = TD._setup(sd, regime, A, random_shift=Pad)
        net.set_option("keep_gradients", 1)
        for bseed in range(5, 25):                             # the first batch whose SHIFTED states meet the oracle's gap conditions
            idx, mb = _batch(om, valid, B, bseed)
            smb, d = _shifted(mb, SEED, 0, Pad)
            g, cost_ref, _, preq = o.gradients(smb)
            if o.last["gaps"].min() > DO.GAP and o.last["edges"].min() > DO.GAP:
                break
        cost = net.train_indexes(mem, idx, want_cost=True)
        assert np.array_equal(net.last_shifts(), d)
        TD._check_step(net, o, regime, g, cost_ref, preq, cost, smb)
        return
    if what == "bootstrap_heads":                              # masks with probability 0.5: keyed by ring index, which the shifted step must still hand the head
        import test_gpu_bootstrap as TB
        regime = (B, geom, {}) + _BR["fp32_b32"][3:]
        net, o, mem, om, valid = TB._setup(sd, regime, 3, 3, bootstrap_mask_probability=0.5, random_shift=Pad)
        net.set_option("keep_gradients", 1)
        idx, mb = _batch(om, valid, B, 5)
        smb, d = _shifted(mb, SEED, 0, Pad)
        o.indexes = idx
        g, cost_ref, _, preq = o.gradients(smb)
        cost = net.train_indexes(mem, idx, want_cost=True)
        assert np.array_equal(net.last_shifts(), d)
        TB._check_step(net, o, regime, g, cost_ref, preq, cost)
        return
    if what == "munchausen":                                   # the target net's forward over the prestates reads the shifted prestates too
        import test_gpu_munchausen as TM
        mem, om = NS._mems(sd, cfg, 1, size=600)
        ws, wt = NS._weights(cfg, 11)
        net = TM._net(sd, cfg, ws, wt, random_shift=Pad)
        assert net.munchausen
        net.set_option("keep_gradients", 1)
        o = TM._oracle(cfg, ws, wt)
        idx = NS._sample(mem, 1, 5)
        smb, d = _shifted(om.gather(idx), SEED, 0, Pad)
        g, _, _, preq = o.gradients(smb)
        net.train_indexes(mem, idx)
        assert np.array_equal(net.last_shifts(), d)
        TM._check_q(net, o, preq, tol)
        TM._check_grads(net, cfg, g)
        return
    if what == "prioritized_replay":
        import test_gpu_per as TP
        size = 600
        mem = TP._mem(sd, size, B, A=A)
        rng = np.random.RandomState(3)
        mem.set_priorities(0, (10.0 ** rng.uniform(-2, 1, size)).astype(np.float32))
        om = ReplayOracle(size, batch_size=B)
        synthetic_fill(om, 3, num_actions=A)
        om.terminals[np.arange(7, size, 97)] = True
        ws = xavier_weights(A, 11)
        net = sd.DeepQNetwork(A, make_args(batch_size=B, random_shift=Pad))
        net.set_weights(ws, 0); net.update_target_network()
        net.set_option("keep_gradients", 1)
        o = P.PEROracle(A, batch_size=B, weights=ws)
        o.Wt = [w.copy() for w in ws]
        leaf = mem.priorities()
        pm0 = mem.max_priority
        random.seed(21)
        st = random.getstate()
        net.train_from_memory(mem, 1)
        idx, w = mem.last_sample()                             # as tests/test_gpu_per.py::test_one_step: indexes, weights, new priorities
        r = random.Random(); r.setstate(st)
        assert np.array_equal(idx, P.sample(leaf, P.uniforms(r, B)))
        np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)
        o.weights = w
        smb, d = _shifted(om.gather(idx), SEED, 0, Pad)
        assert np.array_equal(net.last_shifts(), d)
        g, cost, _, preq = o.gradients(smb)
        q, _ = net.last_q()
        assert np.abs(q - preq).max() < tol * max(1.0, float(np.abs(preq).max()))
        NS._check_grads(net, cfg, g)
        newp = P.new_priority(o.last_abs_delta, TP.ALPHA, TP.EPS)
        pr = mem.priorities()
        last = {int(i): k for k, i in enumerate(idx)}
        got = np.array([pr[i] for i in last]); exp = np.array([newp[k] for k in last.values()])
        assert abs(mem.max_priority - max(pm0, float(exp.max()))) <= 1e-3 * mem.max_priority
        np.testing.assert_allclose(got, exp, rtol=1e-5)
        return
    n = 3 if what == "n_step_3" else 1
    extra = dict(double_dqn=True) if what == "double_dqn" else {}
    mem, om = NS._mems(sd, cfg, n, size=600)
    ws, wt = NS._weights(cfg, 11)
    net = NS._net(sd, cfg, n, ws, wt, random_shift=Pad, **extra)
    net.set_option("keep_gradients", 1)
    o = NS._oracle(cfg, n, ws, wt, cls=N.NStepOracleDDQN if what == "double_dqn" else None)
    idx = NS._sample(mem, n, 5)
    mb = N.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
    smb, d = _shifted(mb, SEED, 0, Pad)
    g, _, _, preq = NS._grads(o, smb)
    net.train_indexes(mem, idx)
    assert np.array_equal(net.last_shifts(), d)
    if what == "double_dqn":                                   # the online net's argmax pass reads the same shifted poststate
        q, mq = net.last_q()
        assert np.abs(q - preq).max() < tol * max(1.0, float(np.abs(preq).max()))
        _check_maxpostq(mq, o, tol)
    else:
        NS._check_q(net, o, preq, tol)
    NS._check_grads(net, cfg, g)


# ---- 3. / 4. launches ------------------------------------------------------------------------------------------------------------------
def _counts(net, fn):
    net.profile(True, -1); net.profile_reset()
    fn()
    net.sync()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


def _ring(sd, B, A=4, size=600, **kw):
    args = make_args(batch_size=B, **kw)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    return mem, args


def _state(net):
    return [np.asarray(net.get_layer(i, w)) for w in (0, 1, 2) for i in range(5)]


def test_p0_is_todays_step(sd):
    A, B = 4, 32
    ws = xavier_weights(A, 4)
    res = []
    for setter in (False, True):
        mem, args = _ring(sd, B)
        net = sd.DeepQNetwork(A, args)
        net.set_weights(ws, 0); net.update_target_network()
        if setter:
            net.set_random_shift(0, 77)
        random.seed(2)
        c = _counts(net, lambda: net.train_from_memory(mem, 5))
        res.append((_state(net), c, random.getstate()))
        assert net.random_shift_steps() == 0
    assert res[0][1] == res[1][1] and SHIFT not in res[0][1]
    assert res[0][2] == res[1][2]
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("B", [32, 256])
def test_one_added_launch_per_step(sd, B):
    """a shifted ring step = the step that reads a device minibatch in place (train(getMinibatch()) on untouched views) + one launch; the
    ring loop's one prep launch per call stays"""
    A, n = 4, 3
    mem, args = _ring(sd, B, size=1200)
    std = sd.DeepQNetwork(A, args)
    random.seed(1)

    def tuples():
        for _ in range(n):
            std.train(mem.getMinibatch())
    c_std = _counts(std, tuples)
    assert std.tuple_counters()[1] == n                        # every one of them read the device minibatch in place
    net = sd.DeepQNetwork(A, make_args(batch_size=B, random_shift=4))
    random.seed(1)
    c = _counts(net, lambda: net.train_from_memory(mem, n))
    gather, prep = SHIFT, "prep(idx+meta)"
    assert c[gather] == n and c[prep] == 1 and gather not in c_std and prep not in c_std
    assert {k: v for k, v in c.items() if k not in (gather, prep)} == c_std


# ---- 5. determinism and independence ---------------------------------------------------------------------------------------------------
def test_determinism_and_independence(sd):
    A, B = 4, 32
    ws = xavier_weights(A, 4)
    out = []
    for Pad, seed in ((4, 9), (4, 9), (4, 10), (0, 9)):
        mem, args = _ring(sd, B)
        net = sd.DeepQNetwork(A, args)
        net.set_weights(ws, 0); net.update_target_network()
        net.set_random_shift(Pad, seed)
        random.seed(6)
        net.train_from_memory(mem, 5)
        out.append((_state(net), net.last_shifts() if Pad else None, random.getstate(), net.random_shift_steps()))
    (w0, s0, r0, t0), (w1, s1, r1, t1), (w2, s2, r2, t2), (w3, _, r3, t3) = out
    assert (t0, t1, t2, t3) == (5, 5, 5, 0)
    assert np.array_equal(s0, s1) and np.array_equal(s0, S.draws(9, 4, B, 4))
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)
    assert not np.array_equal(s0, s2) and np.array_equal(s2, S.draws(10, 4, B, 4))
    assert not all(np.array_equal(a, b) for a, b in zip(w0, w2))
    assert not all(np.array_equal(a, b) for a, b in zip(w0, w3))          # the option moves the weights at all
    assert r0 == r1 == r2 == r3                                # Python's stream: index sampling is what it is with the option off


# ---- 6. acting is untouched ------------------------------------------------------------------------------------------------------------
def test_acting_is_untouched(sd):
    from test_gpu_collect import _args, _device_ring
    ws = xavier_weights(3, 31)
    res = []
    rng = np.random.RandomState(0)
    states = rng.randint(0, 256, (32, 4, 84, 84), dtype=np.uint8)
    for Pad in (0, 4):
        args = _args(batch_size=32, random_shift=Pad)
        net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(32 * 40, args)
        assert net.random_shift == Pad
        side, _ = _ring(sd, 32, A=3)                           # a train step first (shifted on the second net): whatever it leaves behind —
        random.seed(8)                                         # the device minibatch, its generation, the step counter — must not reach acting
        net.train_from_memory(side, 2)
        assert net.random_shift_steps() == (2 if Pad else 0)
        net.set_weights(ws, 0); net.update_target_network()
        mem.set_lanes(32)
        q = net.predict(states)
        ev = net.evaluate(env, 32, 12, 0.05, seed=3, trace=True)
        co = net.collect(env, mem, 32, 12, 0.5, seed=5, trace=True)
        res.append((q, ev, co, _device_ring(mem)))
    (q0, e0, c0, d0), (q1, e1, c1, d1) = res
    assert np.array_equal(q0, q1) and np.array_equal(d0, d1)
    for a, b in ((e0, e1), (c0, c1)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 7. the main loop ------------------------------------------------------------------------------------------------------------------
def test_main_loop(sd, tmp_path):
    from simple_dqn_amd import main as M
    csv = str(tmp_path / "shift.csv")
    args = M.build_parser().parse_args(
        ["--environment", "catch", "--train_envs", "32", "--random_shift", "4", "--replay_size", "3200", "--random_steps", "320",
         "--train_steps", "2000", "--test_steps", "0", "--epochs", "1", "--exploration_decay_steps", "1000", "--target_steps", "256",
         "--random_seed", "7", "--csv_file", csv])
    stats = M.run(args)
    assert stats.net.random_shift == 4 and stats.net.random_shift_steps() == stats.net.train_iterations > 0
    assert open(csv).read().count("\n") >= 2


# ---- a pending getMinibatch() survives a shifted step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["train_from_memory", "train_indexes"])
def test_pending_minibatch_survives_a_shifted_step(sd, how):
    """getMinibatch() leaves its states on the device only; the shifted step writes that very buffer, so the lazy views are fetched first and
    still read the gather of their own indexes, next to their own (a, r, t)"""
    A, B = 4, 8
    cfg = _cfg(B)
    mem, om = NS._mems(sd, cfg, 1, size=600)
    net = sd.DeepQNetwork(A, make_args(batch_size=B, random_shift=4))
    random.seed(12)
    idx = np.array(mem.sample_indexes(), dtype=np.int64)
    mb = mem.gather(idx)
    if how == "train_from_memory":
        net.train_from_memory(mem, 2)
    else:
        net.train_indexes(mem, NS._sample(mem, 1, 13))
    opre, oact, orew, opost, oterm = om.gather(idx)
    assert np.array_equal(np.asarray(mb[0]), opre) and np.array_equal(np.asarray(mb[3]), opost)
    assert np.array_equal(mb[1], oact) and np.array_equal(mb[2], orew) and np.array_equal(mb[4], oterm)
    pre, post = mem.device_minibatch()                          # ... while the device minibatch holds the last step's shifted states
    assert not np.array_equal(pre, opre)
