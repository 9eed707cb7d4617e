"""--advantage_learning / --persistent_advantage on the GPU against the advantage-learning restatement of the numpy oracles
(tests/advantage_oracle.py).  Configurations, bounds and gradient rules are those of tests/test_gpu_munchausen.py.

Online and target weights come from different Xavier draws.  Every parity test first checks, on the oracle alone, that the AL targets lie
far from the standard ones on at least half of the samples, that (PAL) each branch of its max is taken on a non-terminal sample and that
(B >= 32) some sample has a gap of exactly zero: a library that ignores alpha, reads the wrong q slot or drops the PAL branch fails the
comparison that follows.  No sample is left out of any comparison: both maxima are continuous in the Q-values.

The oracle of a float32 net runs in float64 on the same float32 draws (as tests/test_gpu_batch_edges.py's does), against the float32 bounds of
the table: the targets are continuous but a Rectlin gate is not, and a float32 reference decides the gates within its own rounding of
zero by that rounding.  Measured on this file's minibatches: where the float32 oracle and the library differed by 1e-2 in
a gradient, the library stood 1.4e-7 from the float64 oracle and the float32 oracle 7e-3 from it.  float16 nets keep the half oracle."""
import random

import numpy as np
import pytest

import advantage_oracle as AO
import nstep_oracle as N
import per_oracle as P
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from test_gpu_double_dqn import _counts, _minibatch
from test_gpu_munchausen import CONFIGS, _cfg, _check_grads, _check_priorities, _dt, _layers
from test_gpu_nstep import GAMMA, MAXR, MINR, _mems, _per_kw
from util import make_args

pytestmark = pytest.mark.gpu

ALPHA = 0.9
ERR_ARG = -1                                                 # include/sdqn.h: SDQN_ERR_ARG


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _kw(pal, alpha=ALPHA):
    return dict(advantage_learning=alpha, persistent_advantage=pal)


def _oracle(name, ws, wt, pal, cls=AO.AdvantageOracle, A=None, **attrs):
    A0, B, (hist, H, W), kw, _, _ = _cfg(name)
    half = kw.get("datatype") == "float16"
    o = cls(A or A0, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=np.float32 if half else np.float64, weights=ws,
            half_activations=half)
    o.Wt = [np.array(w, dtype=o.dtype) for w in wt]
    o.advantage_learning, o.persistent_advantage = ALPHA, pal
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _net(sd, name, ws, wt, pal, A=None, **extra):
    A0, B, geom, kw, _, _ = _cfg(name)
    al = _kw(pal); al.update(extra)
    net = sd.DeepQNetwork(A or A0, make_args(batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2], **kw, **al))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    return net


def _discriminates(o, mb, tol, pal, B):
    """On the oracle alone.  |y_AL - y_std| = alpha gap(qbar(s), a) exceeds `far` on at least half of the samples, far = 100 x the Q bound, or
    10 x where 100 x would exceed the configuration's median alpha gap; PAL: each branch of the max on a non-terminal sample; B >= 32: a
    sample whose gap is exactly zero."""
    d = ALPHA * o.last_gap_pre
    far = 100 * tol if 100 * tol <= float(np.median(d)) else 10 * tol
    live = ~np.asarray(mb[4], bool)
    ok = (d > far).mean() >= 0.5
    if pal:
        ok = ok and o.last_pal_took_post[live].any() and (~o.last_pal_took_post[live]).any()
    if B >= 32:
        ok = ok and (o.last_gap_pre == 0.0).any()
    return bool(ok)


def _setup(sd, name, seed, mb, pal, **extra):
    """net + oracle from different Xavier draws on which mb discriminates (the seed is walked until it does)"""
    A, B, geom, kw, tol, _ = _cfg(name)
    for s in range(seed, seed + 20):
        ws, wt = xavier_weights(A, s, _dt(kw), *geom), xavier_weights(A, s + 100, _dt(kw), *geom)
        o = _oracle(name, ws, wt, pal)
        o.gradients(mb)
        if _discriminates(o, mb, max(tol, 1e-6), pal, B):
            return _net(sd, name, ws, wt, pal, **extra), _oracle(name, ws, wt, pal)
    pytest.fail("no pair of draws on which the advantage-learning targets discriminate")


def _maxq_ref(o, mb):
    return o.fprop(o.Wt, o._normalize(mb[3])).max(1)


def _check_q(net, preq, maxq, tol):
    """Q(pre), and maxq = max_a qbar(s')[a] as the standard step reports it"""
    tol = max(tol, 1e-6)                                     # (last_q returns float32)
    q, mq = net.last_q()
    eq, ev = np.abs(q - preq).max(), np.abs(mq - maxq).max()
    print("Q(pre) max abs err %.3e, maxq max abs err %.3e" % (eq, ev))
    assert eq < tol * max(1.0, float(np.abs(preq).max()))
    assert ev < 3 * tol * max(1.0, float(np.abs(maxq).max()))


@pytest.mark.parametrize("pal", [False, True], ids=["al", "pal"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_step_parity(sd, name, pal):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 5)
    net, o = _setup(sd, name, 11, mb, pal)
    net.set_option("keep_gradients", 1)
    g, cost, _, preq = o.gradients(mb)
    assert _discriminates(o, mb, max(tol, 1e-6), pal, B)
    print("%s: alpha gap median %.3f max %.3f, zero gaps %d, PAL took post %d" % (name, np.median(ALPHA * o.last_gap_pre),
          (ALPHA * o.last_gap_pre).max(), (o.last_gap_pre == 0).sum(), o.last_pal_took_post.sum()))
    net.train(mb)
    _check_q(net, preq, o.last_post_target_q.max(1), tol)
    _check_grads(net, name, g)


@pytest.mark.parametrize("pal", [False, True], ids=["al", "pal"])
@pytest.mark.parametrize("name", ["fp32_b32", "fp16_b32", "f64_b8", "f32_generic"])
def test_ten_free_running_steps_with_target_sync(sd, name, pal):
    A, B, geom, kw, tol, tol10 = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 100 + s, p_term=0.05) for s in range(10)]
    net, o = _setup(sd, name, 21, mbs[0], pal)
    for s in range(10):
        if s == 5:
            net.update_target_network(); o.update_target_network()
        net.train(mbs[s])
        o.train(mbs[s])
    hold = _minibatch(B, A, geom, 99)[0]
    ref = o.predict(hold)
    err = np.abs(net.predict(hold) - ref).max()
    print("%s: Q max abs err after 10 steps %.3e" % (name, err))
    assert err < tol10 * max(1.0, float(np.abs(ref).max()))


def _force(net, o):
    """teacher forcing: the net takes the oracle's online weights and optimizer state.  The oracle first rounds both to the net's storage
    precision (a float64 oracle of a float32 net), so that the two sides hold the same numbers: a copy that differs in the last float32 bit
    moves a Rectlin pre-activation that lies within 1e-7 of zero across it, and that gate's whole delta with it"""
    o.W = [np.asarray(w, net._np).astype(o.dtype) for w in o.W]
    o.S = [np.asarray(x, net._np).astype(o.dtype) for x in o.S]
    net.set_weights(o.W, 0)
    for i in range(5):
        net.set_layer(i, o.S[i], 2)


@pytest.mark.parametrize("pal", [False, True], ids=["al", "pal"])
def test_ten_teacher_forced_steps_b128(sd, pal):
    """float32 B = 128, the other launch structure: held step by step across a target sync (why not free-running: DESIGN.md §27.3)"""
    name = "fp32_b128"
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 100 + s, p_term=0.05) for s in range(10)]
    net, o = _setup(sd, name, 21, mbs[0], pal)
    net.set_option("keep_gradients", 1)
    for s in range(10):
        _force(net, o)
        if s == 5:
            o.update_target_network()
            net.set_weights(o.Wt, 1)
        g, _, _, preq = o.gradients(mbs[s])
        net.train(mbs[s])
        _check_q(net, preq, o.last_post_target_q.max(1), tol)
        _check_grads(net, name, g)
        o.optimize(g, B)


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_one_action_and_alpha_zero_are_bit_identical_to_standard(sd, name):
    """A = 1: gap = +0 exactly; alpha = 0: nothing new runs.  Three steps leave the weights of a standard net"""
    A, B, geom, kw, _, _ = CONFIGS[name]
    for acts, alphas in ((1, (ALPHA, None)), (A, (0.0, None))):
        mbs = [_minibatch(B, acts, geom, 40 + s) for s in range(3)]
        ws, wt = xavier_weights(acts, 41, _dt(kw), *geom), xavier_weights(acts, 141, _dt(kw), *geom)
        nets = []
        for alpha in alphas:
            extra = {} if alpha is None else dict(advantage_learning=alpha, persistent_advantage=bool(alpha))
            net = sd.DeepQNetwork(acts, make_args(batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2], **kw, **extra))
            net.set_weights(wt, 1); net.set_weights(ws, 0)
            nets.append(net)
        assert nets[0].advantage_learning == alphas[0] and nets[1].advantage_learning == 0.0
        counts = [_counts(net, lambda: [net.train(mb) for mb in mbs], n=1) for net in nets]
        if alphas[0] == 0.0:
            assert counts[0] == counts[1]                    # the same launches
        for a, b in zip(_layers(nets[0]), _layers(nets[1])):
            assert np.array_equal(a, b)
        assert np.array_equal(nets[0].last_q()[1], nets[1].last_q()[1])


@pytest.mark.parametrize("pal", [False, True], ids=["al", "pal"])
@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_all_terminal_and_exact_ties(sd, name, pal):
    """every sample terminal: y = r_c - alpha gap(qbar(s), a), PAL = AL; equal fc5 rows in the target net: every qbar row is exactly tied, both
    gaps are exactly zero and y = y_std.  Q, maxq and gradients within bound, no device error flag"""
    A, B, geom, kw, tol, _ = CONFIGS[name]
    pre, act, rew, post, term = _minibatch(B, A, geom, 8)
    ws, wt = xavier_weights(A, 61, _dt(kw), *geom), xavier_weights(A, 161, _dt(kw), *geom)
    # all terminal
    net, o = _net(sd, name, ws, wt, pal), _oracle(name, ws, wt, pal)
    net.set_option("keep_gradients", 1)
    mb = (pre, act, rew, post, np.ones(B, bool))
    g, _, _, preq = o.gradients(mb)
    assert np.abs(o.last_y - (np.clip(rew, -1, 1) - ALPHA * o.last_gap_pre)).max() <= 1e-12 and not o.last_pal_took_post.any()
    assert (ALPHA * o.last_gap_pre > 100 * max(tol, 1e-6)).mean() >= 0.5
    net.train(mb)
    net.sync()                                               # (raises on a device error flag)
    _check_q(net, preq, o.last_post_target_q.max(1), tol)
    _check_grads(net, name, g)
    # exact ties
    wt[4][:] = wt[4][0]
    net, o = _net(sd, name, ws, wt, pal), _oracle(name, ws, wt, pal)
    net.set_option("keep_gradients", 1)
    mb = (pre, act, rew, post, term)
    g, _, _, preq = o.gradients(mb)
    assert np.array_equal(o.last_gap_pre, np.zeros(B)) and np.array_equal(o.last_gap_post, np.zeros(B))
    assert np.array_equal(o.last_y, o.last_y_std)
    net.train(mb)
    net.sync()
    _check_q(net, preq, o.last_post_target_q.max(1), tol)
    _check_grads(net, name, g)
    std = _net(sd, name, ws, wt, pal, advantage_learning=0.0, persistent_advantage=False)      # ... and bit for bit the standard step's
    std.set_option("keep_gradients", 1)
    std.train(mb)
    for i in range(5):
        assert np.array_equal(net.get_layer(i, 3), std.get_layer(i, 3)), i


def _fc4_margin(o, mb):
    """smallest |pre-activation| of the fc4 Rectlin on mb's prestates at the oracle's online weights"""
    _, (_, _, a3f, _) = o.fprop(o.W, o._normalize(mb[0]), keep=True)
    return float(np.abs(a3f @ o._h(o.W[3]).T).min())


def _ring_seed(name, mem, om, ws, wt, pal, cls, n):
    """On the oracle alone: the first sampling seed from 17 on whose three uniform minibatches keep every fc4 pre-activation further than
    1e-6 from zero.  The step's gradient is discontinuous in those: the float32 sum of fc4's 3136 products carries ~1e-7 of rounding, a unit
    inside it is gated by summation order, and its whole delta (it reaches every conv layer) comes or goes with it.  Measured with seed 17:
    step 2 holds such a unit — at one set of weights the library stood 1.4e-7 from the float64 oracle and the float32 oracle 7e-3 from it, at
    weights 1e-8 away the library 7e-3 from the float64 oracle."""
    B = _cfg(name)[1]
    for seed in range(17, 37):
        o = _oracle(name, ws, wt, pal, cls, n_step=n)
        random.seed(seed)
        ok = True
        for s in range(3):
            idx = np.array(mem.sample_indexes(), dtype=np.int64)
            mb = N.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
            ok = ok and _fc4_margin(o, mb) > 1e-6
            g = o.gradients(mb)[0]
            o.optimize(g, B)
            o.W = [np.asarray(w, np.float32).astype(o.dtype) for w in o.W]
        if ok:
            return seed
    pytest.fail("no sampling seed with a well-conditioned reference")


def _composed(sd, n, per, pal, name="fp32_b32"):
    """three teacher-forced steps through train_from_memory on a 600-slot ring with terminals against the combined oracle fed the same
    indexes: Q(pre), maxq, every gradient; PER: the priorities written back.  name: a configuration of CONFIGS that
    tests/test_gpu_nstep.py's CONFIGS (the ring's) holds too"""
    A, B, geom, kw, tol, _ = _cfg(name)
    per_kw = _per_kw() if per else {}
    mem, om = _mems(sd, name, n, size=600, **dict(_kw(pal), **per_kw))
    ws, wt = xavier_weights(A, 71, _dt(kw), *geom), xavier_weights(A, 171, _dt(kw), *geom)
    net = _net(sd, name, ws, wt, pal, n_step=n, **per_kw)
    net.set_option("keep_gradients", 1)
    cls = {(False, False): AO.AdvantageOracle, (True, False): AO.AdvantageOracleNStep,
           (False, True): AO.AdvantageOraclePER, (True, True): AO.AdvantageOraclePERNStep}[(n > 1, per)]
    o = _oracle(name, ws, wt, pal, cls, n_step=n)
    random.seed(17 if per else _ring_seed(name, mem, om, ws, wt, pal, cls, n))      # (PER samples by the net's priorities: no oracle-only walk)
    seen_done = False
    for s in range(3):
        _force(net, o)
        st = random.getstate()
        net.train_from_memory(mem, 1)
        if per:
            idx, w = mem.last_sample()
            o.weights = w
        else:
            after = random.getstate()
            random.setstate(st)
            idx = np.array(mem.sample_indexes(), dtype=np.int64)
            random.setstate(after)
        mb = N.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
        seen_done = seen_done or bool(np.asarray(mb[4]).any())
        g, _, _, preq = o.gradients(mb)
        far = 100 * tol
        if kw.get("datatype") == "float16" and far > float(np.median(ALPHA * o.last_gap_pre)):
            far = 10 * tol                                       # (_discriminates' fallback: 100 x 3e-3 exceeds the median alpha gap)
        assert (ALPHA * o.last_gap_pre > far).mean() >= 0.5
        _check_q(net, preq, o.last_post_target_q.max(1), tol)
        _check_grads(net, name, g)
        if per:
            _check_priorities(mem, idx, o, kw)
        o.optimize(g, B)
    assert seen_done


def test_composed_with_n_step(sd):
    _composed(sd, 3, False, False)


@pytest.mark.parametrize("pal", [False, True], ids=["al", "pal"])
def test_composed_with_prioritized_replay(sd, pal):
    _composed(sd, 1, True, pal)


def test_composed_with_both(sd):
    _composed(sd, 3, True, False)


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_switching_between_steps(sd, name):
    """AL 0.9 -> off -> PAL 0.5 -> AL 0.5 (persistent switched off alone): each step is the oracle's with the same settings"""
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 90 + s) for s in range(4)]
    net, o = _setup(sd, name, 91, mbs[0], False)
    net.set_option("keep_gradients", 1)
    for s, (alpha, pal) in enumerate(((ALPHA, False), (0.0, False), (0.5, True), (0.5, False))):
        net.set_advantage_learning(alpha, pal); o.advantage_learning, o.persistent_advantage = alpha, pal
        assert (net.advantage_learning, net.persistent_advantage) == (alpha, pal)
        _force(net, o)
        g, _, _, preq = o.gradients(mbs[s])
        net.train(mbs[s])
        _check_q(net, preq, _maxq_ref(o, mbs[s]), tol)
        _check_grads(net, name, g)
        o.optimize(g, B)
    net.set_advantage_learning(0.0)                          # off switches the persistent form off with it
    assert net.persistent_advantage is False


@pytest.mark.parametrize("kw,word", [(dict(double_dqn=True), "double_dqn"), (dict(munchausen=True), "munchausen"),
                                     (dict(bootstrap_heads=2), "bootstrap_heads"), (dict(batch_norm=True), "batch_norm"),
                                     (dict(n_step=2), "n_step"),
                                     (dict(double_dqn=True, datatype="float64", batch_size=8), "double_dqn"),
                                     (dict(munchausen=True, datatype="float64", batch_size=8), "munchausen")])
def test_library_refusals(sd, kw, word):
    net = sd.DeepQNetwork(2, make_args(**dict(dict(batch_size=32), **kw)))
    lib = sd.load()
    pal = 1 if word == "n_step" else 0
    rc = lib.sdqn_net_set_advantage_learning(net._h, 0.9, pal)
    msg = lib.sdqn_last_error().decode()
    assert rc == ERR_ARG and word in msg and ("persistent_advantage" if pal else "advantage_learning") in msg, msg
    assert net.train_iterations == 0
    for bad in ((1.0, 0), (-0.1, 0), (float("nan"), 0), (0.0, 1), (0.5, 2)):
        assert lib.sdqn_net_set_advantage_learning(net._h, *bad) == ERR_ARG, bad
    if word == "n_step":
        assert lib.sdqn_net_set_advantage_learning(net._h, 0.9, 0) == 0       # AL alone composes with n-step returns
        return
    if word == "batch_norm":
        return                                               # (batch_norm is fixed at creation: one order only)
    # the other order: the option on an advantage-learning net
    al = sd.DeepQNetwork(2, make_args(batch_size=kw.get("batch_size", 32), datatype=kw.get("datatype", "float32"), **_kw(True)))
    with pytest.raises(Exception) as ei:
        if word == "double_dqn":
            al.set_option("double_dqn", 1)
        elif word == "munchausen":
            al.set_munchausen(True)
        else:
            from simple_dqn_amd import _lib
            _lib.check(lib.sdqn_net_set_bootstrap(al._h, 2, 1.0, 0))
    assert "advantage_learning" in str(ei.value), str(ei.value)
    with pytest.raises(Exception) as ei:                     # PAL net, then n_step 2
        al.set_option("n_step", 2)
    assert "persistent_advantage" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("name", ["fp32_b32", "fp32_b128", "fp16_b32", "fp16_b128"])
def test_launches_per_step(sd, name):
    """an advantage-learning step = the standard step's launches + the launches of one predict of that net (+5 float32, +3 float16); the
    backward is the standard one"""
    A, B, geom, kw, _, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 50)
    ws, wt = xavier_weights(A, 52, _dt(kw), *geom), xavier_weights(A, 152, _dt(kw), *geom)
    al, std = _net(sd, name, ws, wt, True), _net(sd, name, ws, wt, False, advantage_learning=0.0)
    assert al.step_structure() == std.step_structure()
    c_al = _counts(al, lambda: al.train(mb))
    c_std = _counts(std, lambda: std.train(mb))
    c_fwd = _counts(std, lambda: std.predict(mb[0]))
    print(name, c_al, c_std, c_fwd)
    assert sum(c_fwd.values()) == 3 * (3 if kw.get("datatype") == "float16" else 5)       # (_counts runs its callable three times)
    for k in set(c_al) | set(c_std) | set(c_fwd):
        assert c_al.get(k, 0) == c_std.get(k, 0) + c_fwd.get(k, 0), (k, c_al, c_std, c_fwd)
    for k in c_std:                                          # ids no forward issues (the backward and the optimizer): unchanged
        if k not in c_fwd:
            assert c_al[k] == c_std[k], k
    al.set_advantage_learning(0.0)                           # switched off between steps: the standard step again
    assert _counts(al, lambda: al.train(mb)) == c_std


def test_fused_loop_equals_tuple_api(sd):
    A, B, size = 4, 32, 5000
    args = make_args(batch_size=B, **_kw(True))
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    ws, wt = xavier_weights(A, 61), xavier_weights(A, 161)
    nets = []
    for _ in range(3):
        net = sd.DeepQNetwork(A, args if len(nets) < 2 else make_args(batch_size=B))
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        nets.append(net)
    n1, n2, n3 = nets
    random.seed(6)
    for _ in range(3):
        st = random.getstate()
        n1.train(mem.getMinibatch())
        random.setstate(st)
        n2.train_from_memory(mem, 1)
    for a, b in zip(_layers(n1), _layers(n2)):
        assert np.array_equal(a, b)
    random.seed(6)                                           # and the option is honoured on the fused loop: a standard net moves elsewhere
    n3.train_from_memory(mem, 3)
    assert not np.array_equal(n1.get_layer(4), n3.get_layer(4))


def test_agent_fused_loop_equals_tuple_api(sd):
    """Agent(fused=True) trains through train_from_memory, Agent(fused=False) through net.train(mem.getMinibatch())"""
    res = []
    for fused in (True, False):
        args = make_args(batch_size=32, replay_size=2000, random_steps=0, train_frequency=4, train_repeat=1, target_steps=16,
                         exploration_decay_steps=100, **_kw(False))
        random.seed(3)
        env = sd.SyntheticEnvironment(args, num_actions=4, seed=1)
        mem = sd.ReplayMemory(2000, args)
        net = sd.DeepQNetwork(4, args)
        net.set_weights(xavier_weights(4, 5), 0); net.update_target_network()
        agent = sd.Agent(env, mem, net, args, fused=fused)
        agent.play_random(200)
        agent.train(12, 0)
        res.append(_layers(net))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_main_loop_on_catch_with_train_envs(sd, tmp_path):
    from simple_dqn_amd import main as M
    csv = tmp_path / "al.csv"
    args = M.build_parser().parse_args(
        ["--environment", "catch", "--train_envs", "4", "--replay_size", "800", "--random_steps", "160", "--train_steps", "240",
         "--test_steps", "40", "--epochs", "1", "--exploration_decay_steps", "200", "--target_steps", "64", "--random_seed", "7",
         "--advantage_learning", "0.9", "--persistent_advantage", "true", "--csv_file", str(csv)])
    stats = M.run(args)
    assert stats.net.advantage_learning == 0.9 and stats.net.persistent_advantage is True and stats.net.train_iterations > 0
    assert csv.read_text().count("\n") >= 2
