"""--munchausen on the GPU against the Munchausen restatement of the numpy oracles (tests/munchausen_oracle.py).

Online and target weights come from different Xavier draws.  Every parity test first checks, on the oracle alone, that the Munchausen
targets lie far from the standard ones on at least half of the non-terminal samples and that the bonus is clipped on some samples and not
on others: a library that ignores the option, or one of its three parameters, fails the comparison that follows."""
import random

import numpy as np
import pytest

import munchausen_oracle as MO
import nstep_oracle as N
import per_oracle as P
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from test_gpu_double_dqn import CONFIGS as _DD, _counts, _minibatch
from test_gpu_nstep import GAMMA, MAXR, MINR, _mems, _per_kw
from util import make_args

pytestmark = pytest.mark.gpu

# name: (A, B, screen (hist, H, W), make_args keywords, Q tolerance, 10-step Q tolerance): the bounds of tests/test_gpu_double_dqn.py
# (B = 128, the first batch size of the other launch structure, and the A = 5 bucket take those of their datatype)
CONFIGS = {
    "fp32_b32": _DD["fp32_b32"],
    "fp32_b128": (4, 128, (4, 84, 84), {}, _DD["fp32_b256"][4], _DD["fp32_b256"][5]),
    "fp16_b32": _DD["fp16_b32"],
    "fp16_b128": (4, 128, (4, 84, 84), dict(datatype="float16"), _DD["fp16_b256"][4], _DD["fp16_b256"][5]),
    "f64_b8": _DD["f64_b8"],
    "f32_generic": _DD["f32_generic"],
    "a18_ragged": _DD["a18_ragged"],
    "a5_b3": (5, 3, (4, 84, 84), {}, 1e-4, 1e-4),
}
ALPHA, TAU, L0 = 0.9, 0.03, -0.05
MU = dict(munchausen=True, munchausen_alpha=ALPHA, munchausen_tau=TAU, munchausen_clip=L0)


def _cfg(name):
    """a key of CONFIGS, or a configuration of its form itself (tests/test_gpu_option_head_edges.py passes its own)"""
    return CONFIGS[name] if isinstance(name, str) else name


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _dt(kw):
    return np.float64 if kw.get("datatype") == "float64" else np.float32


def _oracle(name, ws, wt, cls=MO.MunchausenOracle, dtype=None, **attrs):
    """dtype: the oracle's precision where it is not the net's (the float64 oracle of a float32 net)"""
    A, B, (hist, H, W), kw, _, _ = _cfg(name)
    o = cls(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=dtype or _dt(kw), weights=ws,
            half_activations=kw.get("datatype") == "float16")
    o.Wt = [np.array(w, dtype=o.dtype) for w in wt]
    o.munchausen_alpha, o.munchausen_tau, o.munchausen_clip = ALPHA, TAU, L0
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _net(sd, name, ws, wt, A=None, **extra):
    A0, B, geom, kw, _, _ = _cfg(name)
    mu = dict(MU); mu.update(extra)
    net = sd.DeepQNetwork(A or A0, make_args(batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2], **kw, **mu))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    return net


def _y_standard(o, mb):
    """the standard targets of the taken actions from the oracle's own target-net Q-values"""
    r = np.clip(mb[2], o.min_reward, o.max_reward).astype(np.float64)
    return np.where(mb[4], r, r + o.discount_rate * o.last_post_target_q.max(1).astype(np.float64))


def _discriminates(o, mb, tol):
    """On the oracle alone: Munchausen targets far from the standard ones on at least half of the non-terminal samples, and the bonus clipped
    on some samples and not on others.  The distance asked for is 100 x the Q bound where the parameters can reach it: |y - y_std| <=
    alpha |l0| + gamma tau ln A = 0.045 + 0.041 here, so the float16 bound of 3e-3 is held to 10 x (0.03) — 100 x (0.3) lies above what any
    draw can give with l0 = -0.05, while 10 x is still three times the 3 x tol that maxpostq is accepted at."""
    far = 100 * tol if 100 * tol < ALPHA * -L0 else 10 * tol
    live = ~np.asarray(mb[4], bool)
    d = np.abs(o.last_y - _y_standard(o, mb))
    lp = o.last_bonus / ALPHA
    clipped = lp <= L0
    return live.any() and (d[live] > far).mean() >= 0.5 and clipped.any() and (~clipped).any() and (lp[~clipped] < 0).any()


def _setup(sd, name, seed, mb, **extra):
    """net + oracle from different Xavier draws on which mb discriminates (the seed is walked until it does)"""
    A, B, geom, kw, tol, _ = _cfg(name)
    for s in range(seed, seed + 20):
        ws, wt = xavier_weights(A, s, _dt(kw), *geom), xavier_weights(A, s + 100, _dt(kw), *geom)
        o = _oracle(name, ws, wt)
        o.gradients(mb)
        if _discriminates(o, mb, max(tol, 1e-6)):
            return _net(sd, name, ws, wt, **extra), _oracle(name, ws, wt)
    pytest.fail("no pair of draws on which the Munchausen targets discriminate")


def _check_grads(net, name, g, layers=range(5)):
    """the rules of tests/test_gpu_double_dqn.py::_check_grads (B >= 128 float32: tests/test_gpu_nstep.py's relative norm, for its reason)"""
    A, B, _, kw, _, _ = _cfg(name)
    for i in layers:
        gg = np.asarray(net.get_layer(i, 3), np.float64)
        ref = np.asarray(g[i], np.float64)
        rel = np.linalg.norm(gg - ref) / max(np.linalg.norm(ref), 1e-300)
        print("%s layer %d: grad max abs err %.3e of %.3e, rel norm %.3e" % (name, i, np.abs(gg - ref).max(), np.abs(ref).max(), rel))
        if kw.get("datatype") == "float64":
            assert rel < 1e-11, i
        elif kw.get("datatype") == "float16":
            assert rel < 5e-2, i
        elif B >= 128:
            assert rel < 1e-2, i
        else:
            assert np.abs(gg - ref).max() < 1e-4 * max(1e-3, np.abs(ref).max()), i


def _check_q(net, o, preq, tol):
    tol = max(tol, 1e-6)                                     # (last_q returns float32)
    q, mq = net.last_q()
    eq, ev = np.abs(q - preq).max(), np.abs(mq - o.last_V).max()
    print("Q(pre) max abs err %.3e, V max abs err %.3e" % (eq, ev))
    assert eq < tol * max(1.0, float(np.abs(preq).max()))
    assert ev < 3 * tol * max(1.0, float(np.abs(o.last_V).max()))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_step_parity(sd, name):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 5)
    net, o = _setup(sd, name, 11, mb)
    net.set_option("keep_gradients", 1)
    g, cost, _, preq = o.gradients(mb)
    assert _discriminates(o, mb, max(tol, 1e-6))
    net.train(mb)
    _check_q(net, o, preq, tol)
    _check_grads(net, name, g)


@pytest.mark.parametrize("name", ["fp32_b32", "fp16_b32", "f64_b8", "f32_generic"])
def test_ten_free_running_steps_with_target_sync(sd, name):
    A, B, geom, kw, tol, tol10 = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 100 + s, p_term=0.05) for s in range(10)]
    net, o = _setup(sd, name, 21, mbs[0])
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


def _layers(net):
    return [np.array(net.get_layer(i)) for i in range(5)]


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_one_action_is_bit_identical_to_standard(sd, name):
    """A = 1: V = q and m = +0.0 exactly, so three steps leave the weights of a standard net"""
    _, B, geom, kw, _, _ = CONFIGS[name]
    mbs = [_minibatch(B, 1, geom, 40 + s) for s in range(3)]
    ws, wt = xavier_weights(1, 41, _dt(kw), *geom), xavier_weights(1, 141, _dt(kw), *geom)
    nets = [_net(sd, name, ws, wt, A=1), _net(sd, name, ws, wt, A=1, munchausen=False)]
    assert nets[0].munchausen and not nets[1].munchausen
    for net in nets:
        for mb in mbs:
            net.train(mb)
    for a, b in zip(_layers(nets[0]), _layers(nets[1])):
        assert np.array_equal(a, b)
    assert np.array_equal(nets[0].last_q()[1], nets[1].last_q()[1])


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_tiny_tau_stays_finite(sd, name):
    """tau = 1e-4: every non-maximal term of the sums underflows; finite, within bound of the oracle, no device error flag"""
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 6)
    ws, wt = xavier_weights(A, 51, _dt(kw), *geom), xavier_weights(A, 151, _dt(kw), *geom)
    net = _net(sd, name, ws, wt, munchausen_tau=1e-4)
    net.set_option("keep_gradients", 1)
    o = _oracle(name, ws, wt, munchausen_tau=1e-4)
    g, _, _, preq = o.gradients(mb)
    assert np.isfinite(o.last_V).all() and np.isfinite(o.last_bonus).all()
    net.train(mb)
    net.sync()                                               # (raises on a device error flag)
    assert np.isfinite(net.last_q()[0]).all() and np.isfinite(net.last_q()[1]).all()
    _check_q(net, o, preq, tol)
    _check_grads(net, name, g)


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_exact_ties_and_all_terminal(sd, name):
    """target fc5 weights zero: every qbar row is exactly zero, V = tau ln A and m = alpha max(l0, -tau ln A); every sample terminal:
    y = r_c + m, so delta = Q(pre)[a] - (r_c + m)"""
    A, B, geom, kw, tol, _ = CONFIGS[name]
    pre, act, rew, post, _ = _minibatch(B, A, geom, 8)
    ws, wt = xavier_weights(A, 61, _dt(kw), *geom), xavier_weights(A, 161, _dt(kw), *geom)
    wt[4] = np.zeros_like(wt[4])
    net = _net(sd, name, ws, wt)
    V, m = TAU * np.log(A), ALPHA * max(L0, -TAU * np.log(A))
    net.train((pre, act, rew, post, np.zeros(B, bool)))
    assert np.abs(net.last_q()[1] - V).max() <= 1e-6
    # all terminal, on a fresh net (same weights): the clipped deltas are those of y = r_c + m
    net = _net(sd, name, ws, wt)
    net.set_option("keep_gradients", 1)
    o = _oracle(name, ws, wt)
    mb = (pre, act, rew, post, np.ones(B, bool))
    g, _, _, preq = o.gradients(mb)
    assert np.abs(o.last_bonus - m).max() <= 1e-12 and np.abs(o.last_y - (np.clip(rew, -1, 1) + m)).max() <= 1e-12
    net.train(mb)
    q, mq = net.last_q()
    assert np.abs(mq - V).max() <= 1e-6
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    _check_grads(net, name, g)


def _check_priorities(mem, idx, o, kw):
    """the priorities written back for idx (the last occurrence of a slot wins) against those of the oracle's |delta|; float16: the
    relative 3e-3 tests/test_gpu_per.py::test_one_step holds float16 priorities to at B <= 32"""
    newp = P.new_priority(o.last_abs_delta, 0.6, 1e-6)
    pr = mem.priorities()
    last = {int(i): k for k, i in enumerate(idx)}
    rt = 3e-3 if kw.get("datatype") == "float16" else 1e-4
    np.testing.assert_allclose(np.array([pr[i] for i in last]), np.array([newp[k] for k in last.values()]), rtol=rt)


def _composed(sd, n, per, name="fp32_b32", dtype=None, seed=17):
    """three teacher-forced steps through train_from_memory on a 600-slot ring with terminals against the combined oracle fed the same
    indexes: Q(pre), the soft value, every gradient; PER: the priorities written back.  name: a configuration of CONFIGS that
    tests/test_gpu_nstep.py's CONFIGS (the ring's) holds too; dtype: _oracle's; seed: of the sampling"""
    A, B, geom, kw, tol, _ = _cfg(name)
    per_kw = _per_kw() if per else {}
    mem, om = _mems(sd, name, n, size=600, **dict(MU, **per_kw))
    ws, wt = xavier_weights(A, 71, _dt(kw), *geom), xavier_weights(A, 171, _dt(kw), *geom)
    net = _net(sd, name, ws, wt, n_step=n, **per_kw)
    net.set_option("keep_gradients", 1)
    cls = {(False, False): MO.MunchausenOracle, (True, False): MO.MunchausenOracleNStep,
           (False, True): MO.MunchausenOraclePER, (True, True): MO.MunchausenOraclePERNStep}[(n > 1, per)]
    o = _oracle(name, ws, wt, cls, dtype=dtype, n_step=n)
    random.seed(seed)
    seen_done = False
    for s in range(3):
        if o.dtype != net._np:                                   # (tests/test_gpu_advantage_learning.py::_force: both sides hold the same numbers)
            o.W = [np.asarray(w, net._np).astype(o.dtype) for w in o.W]
            o.S = [np.asarray(x, net._np).astype(o.dtype) for x in o.S]
        net.set_weights(o.W, 0)
        for i in range(5):
            net.set_layer(i, o.S[i], 2)
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
        _check_q(net, o, preq, tol)
        _check_grads(net, name, g)
        if per:
            _check_priorities(mem, idx, o, kw)
        o.optimize(g, B)
    assert seen_done


def test_composed_with_n_step(sd):
    _composed(sd, 3, False)


def test_composed_with_prioritized_replay(sd):
    _composed(sd, 1, True)


def test_composed_with_both(sd):
    _composed(sd, 3, True)


def test_option_off_is_the_parent_step(sd):
    """off: three steps bit-identical to a net built without the arguments, the same launches"""
    name = "fp32_b32"
    A, B, geom, kw, _, _ = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 80 + s) for s in range(3)]
    ws, wt = xavier_weights(A, 81, np.float32, *geom), xavier_weights(A, 181, np.float32, *geom)
    off = _net(sd, name, ws, wt, munchausen=False)
    plain = sd.DeepQNetwork(A, make_args(batch_size=B))
    assert plain.munchausen is False
    plain.set_weights(wt, 1); plain.set_weights(ws, 0)
    counts = []
    for net in (off, plain):
        counts.append(_counts(net, lambda: [net.train(mb) for mb in mbs], n=1))
    assert counts[0] == counts[1]
    for a, b in zip(_layers(off), _layers(plain)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_switching_between_steps(sd, name):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 90 + s) for s in range(3)]
    net, o = _setup(sd, name, 91, mbs[0])
    net.set_option("keep_gradients", 1)
    for s, on in enumerate((True, False, True)):
        net.set_munchausen(on); o.munchausen = on
        net.set_weights(o.W, 0)
        for i in range(5):
            net.set_layer(i, o.S[i], 2)
        g, _, _, preq = o.gradients(mbs[s])
        net.train(mbs[s])
        q, mq = net.last_q()
        assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
        ref = o.last_V if on else o.fprop(o.Wt, o._normalize(mbs[s][3])).max(1)
        assert np.abs(mq - ref).max() < 3 * max(tol, 1e-6) * max(1.0, float(np.abs(ref).max())), s
        _check_grads(net, name, g)
        o.optimize(g, B)


@pytest.mark.parametrize("kw,word", [(dict(double_dqn=True), "double_dqn"), (dict(batch_norm=True), "batch_norm"),
                                     (dict(double_dqn=True, datatype="float64", batch_size=8), "double_dqn")])
def test_library_refusals(sd, kw, word):
    net = sd.DeepQNetwork(4, make_args(**dict(dict(batch_size=32), **kw)))
    lib = sd.load()
    ERR_ARG = -1                                             # include/sdqn.h: SDQN_ERR_ARG
    rc = lib.sdqn_net_set_munchausen(net._h, 1, 0.9, 0.03, -1.0)
    assert rc == ERR_ARG and word in lib.sdqn_last_error().decode() and "munchausen" in lib.sdqn_last_error().decode()
    for bad in ((0.9, 0.0, -1.0), (1.5, 0.03, -1.0), (-0.1, 0.03, -1.0), (0.9, 0.03, 0.5), (0.9, float("nan"), -1.0)):
        assert lib.sdqn_net_set_munchausen(net._h, 0, *bad) == ERR_ARG, bad
    if "double_dqn" in kw:                                   # the other order: double_dqn on a Munchausen net
        net.set_option("double_dqn", 0)
        net.set_munchausen(True)
        with pytest.raises(Exception) as ei:
            net.set_option("double_dqn", 1)
        assert "munchausen" in str(ei.value)


@pytest.mark.parametrize("name", ["fp32_b32", "fp32_b128", "fp16_b32", "fp16_b128"])
def test_launches_per_step(sd, name):
    """a Munchausen step = the standard step's launches + the launches of one predict of that net; the backward is the standard one"""
    A, B, geom, kw, _, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 50)
    ws, wt = xavier_weights(A, 52, _dt(kw), *geom), xavier_weights(A, 152, _dt(kw), *geom)
    mu, std = _net(sd, name, ws, wt), _net(sd, name, ws, wt, munchausen=False)
    assert mu.step_structure() == std.step_structure()
    c_mu = _counts(mu, lambda: mu.train(mb))
    c_std = _counts(std, lambda: std.train(mb))
    c_fwd = _counts(std, lambda: std.predict(mb[0]))
    print(name, c_mu, c_std, c_fwd)
    assert sum(c_fwd.values()) > 0
    for k in set(c_mu) | set(c_std) | set(c_fwd):
        assert c_mu.get(k, 0) == c_std.get(k, 0) + c_fwd.get(k, 0), (k, c_mu, c_std, c_fwd)
    for k in c_std:                                          # ids no forward issues (the backward and the optimizer): unchanged
        if k not in c_fwd:
            assert c_mu[k] == c_std[k], k
    mu.set_munchausen(False)                                 # switched off between steps: the standard step again
    assert _counts(mu, lambda: mu.train(mb)) == c_std


def test_fused_loop_equals_tuple_api(sd):
    A, B, size = 4, 32, 5000
    args = make_args(batch_size=B, **MU)
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
    random.seed(9)
    st = random.getstate()
    n1.train_from_memory(mem, 4)
    random.setstate(st)
    for _ in range(4):
        n2.train(mem.getMinibatch())
    for a, b in zip(_layers(n1), _layers(n2)):
        assert np.array_equal(a, b)
    random.seed(6)                                           # and the option is honoured on the fused loop: a standard net moves elsewhere
    n3.train_from_memory(mem, 3)
    n3.train_from_memory(mem, 4)
    assert not np.array_equal(n1.get_layer(4), n3.get_layer(4))


def test_agent_fused_loop_equals_tuple_api(sd):
    """Agent(fused=True) trains through train_from_memory, Agent(fused=False) through net.train(mem.getMinibatch())"""
    res = []
    for fused in (True, False):
        args = make_args(batch_size=32, replay_size=2000, random_steps=0, train_frequency=4, train_repeat=1, target_steps=16,
                         exploration_decay_steps=100, **MU)
        random.seed(3)
        env = sd.SyntheticEnvironment(args, num_actions=4, seed=1)
        mem = sd.ReplayMemory(2000, args)
        net = sd.DeepQNetwork(4, args)
        net.set_weights(xavier_weights(4, 5), 0); net.update_target_network()
        agent = sd.Agent(env, mem, net, args, fused=fused)
        agent.play_random(200)
        agent.train(48, 0)
        res.append(_layers(net))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_main_loop(sd, tmp_path):
    from simple_dqn_amd import main as M
    csv = tmp_path / "mu.csv"
    args = M.build_parser().parse_args(
        ["--replay_size", "3000", "--random_steps", "300", "--train_steps", "200", "--test_steps", "40", "--epochs", "2",
         "--exploration_decay_steps", "200", "--target_steps", "64", "--random_seed", "7", "--munchausen", "true", "--csv_file", str(csv)])
    stats = M.run(args)
    assert stats.net.munchausen is True and stats.net.train_iterations == 2 * 200 // 4
    assert csv.read_text().count("\n") >= 2
