"""--prioritized_replay on the GPU against the numpy restatement (tests/per_oracle.py).

Every test here fails on a library that samples uniformly or ignores the weights: the sampled indexes are compared exactly with the
oracle's stratified draw, the priority fixtures spread the importance weights (min w < 0.5), and the gradients are compared with the
weighted oracle."""
import random

import numpy as np
import pytest

import per_oracle as P
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill
from test_gpu_double_dqn import CONFIGS, _check_grads
from util import make_args

pytestmark = pytest.mark.gpu

ALPHA, EPS = 0.6, 1e-6


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _mem(sd, size, B, seed=3, count=None, current=None, A=4, **kw):
    args = make_args(batch_size=B, prioritized_replay=True, priority_alpha=ALPHA, priority_beta=0.4,
                     priority_beta_steps=1000, priority_epsilon=EPS, **kw)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, seed, num_actions=A, count=count, current=current)
    mem.terminals[np.arange(7, size, 97)] = True          # scattered terminals
    mem.sync_mirror()
    return mem


def _mask(mem):
    return P.valid_mask(np.asarray(mem.terminals), mem.count, mem.current, mem.history_length, mem.size)


def _words():
    import ctypes as C
    from simple_dqn_amd import _lib
    w = C.c_uint64()
    _lib.load().sdqn_mt_words(C.byref(w))
    return w.value


@pytest.mark.parametrize("size", [600, 300000])
def test_exact_sampling(sd, size):
    B = 32
    mem = _mem(sd, size, B, current=size // 2 + 11)
    rng = np.random.RandomState(size)
    raw = rng.randint(1, 50, size).astype(np.float32)     # integers: exact in fp32 and fp64
    mem.set_priorities(0, raw)
    mask = _mask(mem)
    leaf = np.where(mask, raw, 0).astype(np.float32)
    assert np.array_equal(mem.priorities(), leaf)
    random.seed(7)
    for call in range(50):
        st = random.getstate()
        w0 = _words()
        idx = mem.sample_indexes().copy()
        assert _words() - w0 == 2 * B
        r = random.Random(); r.setstate(st)
        u = P.uniforms(r, B)
        assert random.getstate() == r.getstate()          # Python's stream in step
        ref = P.sample(leaf, u)
        assert np.array_equal(idx, ref), call
        assert all(P.accepts(int(i), np.asarray(mem.terminals), mem.count, mem.current, 4) for i in idx)
        _, w = mem.last_sample()
        np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)


def test_distribution_chi_square(sd):
    B, size = 32, 600
    mem = _mem(sd, size, B)
    mask = _mask(mem)
    raw = np.ones(size, np.float32)
    hot = int(np.nonzero(mask)[0][10])
    raw[hot] = 1000.0
    mem.set_priorities(0, raw)
    leaf = np.where(mask, raw, 0).astype(np.float64)
    random.seed(11)
    counts = np.zeros(size)
    for _ in range(10000):
        np.add.at(counts, mem.sample_indexes(), 1)
    assert counts[~mask].sum() == 0
    p = leaf / leaf.sum()
    exp = p * counts.sum()
    v = mask
    chi2 = (((counts[v] - exp[v]) ** 2) / exp[v]).sum()
    dof = v.sum() - 1
    # stratification makes the draw less dispersed than multinomial: the statistic sits below its dof; uniform sampling is far above
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)
    assert abs(counts[hot] / counts.sum() - p[hot]) < 0.01


def test_validity_maintenance(sd):
    B, size = 8, 200
    mem = _mem(sd, size, B, count=150, current=150)
    mem.set_priorities(0, np.full(size, 2.0, np.float32))
    mem.set_priorities(20, np.float32([5.0]))
    assert mem.max_priority == 5.0
    scr = np.zeros((84, 84), np.uint8)
    for k in range(60):                                   # across a terminal and the ring's wrap
        mem.add(k % 4, 0, scr, k == 10)
    pr = mem.priorities()
    mask = _mask(mem)
    assert np.array_equal(pr == 0, ~mask)
    new = [(150 + k) % size for k in range(60)]
    assert (pr[[i for i in new if mask[i]]] == 5.0).all()
    t = (150 + 10) % size
    assert (pr[t + 1:t + 5] == 0).all()                   # the history window after the terminal
    cur = mem.current
    assert (pr[cur:cur + 4] == 0).all()
    # a write through a tracked view: the slots get p_max, the following hist slots are re-evaluated
    s = next(k for k in range(20, 140) if mask[k:k + 5].all())
    mem.terminals[s] = True
    pr2 = mem.priorities()
    assert pr2[s] == 5.0 and (pr2[s + 1:s + 5] == 0).all()
    mem.terminals[s] = False
    pr3 = mem.priorities()
    assert pr3[s] == 5.0 and (pr3[s + 1:s + 5] == pr[s + 1:s + 5]).all() and (pr3[s + 1:s + 5] > 0).all()


STEP_CONFIGS = list(CONFIGS) + ["fp32_b32_ddqn"]


def _step_setup(sd, name, size=3000, seed=3):
    base = "fp32_b32" if name == "fp32_b32_ddqn" else name
    A, B, geom, kw, tol, _ = CONFIGS[base]
    hist, H, W = geom
    ddqn = name.endswith("ddqn")
    gk = dict(history_length=hist, screen_height=H, screen_width=W)
    mem = _mem(sd, size, B, seed=seed, A=A, **gk, **kw)
    rng = np.random.RandomState(seed)
    mem.set_priorities(0, (10.0 ** rng.uniform(-2, 1, size)).astype(np.float32))
    omem = ReplayOracle(size, screen_height=H, screen_width=W, history_length=hist, batch_size=B)
    synthetic_fill(omem, seed, num_actions=A, current=None)
    omem.terminals[np.arange(7, size, 97)] = True
    dt = np.float64 if kw.get("datatype") == "float64" else np.float32
    ws = xavier_weights(A, 11, dt, *geom)
    wt = xavier_weights(A, 12, dt, *geom) if ddqn else ws
    net = sd.DeepQNetwork(A, make_args(batch_size=B, double_dqn=ddqn, **gk, **kw))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    if not ddqn:
        net.update_target_network()
    cls = P.PEROracleBN if kw.get("batch_norm") else (P.PEROracleDDQN if ddqn else P.PEROracle)
    o = cls(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=dt, weights=ws,
            half_activations=kw.get("datatype") == "float16")
    o.Wt = [w.copy() for w in wt]
    return mem, omem, net, o, base


def _check_update(net, o, g, B, kw):
    """the updated online weights against the oracle's optimizer on its gradients.  RMSProp from a zero state moves every weight by about
    lr / sqrt(1 - rho) whatever the gradient's size, so a gradient within round-off of zero may move either way: at most 1 % of a layer
    may leave the close bound, and none by more than twice the largest step"""
    w0 = [np.array(w, np.float64) for w in o.W]
    o.optimize(g, B)
    for i in range(5):
        ref = np.asarray(o.W[i], np.float64)
        got = np.asarray(net.get_layer(i, 0), np.float64).reshape(ref.shape)
        step = np.abs(ref - w0[i]).max()
        diff = np.abs(got - ref)
        close = 1e-9 if kw.get("datatype") == "float64" else (1e-2 if kw.get("datatype") == "float16" else 1e-3) * step + 1e-7
        assert (diff <= close).mean() > 0.99, (i, (diff <= close).mean())
        assert diff.max() <= 2.5 * step, i


@pytest.mark.parametrize("name", STEP_CONFIGS)
def test_one_step(sd, name):
    mem, omem, net, o, base = _step_setup(sd, name)
    A, B, geom, kw, tol, _ = CONFIGS[base]
    net.set_option("keep_gradients", 1)
    leaf = mem.priorities()
    pm0 = mem.max_priority
    random.seed(21)
    st = random.getstate()
    net.train_from_memory(mem, 1)
    idx, w = mem.last_sample()
    r = random.Random(); r.setstate(st)
    ref = P.sample(leaf, P.uniforms(r, B))
    assert np.array_equal(idx, ref)
    np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)
    assert w.min() < 0.5
    o.weights = w
    g, cost, _, preq = o.gradients(omem.gather(idx))
    q, _ = net.last_q()
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    _check_grads(net, base, g)
    _check_update(net, o, g, B, kw)
    newp = P.new_priority(o.last_abs_delta, ALPHA, EPS)
    pr = mem.priorities()
    last = {int(i): k for k, i in enumerate(idx)}
    rt = 3e-3 if kw.get("datatype") == "float16" else 1e-5
    got = np.array([pr[i] for i in last]); exp = np.array([newp[k] for k in last.values()])
    assert abs(mem.max_priority - max(pm0, float(exp.max()))) <= 1e-3 * mem.max_priority
    if B <= 32:
        np.testing.assert_allclose(got, exp, rtol=rt)
    else:
        # |delta| back out of the priority, held to the step's Q bound (B = 256: the throughput routines' Q carries 1e-4 of max |Q|, a
        # large relative error of a small |delta|)
        absd = np.array([o.last_abs_delta[k] for k in last.values()], np.float64)
        assert np.abs((got.astype(np.float64) ** (1 / ALPHA) - EPS) - absd).max() < 2 * max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))


@pytest.mark.parametrize("name", ["fp32_b32", "f32_generic"])
def test_add_between_sample_and_train(sd, name):
    """getMinibatch(); add(...); train(mb): the slots written in between end at p_max after the step's write-back, and every leaf
    follows the reference's acceptance rule"""
    mem, _, net, _, base = _step_setup(sd, name, size=600)
    hist, H, W = CONFIGS[base][2]
    random.seed(4)
    mb = mem.getMinibatch()
    cur = mem.current
    scr = np.zeros((H, W), np.uint8)
    mem.add(1, 0, scr, True)                                # a terminal: the following hist slots turn invalid
    for _ in range(3):
        mem.add(2, 0, scr, False)
    pm = mem.max_priority
    net.train(mb)
    pr = mem.priorities()
    mask = _mask(mem)
    assert np.array_equal(pr == 0, ~mask)
    written = [(cur + k) % mem.size for k in range(4)]
    assert not mask[written[1:1 + min(hist, 3)]].any()      # inside the terminal's history window
    assert mem.max_priority >= pm
    assert (pr[[i for i in written if mask[i]]] == mem.max_priority).all()


def test_ten_teacher_forced_steps_across_target_sync(sd):
    mem, omem, net, o, base = _step_setup(sd, "fp32_b32")
    A, B, geom, kw, tol, _ = CONFIGS[base]
    raw = mem.priorities().copy()
    valid = _mask(mem)
    random.seed(31)
    for s in range(10):
        if s == 5:
            net.update_target_network(); o.update_target_network()
        leaf = np.where(valid, raw, 0).astype(np.float32)
        st = random.getstate()
        net.train_from_memory(mem, 1)
        idx, w = mem.last_sample()
        r = random.Random(); r.setstate(st)
        assert np.array_equal(idx, P.sample(leaf, P.uniforms(r, B))), s
        np.testing.assert_allclose(w, P.weights(leaf[idx], 0.4), rtol=1e-6)
        o.weights = w
        g, _, _, preq = o.gradients(omem.gather(idx))
        newp = P.new_priority(o.last_abs_delta, ALPHA, EPS)
        pr = mem.priorities()
        for k, i in {int(i): k for k, i in enumerate(idx)}.items():
            assert abs(pr[k] - newp[i]) <= 1e-4 * newp[i], (s, k)
        raw = np.where(valid, pr, raw)
        raw[idx] = pr[idx]
        o.W = [np.array(x, dtype=np.float32).reshape(y.shape) for x, y in zip(net.get_weights(0), o.W)]   # teacher forcing
        q, _ = net.last_q()
        assert np.abs(q - preq).max() < 1e-4 * max(1.0, float(np.abs(preq).max()))


def _counts(net, fn):
    net.profile(True, -1); net.profile_reset()
    fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("name", ["fp32_b32", "fp32_b256", "fp16_b32", "fp16_b256", "bn_b32"])
def test_launch_counts(sd, name):
    """one added launch per PER step in every tuned regime (the per_step launch under the prep slot)"""
    mem, _, net, _, base = _step_setup(sd, name, size=2000)
    A, B, geom, kw, _, _ = CONFIGS[base]
    args = make_args(batch_size=B, **kw)
    smem = sd.ReplayMemory(2000, args)
    synthetic_fill(smem, 3, num_actions=A)
    smem.sync_mirror()
    std = sd.DeepQNetwork(A, args)
    n = 3
    random.seed(1)
    c_std = _counts(std, lambda: std.train_from_memory(smem, n))
    random.seed(1)
    c_per = _counts(net, lambda: net.train_from_memory(mem, n))
    key = "prep(idx+meta)"
    assert c_per[key] == c_std[key] + n
    assert {k: v for k, v in c_per.items() if k != key} == {k: v for k, v in c_std.items() if k != key}


def test_option_off_is_the_standard_net(sd):
    """prioritized_replay false (with non-default priority arguments) against args that never name the option: the same weights, the same
    launches, and the standard loop's launch structure (one prep per train_from_memory / train_indexes call, none for train(mb))"""
    A, B = 4, 32
    ws = xavier_weights(A, 4)
    res = []
    for per_args in (None, dict(prioritized_replay=False, priority_alpha=0.9, priority_beta=0.1, priority_beta_steps=5,
                                priority_epsilon=0.5)):
        a = make_args(batch_size=B, **(per_args or {}))
        m = sd.ReplayMemory(2000, a); synthetic_fill(m, 3, num_actions=A); m.sync_mirror()
        n = sd.DeepQNetwork(A, a); n.set_weights(ws, 0); n.update_target_network()
        random.seed(2)

        def run():
            n.train_from_memory(m, 3)
            n.train(m.getMinibatch())
            n.train_indexes(m, np.arange(100, 100 + B, dtype=np.int64))
            n.train_from_memory(m, 2)
            n.sync()
        res.append((n, m, _counts(n, run)))
    (n0, m0, c0), (n1, m1, c1) = res
    assert not m1.prioritized and not hasattr(m0, "_priority_args")
    assert c0 == c1
    assert c0["prep(idx+meta)"] == 3
    for i in range(5):
        assert np.array_equal(n0.get_layer(i), n1.get_layer(i)), i


def test_alpha0_beta0_equals_standard_step_bytes(sd):
    A, B = 4, 32
    ws = xavier_weights(A, 4)
    idx = np.arange(100, 100 + 4 * B, 4, dtype=np.int64)
    out = []
    for per in (False, True):
        a = make_args(batch_size=B, prioritized_replay=per, priority_alpha=0.0, priority_beta=0.0, priority_beta_steps=1,
                      priority_epsilon=1e-6)
        m = sd.ReplayMemory(2000, a); synthetic_fill(m, 3, num_actions=A, current=1900); m.sync_mirror()
        if per:
            m.set_priority_beta(0.0)
        n = sd.DeepQNetwork(A, a); n.set_weights(ws, 0); n.update_target_network()
        n.train_indexes(m, idx)
        out.append(n)
        if per:
            assert (m.priorities()[idx] == 1.0).all()
    for i in range(5):
        assert np.array_equal(out[0].get_layer(i), out[1].get_layer(i)), i


def test_fused_and_unfused_agents_agree(sd):
    """Agent(fused=True) trains through train_from_memory, Agent(fused=False) through net.train(mem.getMinibatch()); both anneal beta.
    Same seed: the same weights and priorities after 20 learns"""
    from simple_dqn_amd import Agent, SyntheticEnvironment
    A, B = 4, 32
    ws = xavier_weights(A, 8)
    res = []
    for fused in (True, False):
        args = make_args(batch_size=B, prioritized_replay=True, priority_alpha=ALPHA, priority_beta=0.4, priority_beta_steps=60,
                         priority_epsilon=EPS, exploration_decay_steps=100)
        random.seed(41)
        env = SyntheticEnvironment(args, num_actions=A, seed=41)
        mem = sd.ReplayMemory(3000, args)
        net = sd.DeepQNetwork(A, args)
        net.set_weights(ws, 0); net.update_target_network()
        agent = Agent(env, mem, net, args, fused=fused)
        assert agent.fused == fused
        agent.play_random(200)
        agent.train(80)
        assert net.train_iterations == 20
        res.append((net, mem.priorities(), mem.last_sample()))
    for i in range(5):
        assert np.array_equal(res[0][0].get_layer(i), res[1][0].get_layer(i)), i
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2][0], res[1][2][0]) and np.array_equal(res[0][2][1], res[1][2][1])
    pr = res[0][1][res[0][1] > 0]
    assert len(set(pr.tolist())) > 10


def test_refusals(sd):
    from simple_dqn_amd import _lib
    A, B = 4, 32
    lib = _lib.load()
    zc = sd.ReplayMemory(500, make_args(batch_size=B), flags=2)
    assert lib.sdqn_replay_enable_priorities(zc._h, 0.6, 1e-6) == -1
    mem = _mem(sd, 500, B)
    assert lib.sdqn_replay_enable_priorities(mem._h, -0.1, 1e-6) == -1
    assert lib.sdqn_replay_enable_priorities(mem._h, 0.6, 0.0) == -1
    assert lib.sdqn_replay_set_priority_beta(mem._h, 1.5) == -1
    assert lib.sdqn_replay_set_priority_beta(mem._h, -0.1) == -1
    with pytest.raises(AssertionError):
        mem.set_priorities(0, [np.inf])
    with pytest.raises(AssertionError):
        mem.set_priorities(0, [0.0])
    # a non-finite TD error is refused (reported by the next synchronising call), the tree keeps its priorities
    net = sd.DeepQNetwork(A, make_args(batch_size=B))
    ws = xavier_weights(A, 4)
    ws[4][:] = np.nan
    net.set_weights(ws, 0); net.update_target_network()
    before = mem.priorities()
    random.seed(3)
    with pytest.raises(AssertionError):
        net.train_from_memory(mem, 1, want_cost=True)
    assert np.array_equal(mem.priorities(), before)


def test_main_loop(sd, tmp_path):
    from simple_dqn_amd import main as M
    csv = str(tmp_path / "per.csv")
    args = M.build_parser().parse_args(
        ["--replay_size", "3000", "--random_steps", "300", "--train_steps", "200", "--test_steps", "40", "--epochs", "1",
         "--exploration_decay_steps", "200", "--target_steps", "64", "--random_seed", "7", "--prioritized_replay", "true",
         "--csv_file", csv])
    stats = M.run(args)
    assert stats.net.train_iterations == 200 // 4
    pr = stats.mem.priorities()
    assert len(set(pr[pr > 0].tolist())) > 10
    assert open(csv).read().count("\n") >= 2
