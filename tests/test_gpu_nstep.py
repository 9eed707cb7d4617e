"""--n_step on the GPU against the numpy restatement (tests/nstep_oracle.py): the tuple gather, one step and ten steps in every
datatype / regime, composition with --double_dqn and --prioritized_replay, launch counts, n = 1 identity, the tuple API's upload
skipping, refusals and the command line.  The steps read the poststate n frames after the prestate and bootstrap with gamma^n: a library
that ignored the option would train on different targets and fail the parity checks."""
import ctypes as C
import random

import numpy as np
import pytest

import nstep_oracle as N
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill
from util import make_args

pytestmark = pytest.mark.gpu

GAMMA, MINR, MAXR = 0.99, -1.0, 1.0
# name: (A, B, screen (hist, H, W), make_args keywords, Q tolerance, 10-step Q tolerance) — the bounds of tests/test_gpu_double_dqn.py
CONFIGS = {
    "fp32_b32": (4, 32, (4, 84, 84), {}, 1e-4, 1e-4),
    "fp32_b256": (4, 256, (4, 84, 84), {}, 1e-4, 2e-3),
    "fp16_b32": (4, 32, (4, 84, 84), dict(datatype="float16"), 3e-3, 2e-1),
    "fp16_b256": (4, 256, (4, 84, 84), dict(datatype="float16"), 3e-3, 2e-1),
    "bn_b32": (4, 32, (4, 84, 84), dict(batch_norm=True), 1e-4, 2e-2),
    "f64_b8": (6, 8, (4, 84, 84), dict(datatype="float64"), 1e-9, 1e-9),
    "f32_96": (4, 8, (4, 96, 96), {}, 1e-5, 1e-4),
}


def _cfg(name):
    """a key of CONFIGS, or a configuration of its form itself (tests/test_gpu_option_head_edges.py passes its own)"""
    return CONFIGS[name] if isinstance(name, str) else name


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _dt(kw):
    return np.float64 if kw.get("datatype") == "float64" else np.float32


def _args(name, n, **extra):
    A, B, (hist, H, W), kw, _, _ = _cfg(name)
    return make_args(batch_size=B, history_length=hist, screen_height=H, screen_width=W, n_step=n, **kw, **extra)


def _mems(sd, name, n, size=600, seed=3, p_term=0.05, **extra):
    """a product memory and an oracle ring with the same content: full, wrapped (current inside), terminals every ~20 slots"""
    A, B, (hist, H, W), kw, _, _ = _cfg(name)
    mem = sd.ReplayMemory(size, _args(name, n, **extra))
    om = ReplayOracle(size, H, W, hist, B)
    for m in (mem, om):
        synthetic_fill(m, seed, num_actions=A)
        rng = np.random.RandomState(seed + 1)
        m.terminals[:] = rng.rand(size) < p_term
        m.rewards[:] = rng.randint(-3, 4, size)                  # outside the clip range too
    mem.sync_mirror()
    return mem, om


def _net(sd, name, n, ws, wt, **extra):
    net = sd.DeepQNetwork(_cfg(name)[0], _args(name, n, **extra))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    return net


def _oracle(name, n, ws, wt, cls=None):
    A, B, (hist, H, W), kw, _, _ = _cfg(name)
    if cls is None:
        cls = N.NStepOracleBN if kw.get("batch_norm") else N.NStepOracle
    o = cls(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=_dt(kw), weights=ws,
            half_activations=kw.get("datatype") == "float16")
    o.Wt = [w.copy() for w in wt]
    o.n_step = n
    return o


def _weights(name, s):
    A, _, geom, kw, _, _ = _cfg(name)
    return xavier_weights(A, s, _dt(kw), *geom), xavier_weights(A, s + 100, _dt(kw), *geom)


def _sample(mem, n, seed):
    random.seed(seed)
    return np.array(mem.sample_indexes(), dtype=np.int64)


def _check_grads(net, name, g):
    kw = _cfg(name)[3]
    for i in range(5):
        gg = np.asarray(net.get_layer(i, 3), np.float64)
        ref = np.asarray(g[i], np.float64)
        if kw.get("datatype") == "float64":
            assert np.linalg.norm(gg - ref) / max(np.linalg.norm(ref), 1e-300) < 1e-11, i
        elif kw.get("datatype") == "float16":
            assert np.linalg.norm(gg - ref) / max(1e-12, np.linalg.norm(ref)) < 5e-2, i
        elif _cfg(name)[1] >= 128:
            # float32 B = 256: a Rectlin gate of the throughput routines that lands on the other side of zero moves single elements of
            # the conv gradients far past the element bound, in the standard step as well (tests/test_gpu_double_dqn.py,
            # test_ten_teacher_forced_steps): held to a relative norm instead (conv1 measured 4.7e-3 here; a wrong frame would be O(1))
            print("%s layer %d: grad max abs err %.3e, rel norm %.3e" % (name, i, np.abs(gg - ref).max(),
                                                                        np.linalg.norm(gg - ref) / np.linalg.norm(ref)))
            assert np.linalg.norm(gg - ref) / max(1e-12, np.linalg.norm(ref)) < 1e-2, i
        else:
            bound = 5e-4 if kw.get("batch_norm") else 1e-4
            assert np.abs(gg - ref).max() < bound * max(1e-3, np.abs(ref).max()), i


def _check_q(net, o, preq, tol):
    q, mq = net.last_q()
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    ref = o.fprop(o.Wt, o._normalize(o._last_post)).max(1)
    assert np.abs(mq - ref).max() < max(tol, 1e-6) * max(1.0, float(np.abs(ref).max()))


def _grads(o, mb):
    o._last_post = mb[3]
    return o.gradients(mb)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_tuple_gather_equals_oracle(sd, n):
    mem, om = _mems(sd, "fp32_b32", n, p_term=0.1)
    assert mem.count == mem.size and 0 < mem.current < mem.size
    idx = _sample(mem, n, 11)
    o_idx, _ = N.sample_indexes(_mt_from_seed(11), om.terminals, om.count, om.current, om.history_length, n, 32)
    assert np.array_equal(idx, o_idx)
    pre, act, R, post, done = mem.gather(idx)
    opre, oact, oR, opost, odone = N.gather(om, idx, n, GAMMA, MINR, MAXR)
    assert np.array_equal(np.asarray(pre), opre) and np.array_equal(np.asarray(post), opost)
    assert np.array_equal(act, oact) and np.array_equal(done, odone)
    assert R.dtype == np.float64 and np.array_equal(R.view(np.int64), oR.view(np.int64))
    assert done.any() and (np.abs(oR) > 1).any()                 # the minibatch exercises truncation and multi-step sums
    # the device copy the gather left: (R, done) bits in the reward / terminal staging
    mb_r = mem._mb_rewards.view(np.float64)
    mem._materialize()
    assert np.array_equal(mb_r.view(np.int64), oR.view(np.int64)) and np.array_equal(mem._mb_terminals, odone)


def _mt_from_seed(seed):
    from oracle.replay_numpy import MT19937
    return MT19937(seed)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_step_parity(sd, name):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    n = 3
    mem, om = _mems(sd, name, n, size=max(600, 3 * B))
    ws, wt = _weights(name, 11)
    net = _net(sd, name, n, ws, wt)
    net.set_option("keep_gradients", 1)
    o = _oracle(name, n, ws, wt)
    idx = _sample(mem, n, 5)
    mb = N.gather(om, idx, n, GAMMA, MINR, MAXR)
    g, _, _, preq = _grads(o, mb)
    net.train_indexes(mem, idx)
    _check_q(net, o, preq, tol)
    _check_grads(net, name, g)
    # the tuple path of the same step
    net2 = _net(sd, name, n, ws, wt)
    net2.set_option("keep_gradients", 1)
    net2.train(mem.gather(idx))
    _check_q(net2, o, preq, tol)
    _check_grads(net2, name, g)


@pytest.mark.parametrize("name", ["fp32_b32", "fp16_b32", "f64_b8"])
def test_ten_free_running_steps_with_target_sync(sd, name):
    A, B, geom, kw, tol, tol10 = CONFIGS[name]
    n = 3
    mem, om = _mems(sd, name, n)
    ws, wt = _weights(name, 21)
    net, o = _net(sd, name, n, ws, wt), _oracle(name, n, ws, wt)
    for s in range(10):
        if s == 5:
            net.update_target_network(); o.update_target_network()
        idx = _sample(mem, n, 100 + s)
        net.train_indexes(mem, idx)
        o.train(N.gather(om, idx, n, GAMMA, MINR, MAXR))
    hold = N.gather(om, _sample(mem, n, 99), n, GAMMA, MINR, MAXR)[0]
    err = np.abs(net.predict(hold) - o.predict(hold)).max()
    print("%s: Q max abs err after 10 steps %.3e" % (name, err))
    assert err < tol10 * max(1.0, float(np.abs(o.predict(hold)).max()))


def _layers(net):
    return [np.asarray(net.get_layer(i)).tobytes() for i in range(5)]


def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("name", ["fp32_b32", "fp16_b256", "f64_b8"])
def test_n1_bit_identical_to_standard(sd, name):
    mem, _ = _mems(sd, name, 1)
    ws, wt = _weights(name, 31)
    a = _net(sd, name, 1, ws, wt)
    b = _net(sd, name, 1, ws, wt)
    b.set_option("n_step", 1)
    random.seed(4); a.train_from_memory(mem, 10)
    random.seed(4); b.train_from_memory(mem, 10)
    assert _layers(a) == _layers(b)
    if name != "f64_b8":
        random.seed(5); ca = _counts(a, lambda: a.train_from_memory(mem, 1))
        random.seed(5); cb = _counts(b, lambda: b.train_from_memory(mem, 1))
        assert ca == cb


@pytest.mark.parametrize("name", ["fp32_b32", "fp32_b256", "fp16_b32", "fp16_b256", "bn_b32"])
@pytest.mark.parametrize("double", [False, True])
def test_launches_per_step(sd, name, double):
    ws, wt = _weights(name, 51)
    m1, _ = _mems(sd, name, 1)
    m3, _ = _mems(sd, name, 3)
    std, ns = _net(sd, name, 1, ws, wt, double_dqn=double), _net(sd, name, 3, ws, wt, double_dqn=double)
    assert std.step_structure() == ns.step_structure()
    random.seed(1); c_std = _counts(std, lambda: std.train_from_memory(m1, 2))
    random.seed(1); c_ns = _counts(ns, lambda: ns.train_from_memory(m3, 2))
    assert c_std == c_ns
    i1, i3 = _sample(m1, 1, 2), _sample(m3, 3, 2)
    assert _counts(std, lambda: std.train_indexes(m1, i1)) == _counts(ns, lambda: ns.train_indexes(m3, i3))


def _per_kw():
    return dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6)


def test_launches_per_step_prioritized(sd):
    ws, wt = _weights("fp32_b32", 52)
    m1, _ = _mems(sd, "fp32_b32", 1, **_per_kw())
    m3, _ = _mems(sd, "fp32_b32", 3, **_per_kw())
    std, ns = _net(sd, "fp32_b32", 1, ws, wt), _net(sd, "fp32_b32", 3, ws, wt)
    random.seed(1); c_std = _counts(std, lambda: std.train_from_memory(m1, 2))
    random.seed(1); c_ns = _counts(ns, lambda: ns.train_from_memory(m3, 2))
    assert c_std == c_ns


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_double_dqn_composed(sd, name):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    n = 3
    mem, om = _mems(sd, name, n)
    ws, wt = _weights(name, 61)
    net = _net(sd, name, n, ws, wt, double_dqn=True)
    net.set_option("keep_gradients", 1)
    o = _oracle(name, n, ws, wt, N.NStepOracleDDQN)
    idx = _sample(mem, n, 6)
    mb = N.gather(om, idx, n, GAMMA, MINR, MAXR)
    g, _, _, preq = o.gradients(mb)
    net.train_indexes(mem, idx)
    q, mq = net.last_q()
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    scale = max(1.0, float(np.abs(o.last_maxpostq).max()))
    near = np.sort(o.last_online_postq, axis=1)
    clear = (near[:, -1] - near[:, -2]) > 10 * max(tol, 1e-6)
    assert (np.abs(mq - o.last_maxpostq)[clear] <= max(tol, 1e-6) * scale).all()
    if clear.all():
        _check_grads(net, name, g)


def test_prioritized_composed_and_validity(sd):
    name, n = "fp32_b32", 3
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mem, om = _mems(sd, name, n, size=400, **_per_kw())
    hist = om.history_length
    # every priority starts at 1: the leaves are the n-step validity mask
    mask = N.valid_mask(om.terminals, om.count, om.current, hist, om.size, n)
    assert np.array_equal(mem.priorities() > 0, mask)
    assert not np.array_equal(mask, N.valid_mask(om.terminals, om.count, om.current, hist, om.size, 1))
    ws, wt = _weights(name, 71)
    net = _net(sd, name, n, ws, wt, **_per_kw())
    net.set_option("keep_gradients", 1)
    o = _oracle(name, n, ws, wt, N.NStepOraclePER)
    random.seed(8)
    mb = mem.getMinibatch()
    idx, w = mem.last_sample()
    assert mask[idx].all()
    o.weights = w
    g, _, _, preq = o.gradients(N.gather(om, idx, n, GAMMA, MINR, MAXR))
    net.train(mb)
    q, _ = net.last_q()
    assert np.abs(q - preq).max() < max(tol, 1e-6) * max(1.0, float(np.abs(preq).max()))
    _check_grads(net, name, g)
    # adds that move `current` across sampled windows: validity follows, including the n - 1 slots in front of each write
    scr = np.zeros(geom[1:], np.uint8)
    for k in range(7):
        t = k == 3
        mem.add(1, 1, scr, t)
        om.add(1, 1, scr, t)
        pr = mem.priorities()
        m = N.valid_mask(om.terminals, om.count, om.current, hist, om.size, n)
        assert np.array_equal(pr > 0, m), k


def test_fused_agent_equals_tuple_api(sd):
    name, n = "fp32_b32", 3
    mem, _ = _mems(sd, name, n, size=3000)
    ws, wt = _weights(name, 81)
    n1, n2 = _net(sd, name, n, ws, wt), _net(sd, name, n, ws, wt)
    random.seed(6)
    for _ in range(3):
        st = random.getstate()
        n1.train(mem.getMinibatch())
        random.setstate(st)
        n2.train_from_memory(mem, 1)
    for i in range(5):
        assert np.array_equal(n1.get_layer(i), n2.get_layer(i)), i
    # a standard net on a standard memory moves elsewhere
    m1, _ = _mems(sd, name, 1, size=3000)
    n3 = _net(sd, name, 1, ws, wt)
    random.seed(6)
    n3.train_from_memory(m1, 3)
    assert not np.array_equal(n1.get_layer(4), n3.get_layer(4))


def test_unedited_tuple_uploads_nothing_edited_returns_used(sd):
    name, n = "fp32_b32", 3
    mem, _ = _mems(sd, name, n)
    ws, wt = _weights(name, 91)
    a = _net(sd, name, n, ws, wt)
    random.seed(3)
    a.train(mem.getMinibatch())
    assert a.tuple_counters()[2] == 1                     # (R, done) of the gather equal what the device holds: nothing uploaded
    random.seed(3)
    pre, act, R, post, done = mem.getMinibatch()
    R2 = R + 0.5                                          # an edited returns array: uploaded and used
    b = _net(sd, name, n, ws, wt)
    b.train((pre, act, R2, post, done))
    assert b.tuple_counters()[2] == 0
    assert not np.array_equal(b.get_layer(4), a.get_layer(4))
    c = _net(sd, name, n, ws, wt)
    c.train((np.asarray(pre).copy(), act, R2, np.asarray(post).copy(), done))
    for i in range(5):
        assert np.array_equal(b.get_layer(i), c.get_layer(i)), i


def test_refusals(sd):
    from simple_dqn_amd import _lib
    name = "fp32_b32"
    for bad in (0, 17):
        with pytest.raises(Exception):
            sd.ReplayMemory(600, _args(name, bad))
        with pytest.raises(Exception):
            sd.DeepQNetwork(4, _args(name, bad))
    ws, wt = _weights(name, 5)
    m3, _ = _mems(sd, name, 3)
    m2, _ = _mems(sd, name, 2)
    net = _net(sd, name, 3, ws, wt)
    with pytest.raises(Exception, match="n_step 2 != network n_step 3"):
        net.train_from_memory(m2, 1)
    with pytest.raises(Exception, match="n_step"):
        net.train_indexes(m2, _sample(m2, 2, 1))
    md = sd.ReplayMemory(600, _args(name, 3, discount_rate=0.9))
    synthetic_fill(md, 3); md.sync_mirror()
    with pytest.raises(Exception, match="discount"):
        net.train_from_memory(md, 1)
    # integer rewards in n-step mode
    pre, act, R, post, done = m3.gather(_sample(m3, 3, 2))
    with pytest.raises(ValueError):
        net.train((pre, act, np.zeros(32, np.int64), post, done))
    # count < hist + n
    small = sd.ReplayMemory(600, _args(name, 3))
    scr = np.zeros((84, 84), np.uint8)
    for _ in range(6):
        small.add(0, 0, scr, False)
    with pytest.raises(Exception):
        small.sample_indexes()
    small.add(0, 0, scr, False)
    assert (np.asarray(small.sample_indexes()) == 4).all()
    # the library's own check of the mismatch, through the C ABI
    cost = C.c_float()
    assert net._lib.sdqn_net_train_many(net._h, m2._h, (C.c_uint32 * _lib.MT_WORDS)(), 1, C.byref(cost)) == -1


def test_main_loop(sd, tmp_path):
    from simple_dqn_amd import main as M
    csv = str(tmp_path / "nstep.csv")
    args = M.build_parser().parse_args(
        ["--replay_size", "3000", "--random_steps", "300", "--train_steps", "200", "--test_steps", "40", "--epochs", "1",
         "--exploration_decay_steps", "200", "--target_steps", "64", "--random_seed", "7", "--n_step", "3", "--csv_file", csv])
    stats = M.run(args)
    assert stats.net.n_step == 3 and stats.mem.n_step == 3
    assert stats.net.train_iterations == 200 // 4
    assert open(csv).read().count("\n") >= 2
