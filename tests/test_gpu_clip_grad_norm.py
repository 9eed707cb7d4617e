"""--clip_grad_norm on the GPU: the clipped step bit for bit against the explicit route (grad_only step, host-side scale,
apply_update), the reported norm against the gradient it was taken from, the edges of the reduction, determinism, free-running steps
against the fp64 oracle (tests/clip_oracle.py), launch counts, arguments and the main loop."""
import math
import random

import numpy as np
import pytest

from clip_oracle import ClipOracle, clip_scale, grad_norm
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu
A = 3
RING = 600
UPDATE_ROW = "update(reduce+fc5wgrad+rmsprop)"
GEN64 = dict(datatype="float64", screen_height=36, screen_width=38, history_length=4)
GEN32 = dict(screen_height=96, screen_width=96, history_length=4)
PER = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000)
# name: (batch size, make_args keywords) — the tuned path's regimes
TUNED = {"fp32_b32": (32, {}), "fp32_b128": (128, {}), "fp16_b32": (32, dict(datatype="float16")), "fp16_b128": (128, dict(datatype="float16")),
         "bn_b32": (32, dict(batch_norm=True)), "fp32_b32_adam": (32, dict(optimizer="adam"))}
GENERIC = {"f64_36x38": (8, GEN64), "f32_96x96": (8, GEN32)}


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _geom(kw):
    return kw.get("history_length", 4), kw.get("screen_height", 84), kw.get("screen_width", 84)


def _dtype(kw):
    return np.float64 if kw.get("datatype") == "float64" else np.float32


def _net(sd, B, kw, clip=None, seed=11, a=A):
    net = sd.DeepQNetwork(a, make_args(batch_size=B, **kw))
    ws, wt = xavier_weights(a, seed, _dtype(kw), *_geom(kw)), xavier_weights(a, seed + 1, _dtype(kw), *_geom(kw))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    if clip is not None:
        net.set_clip_grad_norm(clip)
    return net, ws, wt


def _ring(sd, B, kw, seed=3, a=A):
    mem = sd.ReplayMemory(RING, make_args(batch_size=B, **kw))
    synthetic_fill(mem, seed, num_actions=a)
    mem.sync_mirror()
    return mem


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _state(net, bn=False):
    """everything an applied step moves: weights, both optimizer states (+ the BatchNorm block and its running statistics)"""
    whichs = (0, 2) if net.optimizer == "rmsprop" else (0, 2, 4)
    out = [net.get_layer(i, w) for w in whichs for i in range(5)]
    if bn:
        out += [x for l in range(4) for w in whichs for x in net.get_bn(l, w)]
        out += [x for l in range(4) for x in net.get_bn(l, 0, running=True)]
    return out


def _assert_same_state(n1, n2, bn=False):
    for k, (a, b) in enumerate(zip(_state(n1, bn), _state(n2, bn))):
        assert _same_bits(a, b), k


def _grad(net, bn=False):
    """the flat gradient sums as arrays: the five layers (+ the four [beta | gamma] pairs)"""
    out = [net.get_layer(i, 3) for i in range(5)]
    if bn:
        out += [x for l in range(4) for x in net.get_bn(l, 3)]
    return out


def _put_grad(net, g, bn=False):
    for i in range(5):
        net.set_layer(i, g[i], 3)
    if bn:
        for l in range(4):
            net.set_bn(l, g[5 + 2 * l], g[6 + 2 * l], which=3)


def _expected_scale(norm, G, dt=np.float32):
    return clip_scale(norm, G, dt)


# ---- 1 + 2. the clipped step equals the explicit route; the norm is the gradient's ----------------------------------------------------------
@pytest.mark.parametrize("name", list(TUNED))
def test_clipped_step_equals_the_explicit_route(sd, name):
    """X: clipping on, one step.  Y: clipping off, grad_only step; the host scales g in float32 by the scale the semantics give from X's
    reported norm, writes it back and applies it.  Weights, optimizer state(s) and the BatchNorm block bit for bit.
    The norm: X's against sqrt(sum(float64(g)^2)) / B of Y's g, relative 1e-9 — fp64 accumulation in any order over NP < 1.8 M terms
    errs by at most NP x 2^-53 ~ 2e-10; margin 5."""
    B, kw = TUNED[name]
    bn = bool(kw.get("batch_norm"))
    x, _, _ = _net(sd, B, kw)
    y, _, _ = _net(sd, B, kw)
    mem = _ring(sd, B, kw)
    idx = np.arange(10, 10 + B, dtype=np.int64)
    y.set_option("grad_only", 1)
    y.train_indexes(mem, idx)
    g = _grad(y, bn)
    norm_y = grad_norm(g, B)
    assert math.isfinite(norm_y) and norm_y > 0
    G = norm_y / 2
    x.set_clip_grad_norm(G)
    assert x.step_structure()[1] == "clip"
    x.train_indexes(mem, idx)
    norm, scale = x.last_grad_norm()
    print("%s: norm %.17g (host %.17g), scale %.9g" % (name, norm, norm_y, scale))
    assert abs(norm - norm_y) <= 1e-9 * norm_y
    sc = _expected_scale(norm, G)
    assert sc < 1 and float(sc) == scale
    _put_grad(y, [(a * sc).astype(np.float32) for a in g], bn)
    y.apply_update(B)
    _assert_same_state(x, y, bn)
    for a, b in zip(_grad(x, bn), _grad(y, bn)):                           # X's g was scaled in place to the same values
        assert _same_bits(a, b)


def _gen_minibatch(B, kw, seed):
    rng = np.random.RandomState(seed)
    shp = (B,) + _geom(kw)
    return (rng.randint(0, 256, shp, dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8), rng.randint(-2, 3, B).astype(np.int64),
            rng.randint(0, 256, shp, dtype=np.uint8), rng.rand(B) < 0.25)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-300))


@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_path_against_the_oracle(sd, name):
    """The generic nets have no grad_only: one clipped step against ClipOracle at the bounds tests/test_gpu_generic.py holds one step to
    (float64: gradient 1e-11, weights 1e-12, state 1e-10; float32: 2e-5, 2e-6, 8e-5; all relative).  The norm is held to the gradient's
    bound against the oracle's, and against the device's own clipped g: norm(g') / B = norm x scale up to the multiplies' rounding
    (2^-24 relative per element in float32, 2^-53 in float64; bounds 1e-7 / 1e-12 leave the accumulation's 2e-10 room)."""
    B, kw = GENERIC[name]
    dt = _dtype(kw)
    hist, H, W = _geom(kw)
    net, ws, wt = _net(sd, B, kw)
    mb = _gen_minibatch(B, kw, 5)
    o = ClipOracle(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=dt, weights=ws)
    o.Wt = [w.copy() for w in wt]
    G = grad_norm(o.gradients(mb)[0], B) / 2
    o.clip_grad_norm = G
    net.set_clip_grad_norm(G)
    assert net.step_structure() == ("generic", "clip")
    net.train(mb)
    o.train(mb)
    norm, scale = net.last_grad_norm()
    tol_g, tol_w, tol_s = (1e-11, 1e-12, 1e-10) if dt is np.float64 else (2e-5, 2e-6, 8e-5)
    print("%s: norm %.17g (oracle %.17g), scale %.9g" % (name, norm, o.last_norm, scale))
    assert o.last_scale < 1 and abs(norm - o.last_norm) <= tol_g * o.last_norm
    assert float(clip_scale(norm, G, dt)) == scale and scale < 1
    g_dev = [net.get_layer(l, 3) for l in range(5)]
    assert abs(grad_norm(g_dev, B) - norm * scale) <= (1e-12 if dt is np.float64 else 1e-7) * norm * scale
    for l in range(5):
        assert _rel(net.get_layer(l, 0), o.W[l]) < tol_w, ("weights", l)
        assert _rel(net.get_layer(l, 2), o.S[l]) < tol_s, ("rmsprop state", l)


def test_generic_clipped_gradient_against_the_oracle(sd):
    """the clipped gradient itself, float64 generic net: g' = g x scale against the oracle's at the one-step gradient bound 1e-11"""
    B, kw = GENERIC["f64_36x38"]
    hist, H, W = _geom(kw)
    net, ws, wt = _net(sd, B, kw)
    mb = _gen_minibatch(B, kw, 6)
    o = ClipOracle(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=np.float64, weights=ws)
    o.Wt = [w.copy() for w in wt]
    g = o.gradients(mb)[0]
    G = grad_norm(g, B) / 2
    net.set_clip_grad_norm(G)
    net.train(mb)
    sc = clip_scale(grad_norm(g, B), G, np.float64)
    for l in range(5):
        assert _rel(net.get_layer(l, 3), g[l] * sc) < 1e-11, l


# ---- 3. edges of the reduction, through apply_update -----------------------------------------------------------------------------------
def _hand_gradient(net, a, bn):
    """all zero except the FIRST element of the flat buffer = 3 and its LAST = 4 (conv1's (0, 0); fc5's last, or the last gamma of the
    BatchNorm block, which ends the buffer the optimizer reads)"""
    shapes = [(256, 32), (512, 64), (576, 64), (512, 3136), (a, 512)]
    g = [np.zeros(s, np.float32) for s in shapes]
    g[0][0, 0] = 3
    if bn:
        g += [np.zeros(c, np.float32) for c in (32, 32, 64, 64, 64, 64, 512, 512)]
        g[-1][-1] = 4
    else:
        g[4][-1, -1] = 4
    _put_grad(net, g, bn)
    return g


@pytest.mark.parametrize("a,bn,bsz", [(1, False, 32), (3, False, 32), (3, True, 32), (3, False, 64)], ids=["a1", "a3", "bn", "bsz64"])
def test_first_and_last_element_of_the_flat_buffer(sd, a, bn, bsz):
    G = 0.05
    net, _, _ = _net(sd, 32, dict(batch_norm=True) if bn else {}, clip=G, a=a)
    g = _hand_gradient(net, a, bn)
    net.apply_update(bsz)
    norm, scale = net.last_grad_norm()
    assert abs(norm - 5.0 / bsz) <= 1e-12 * (5.0 / bsz)
    sc = _expected_scale(norm, G)
    assert sc < 1 and float(sc) == scale
    want = [(x * sc).astype(np.float32) for x in g]
    got = _grad(net, bn)
    assert got[0][0, 0] == np.float32(3) * sc and got[-1].reshape(-1)[-1] == np.float32(4) * sc
    for x, y in zip(got, want):
        assert _same_bits(x, y)


def test_all_zero_gradient_changes_nothing(sd):
    net, ws, _ = _net(sd, 32, {}, clip=0.05)
    before = _state(net)
    net.apply_update(32)
    assert net.last_grad_norm() == (0.0, 1.0)
    for a, b in zip(before, _state(net)):
        assert _same_bits(a, b)
    assert all(not x.any() for x in _grad(net))


def test_bound_far_above_the_norm_is_the_unclipped_update(sd):
    rng = np.random.RandomState(9)
    g = [rng.standard_normal(s).astype(np.float32) for s in [(256, 32), (512, 64), (576, 64), (512, 3136), (A, 512)]]
    on, _, _ = _net(sd, 32, {}, clip=1e9)
    off, _, _ = _net(sd, 32, {})
    for net in (on, off):
        _put_grad(net, g)
        net.apply_update(32)
    norm, scale = on.last_grad_norm()
    assert scale == 1.0 and abs(norm - grad_norm(g, 32)) <= 1e-9 * norm
    _assert_same_state(on, off)
    for a, b, c in zip(_grad(on), _grad(off), g):
        assert _same_bits(a, b) and _same_bits(a, c)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
def test_the_same_clipped_step_twice_gives_the_same_bits(sd):
    mem = _ring(sd, 32, {})
    nets = []
    for _ in range(2):
        net, _, _ = _net(sd, 32, {}, clip=0.01)
        random.seed(17)
        net.train_from_memory(mem, 2)
        nets.append(net)
    _assert_same_state(*nets)
    assert nets[0].last_grad_norm() == nets[1].last_grad_norm() and nets[0].last_grad_norm()[1] < 1
    for a, b in zip(_grad(nets[0]), _grad(nets[1])):
        assert _same_bits(a, b)


# ---- 5. free-running steps against the fp64 oracle ---------------------------------------------------------------------------------------
_MBS = [random_minibatch(32, A, 100 + i, p_term=0.05, reward_range=(-1, 2)) for i in range(5)]


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_five_free_running_steps_against_the_fp64_oracle(sd, optimizer):
    """float32, B = 32, five free-running steps against the fp64 step with the fp64 clip.  G: half the smallest pre-clip norm the oracle
    computes over the five steps (a probe pass of the oracle in float32, clipping off), so every step clips — asserted on the fp64
    oracle's own scales.  Bound: tests/test_gpu_soft_target.py's five-step test, Q max abs error 1e-4 on a held-out batch."""
    Q_TOL = 1e-4
    kw = dict(optimizer=optimizer)
    net, ws, wt = _net(sd, 32, kw, seed=21)
    probe = ClipOracle(A, batch_size=32, weights=ws, dtype=np.float32, optimizer=optimizer, clip_grad_norm=1e30)
    probe.Wt = [np.asarray(w, np.float32) for w in wt]
    norms = []
    for mb in _MBS:
        probe.train(mb)
        norms.append(probe.last_norm)
    G = min(norms) / 2
    o = ClipOracle(A, batch_size=32, weights=ws, dtype=np.float64, optimizer=optimizer, clip_grad_norm=G)
    o.Wt = [np.asarray(w, np.float64) for w in wt]
    net.set_clip_grad_norm(G)
    hold = random_minibatch(32, A, 99)[0]
    for mb in _MBS:
        net.train(mb)
        o.train(mb)
        assert o.last_scale < 1
    norm, scale = net.last_grad_norm()
    err = np.abs(net.predict(hold) - o.predict(hold)).max()
    print("%s, 5 clipped steps, G %.4g: Q max abs err vs fp64 oracle %.3e; last norm %.6g (oracle %.6g) scale %.6g" %
          (optimizer, G, err, norm, o.last_norm, scale))
    assert err < Q_TOL
    assert scale < 1


def test_composes_with_prioritized_replay_and_n_step(sd):
    """--prioritized_replay and --n_step 3 with clipping: the first step's new priorities come from the TD errors, which the clip does not
    touch, so they equal the unclipped run's bit for bit while the weights differ; five steps on, everything is finite and every
    reported scale is the semantics' function of the reported norm."""
    kw = dict(n_step=3, **PER)
    G = 1e-3
    on, _, _ = _net(sd, 32, kw, clip=G)
    off, _, _ = _net(sd, 32, kw)
    mems = [_ring(sd, 32, kw), _ring(sd, 32, kw)]
    for net, mem in zip((on, off), mems):
        random.seed(23)
        net.train_from_memory(mem, 1)
    assert _same_bits(mems[0].priorities(), mems[1].priorities())
    assert not _same_bits(on.get_layer(3, 0), off.get_layer(3, 0))
    for _ in range(4):
        on.train_from_memory(mems[0], 1)
        norm, scale = on.last_grad_norm()
        assert math.isfinite(norm) and scale < 1 and scale == float(_expected_scale(norm, G))
    assert all(np.isfinite(w).all() for w in on.get_weights(0))
    assert np.isfinite(mems[0].priorities()).all()


# ---- 6. launches ---------------------------------------------------------------------------------------------------------------------------
def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("name", [k for k in TUNED if "adam" not in k] + list(GENERIC))
def test_three_more_launches_per_step_and_none_with_the_option_off(sd, name):
    """on: the update slot holds mode 1, sqnorm, scale and mode 2 where the default step has its one update launch — three more, every
    other row unchanged.  (The generic path's own launches are not bracketed; its clipped step adds sqnorm and scale and brackets them
    together with its deferred optimizer launch: three in the update row, none without the option.)"""
    generic = name in GENERIC
    B, kw = (GENERIC if generic else TUNED)[name]
    mb = _gen_minibatch(B, kw, 4)
    nets = [sd.DeepQNetwork(A, make_args(batch_size=B, **kw)) for _ in range(3)]
    never, off, on = nets
    off.set_clip_grad_norm(0.0)
    on.set_clip_grad_norm(10.0)
    old = never.step_structure()
    assert off.step_structure() == old and on.step_structure() == (old[0], "clip")
    c_never, c_off, c_on = [_counts(net, lambda net=net: net.train(mb)) for net in nets]
    assert c_off == c_never
    assert c_on.get(UPDATE_ROW) == c_never.get(UPDATE_ROW, 0) + 9          # 3 steps x 3
    assert {k: v for k, v in c_on.items() if k != UPDATE_ROW} == {k: v for k, v in c_never.items() if k != UPDATE_ROW}
    assert sum(c_on.values()) == sum(c_never.values()) + 9
    on.set_clip_grad_norm(0.0)                                             # switched off between steps: the default step again
    assert _counts(on, lambda: on.train(mb)) == c_never and on.step_structure() == old


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, GEN64], ids=["tuned", "generic"])
def test_arguments(sd, kw):
    net, _, _ = _net(sd, 8, kw, clip=2.5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AssertionError):
            net.set_clip_grad_norm(bad)
        assert sd.load().sdqn_net_set_clip_grad_norm(net._h, bad) == -1    # SDQN_ERR_ARG
    g = __import__("ctypes").c_double()
    assert sd.load().sdqn_net_get_clip_grad_norm(net._h, g) == 0 and g.value == 2.5 and net.clip_grad_norm == 2.5
    with pytest.raises(sd._lib.SdqnError):
        net.last_grad_norm()                                               # no clipped step yet
    assert sd.load().sdqn_net_last_grad_norm(net._h, None, None) == -4     # SDQN_ERR_STATE
    net.train(_gen_minibatch(8, kw, 2))
    norm, scale = net.last_grad_norm()
    assert math.isfinite(norm) and 0 < scale <= 1


def test_switching_off_restores_the_fused_rmsprop(sd):
    """fc4's RMSProp rides its weight-gradient launch again (StepArgs::fuse_rms): that step does not materialise fc4's gradient, so a
    mark written into g's fc4 block survives it; the clipped step before it wrote the block"""
    net, _, _ = _net(sd, 32, {}, clip=10.0)
    mb = random_minibatch(32, A, 7)
    mark = np.full((512, 3136), 7.0, np.float32)
    net.set_layer(3, mark, 3)
    net.train(mb)
    assert not _same_bits(net.get_layer(3, 3), mark)
    net.set_clip_grad_norm(0.0)
    assert net.step_structure()[1] == "single"
    net.set_layer(3, mark, 3)
    net.train(mb)
    assert _same_bits(net.get_layer(3, 3), mark)


# ---- 8. the loop -------------------------------------------------------------------------------------------------------------------------------
def test_main_loop_on_catch_with_train_envs(sd):
    from simple_dqn_amd import main as M
    argv = ["--environment", "catch", "--train_envs", "8", "--clip_grad_norm", "10", "--replay_size", "800", "--random_steps", "160",
            "--train_steps", "240", "--test_steps", "0", "--epochs", "1", "--exploration_decay_steps", "200", "--target_steps", "64",
            "--random_seed", "7"]
    args = M.build_parser().parse_args(argv)
    stats = M.run(args)
    net = stats.net
    assert net.clip_grad_norm == 10.0 and net.train_iterations == 240 // 4 and net.step_structure()[1] == "clip"
    assert all(np.isfinite(w).all() for w in net.get_weights(0))
    norm, scale = net.last_grad_norm()
    assert math.isfinite(norm) and norm > 0 and 0 < scale <= 1
