"""--target_tau on the GPU: the blend kernel bit for bit against numpy (tests/soft_target_oracle.py), the target's
derived weight copies through the train steps that read them, the per-step mode against explicit calls on every entry point, tau = 1
against the hard update, five free-running steps against the fp64 oracle, launch counts, refusals and the main loop."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from soft_target_oracle import SoftTargetOracle, blend
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu
B = 32
RING = 400
GENERIC = dict(datatype="float64", screen_height=36, screen_width=38, history_length=4)
# name: (A, make_args keywords)
BLEND_CONFIGS = {}
for _a in (1, 4, 18):
    BLEND_CONFIGS["fp32_a%d" % _a] = (_a, {})
    BLEND_CONFIGS["fp16_a%d" % _a] = (_a, dict(datatype="float16"))
BLEND_CONFIGS["bn_a4"] = (4, dict(batch_norm=True))
BLEND_CONFIGS["f64_generic_a4"] = (4, GENERIC)
BLEND_NAME = "target_blend(polyak)"


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _geom(kw):
    return kw.get("history_length", 4), kw.get("screen_height", 84), kw.get("screen_width", 84)


def _dtype(kw):
    return np.float64 if kw.get("datatype") == "float64" else np.float32


def _net(sd, A, kw, tau=None, seed=11, **extra):
    """net with online / target weights from two different draws (returned too)"""
    net = sd.DeepQNetwork(A, make_args(batch_size=B, **kw, **extra))
    ws, wt = xavier_weights(A, seed, _dtype(kw), *_geom(kw)), xavier_weights(A, seed + 1, _dtype(kw), *_geom(kw))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    if tau is not None:
        net.set_target_tau(tau)
    return net, ws, wt


def _bn_fill(net, seed):
    """random BatchNorm parameters and running statistics of both nets; returns {(l, which, running): (first, second)}"""
    rng, out = np.random.RandomState(seed), {}
    for l, c in enumerate((32, 64, 64, 512)):
        for which in (0, 1):
            for running in (False, True):
                a, b = rng.uniform(-0.5, 0.5, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)
                net.set_bn(l, a, b, which=which, running=running)
                out[(l, which, running)] = (a, b)
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ring(sd, A, kw, seed=3):
    args = make_args(batch_size=B, **kw)
    mem = sd.ReplayMemory(RING, args)
    synthetic_fill(mem, seed, num_actions=A)
    mem.sync_mirror()
    return mem


def _state(net, bn=False):
    """everything a train step moves: online weights, target weights, optimizer state (+ the BatchNorm blocks)"""
    out = [net.get_layer(i, which) for which in (0, 1, 2) for i in range(5)]
    if bn:
        out += [x for l in range(4) for which in (0, 1, 2) for x in net.get_bn(l, which)]
        out += [x for l in range(4) for which in (0, 1) for x in net.get_bn(l, which, running=True)]
    return out


def _assert_same_state(n1, n2, bn=False):
    for k, (a, b) in enumerate(zip(_state(n1, bn), _state(n2, bn))):
        assert _same_bits(a, b), k


# ---- 1. one blend, bit-exact -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BLEND_CONFIGS))
def test_one_blend_is_bit_exact(sd, name):
    A, kw = BLEND_CONFIGS[name]
    dt = _dtype(kw)
    net, ws, wt = _net(sd, A, kw)
    bn = _bn_fill(net, 5) if kw.get("batch_norm") else None
    net.soft_update_target_network(0.25)
    for i in range(5):
        assert _same_bits(net.get_layer(i, 1), blend(ws[i], wt[i], 0.25, dt)), i
        assert _same_bits(net.get_layer(i, 0), np.asarray(ws[i], dt)), i
    if bn:
        # a hard update copies beta / gamma AND the running statistics of the target, so a soft update blends both
        for l in range(4):
            for running in (False, True):
                got, on = net.get_bn(l, 1, running=running), net.get_bn(l, 0, running=running)
                for j in range(2):
                    assert _same_bits(got[j], blend(bn[(l, 0, running)][j], bn[(l, 1, running)][j], 0.25)), (l, running, j)
                    assert _same_bits(on[j], bn[(l, 0, running)][j]), (l, running, j)
    # a second blend starts from the first one's result
    net.soft_update_target_network(0.5)
    for i in range(5):
        assert _same_bits(net.get_layer(i, 1), blend(ws[i], blend(ws[i], wt[i], 0.25, dt), 0.5, dt)), i


# ---- 2. derived copies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BLEND_CONFIGS))
def test_derived_copies_follow_the_blend(sd, name):
    """net X blends on the device, net Y receives the oracle's blended target through set_weights(which = 1), which rebuilds the bf16
    planes / half copies; two train steps then read them (a stale copy shows as another maxpostq and other weights)"""
    A, kw = BLEND_CONFIGS[name]
    dt, isbn = _dtype(kw), bool(kw.get("batch_norm"))
    x, ws, wt = _net(sd, A, kw)
    y, _, _ = _net(sd, A, kw)
    if isbn:
        bn = _bn_fill(x, 5); _bn_fill(y, 5)
    x.soft_update_target_network(0.3)
    y.set_weights([blend(ws[i], wt[i], 0.3, dt) for i in range(5)], 1)
    if isbn:
        for l in range(4):
            for running in (False, True):
                y.set_bn(l, *[blend(bn[(l, 0, running)][j], bn[(l, 1, running)][j], 0.3) for j in range(2)], which=1, running=running)
    if "screen_height" in kw:                                              # generic geometry: two minibatches of its own shape
        rng = np.random.RandomState(8)
        shp = (B,) + _geom(kw)
        mbs = [(rng.randint(0, 256, shp, dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8), rng.randint(-1, 2, B).astype(np.int64),
                rng.randint(0, 256, shp, dtype=np.uint8), rng.rand(B) < 0.1) for _ in range(2)]
        for net in (x, y):
            for mb in mbs:
                net.train(mb)
    else:
        mem = _ring(sd, A, kw)
        for net in (x, y):
            random.seed(17)
            net.train_from_memory(mem, 2)
    _assert_same_state(x, y, isbn)
    for a, b in zip(x.last_q(), y.last_q()):
        assert _same_bits(a, b)


# ---- 3. in-step mode equals explicit calls ---------------------------------------------------------------------------------------
STEP_CONFIGS = {
    "fp32": dict(), "fp32_ddqn": dict(double_dqn=True), "fp16": dict(datatype="float16"), "fp16_ddqn": dict(datatype="float16", double_dqn=True),
    "fp32_per": dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000),
}


@pytest.mark.parametrize("name", list(STEP_CONFIGS))
def test_in_step_mode_equals_explicit_calls(sd, name):
    A, kw, tau = 4, STEP_CONFIGS[name], 0.1
    per = bool(kw.get("prioritized_replay"))
    auto, _, _ = _net(sd, A, kw, tau=tau)
    hand, _, _ = _net(sd, A, kw)
    assert auto.get_target_tau() == tau and hand.get_target_tau() == 0.0
    mems = [_ring(sd, A, kw), _ring(sd, A, kw)]                            # (one each: a prioritized memory's priorities move with the steps)

    def same():
        _assert_same_state(auto, hand)
        if per:
            assert _same_bits(mems[0].priorities(), mems[1].priorities())

    random.seed(21)
    auto.train_from_memory(mems[0], 3)
    random.seed(21)
    for _ in range(3):
        hand.train_from_memory(mems[1], 1)
        hand.soft_update_target_network(tau)
    same()
    # the target has moved, and not onto the online net
    assert not _same_bits(auto.get_layer(3, 1), auto.get_layer(3, 0))
    # ... through train(getMinibatch())
    for net, mem in ((auto, mems[0]), (hand, mems[1])):
        random.seed(22)
        for _ in range(2):
            net.train(mem.getMinibatch())
            if net is hand:
                net.soft_update_target_network(tau)
    same()
    # ... and through train_replay (given indexes)
    idx = np.arange(10, 10 + B, dtype=np.int64)
    for net, mem in ((auto, mems[0]), (hand, mems[1])):
        for _ in range(2):
            net.train_indexes(mem, idx)
            if net is hand:
                net.soft_update_target_network(tau)
    same()


def test_grad_only_step_does_not_blend_and_apply_update_does(sd):
    A = 4
    net, ws, wt = _net(sd, A, {}, tau=0.1)
    mb = random_minibatch(B, A, 5)
    net.set_option("grad_only", 1)
    net.train(mb)
    for i in range(5):
        assert _same_bits(net.get_layer(i, 1), wt[i]), i
    net.apply_update(B)
    for i in range(5):
        assert _same_bits(net.get_layer(i, 1), blend(net.get_layer(i, 0), wt[i], 0.1)), i


# ---- 4. tau = 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fp32", "fp16"])
def test_tau_one_is_the_hard_update(sd, name):
    A, kw = 4, STEP_CONFIGS[name]
    soft, _, _ = _net(sd, A, kw, tau=1.0)
    hard, _, _ = _net(sd, A, kw)
    mem = _ring(sd, A, kw)
    random.seed(31)
    soft.train_from_memory(mem, 3)
    random.seed(31)
    for _ in range(3):
        hard.train_from_memory(mem, 1)
        hard.update_target_network()
    _assert_same_state(soft, hard)
    for i in range(5):
        assert _same_bits(soft.get_layer(i, 1), soft.get_layer(i, 0)), i
    for a, b in zip(soft.last_q(), hard.last_q()):
        assert _same_bits(a, b)


# ---- 5. against the fp64 oracle --------------------------------------------------------------------------------------------------
def test_five_free_running_steps_against_the_fp64_oracle(sd):
    """float32, A = 4, tau = 0.05, five free-running steps against the fp64 step + fp64 blend.  Bound: tests/test_gpu_dqn.py's Q_TOL = 1e-4,
    which test_multi_step_q_parity_free_running holds after 1 and after 10 free-running steps."""
    A, tau, Q_TOL = 4, 0.05, 1e-4
    net, ws, wt = _net(sd, A, {}, tau=tau, seed=21)
    o = SoftTargetOracle(A, batch_size=B, weights=ws, dtype=np.float64, tau=tau)
    o.Wt = [np.asarray(w, np.float64) for w in wt]
    hold = random_minibatch(B, A, 99)[0]
    mbs = [random_minibatch(B, A, 100 + i, p_term=0.05, reward_range=(-1, 2)) for i in range(5)]
    for mb in mbs:
        net.train(mb)
        o.train(mb)
    err = np.abs(net.predict(hold) - o.predict(hold)).max()
    errt = max(np.abs(net.get_layer(i, 1) - o.Wt[i]).max() for i in range(5))
    print("5 steps, tau %.2f: Q max abs err vs fp64 oracle %.3e, target weights max abs err %.3e" % (tau, err, errt))
    assert err < Q_TOL
    # and the target really is the blended one: a net whose target stood still is farther from the oracle's target than that
    assert max(np.abs(np.asarray(wt[i], np.float64) - o.Wt[i]).max() for i in range(5)) > 10 * errt


# ---- 6. launches ---------------------------------------------------------------------------------------------------------------------
def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


LAUNCH_CONFIGS = {"fp32_b32": (32, {}), "fp32_b128": (128, {}), "fp16_b32": (32, dict(datatype="float16")),
                  "bn_b32": (32, dict(batch_norm=True)), "generic": (8, GENERIC)}


@pytest.mark.parametrize("name", list(LAUNCH_CONFIGS))
def test_one_more_launch_per_step_and_none_with_the_option_off(sd, name):
    A, (Bn, kw) = 4, LAUNCH_CONFIGS[name]
    rng = np.random.RandomState(4)
    shp = (Bn,) + _geom(kw)
    mb = (rng.randint(0, 256, shp, dtype=np.uint8), rng.randint(0, A, Bn).astype(np.uint8), rng.randint(-1, 2, Bn).astype(np.int64),
          rng.randint(0, 256, shp, dtype=np.uint8), rng.rand(Bn) < 0.1)
    nets = [sd.DeepQNetwork(A, make_args(batch_size=Bn, **kw)) for _ in range(3)]
    never, off, on = nets
    off.set_target_tau(0.0)
    on.set_target_tau(0.005)
    c_never, c_off, c_on = [_counts(net, lambda net=net: net.train(mb)) for net in nets]
    assert c_off == c_never                                                # guards the default: per-kernel counts unchanged
    assert BLEND_NAME not in c_never
    assert c_on.get(BLEND_NAME) == 3                                       # n launches for n steps in the new row
    assert {k: v for k, v in c_on.items() if k != BLEND_NAME} == c_never
    assert sum(c_on.values()) == sum(c_never.values()) + 3
    on.set_target_tau(0.0)                                                 # switched off between steps: the standard step again
    assert _counts(on, lambda: on.train(mb)) == c_never


@pytest.mark.parametrize("kw", [{}, GENERIC], ids=["tuned", "generic"])
def test_without_a_target_net_nothing_is_launched(sd, kw):
    A = 4
    net = sd.DeepQNetwork(A, make_args(batch_size=8, target_steps=0, **kw))
    w0 = net.get_weights(0)
    lib = sd.load()
    net.profile(True, -1); net.profile_reset()
    assert lib.sdqn_net_soft_update(net._h, 0.25) == 0                     # SDQN_OK
    assert lib.sdqn_net_soft_update(net._h, 1.0) == 0
    assert not [p for p in net.profile_read() if p["launches"]]
    net.profile(False)
    for a, b in zip(w0, net.get_weights(0)):
        assert _same_bits(a, b)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, GENERIC], ids=["tuned", "generic"])
def test_refusals_leave_the_target_untouched(sd, kw):
    A = 4
    net, ws, wt = _net(sd, A, kw)
    lib = sd.load()
    for tau in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        assert lib.sdqn_net_soft_update(net._h, tau) == -1, tau            # SDQN_ERR_ARG
        with pytest.raises(AssertionError):
            net.soft_update_target_network(tau)
    for tau in (2.0, -0.5, float("nan")):
        assert lib.sdqn_net_set_target_tau(net._h, tau) == -1, tau
    assert net.get_target_tau() == 0.0
    for i in range(5):
        assert _same_bits(net.get_layer(i, 1), np.asarray(wt[i], _dtype(kw))), i


# ---- 8. the loop -----------------------------------------------------------------------------------------------------------------------
def test_main_loop_on_catch_with_train_envs(sd):
    from simple_dqn_amd import main as M
    argv = ["--environment", "catch", "--train_envs", "8", "--target_tau", "0.01", "--replay_size", "800", "--random_steps", "160",
            "--train_steps", "240", "--test_steps", "0", "--epochs", "1", "--exploration_decay_steps", "200", "--target_steps", "64",
            "--random_seed", "7"]
    args = M.build_parser().parse_args(argv)
    fresh = sd.DeepQNetwork(3, args)                                       # the same seed's initial draws
    w_init, wt_init = fresh.get_weights(0), fresh.get_weights(1)
    stats = M.run(args)
    net = stats.net
    assert net.get_target_tau() == 0.01 and net.train_iterations == 240 // 4
    wt, w = net.get_weights(1), net.get_weights(0)
    assert all(not _same_bits(a, b) for a, b in zip(wt, wt_init))          # left its own initial draw (the step-0 hard copy) ...
    assert all(not _same_bits(a, b) for a, b in zip(wt, w_init))           # ... and the online net's, which it was copied from,
    assert all(not _same_bits(a, b) for a, b in zip(wt, w))                # and has not been hard-copied since
    # 60 blends of 0.01 leave the target closer to where it started than to where the online net went
    d_init = sum(float(np.abs(a - b).sum()) for a, b in zip(wt, w_init))
    d_on = sum(float(np.abs(a - b).sum()) for a, b in zip(wt, w))
    assert d_init < d_on
