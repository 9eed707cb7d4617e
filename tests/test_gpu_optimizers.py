"""Adam and Adadelta (and RMSProp next to them) on every path of the tuned step: the optimizer pass in isolation against the float64
evaluation of oracle/dqn_numpy.py's formulas, the copies derived from the master weights (half weights, conv1's bf16 planes), free-running
parity, the library's loops (uniform, prioritized, single-rank data parallel) and the second state at the API.

Non-default optimizers switch the step to the unfused update (the `opt != 0` branches of opt_apply4); before this file they ran on the
tuned path once, float32 A = 4 B = 16, with the weights never compared."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.dqn_numpy import OracleDQN, xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

OPTS = ["rmsprop", "adam", "adadelta"]
Q_TOL = 1e-4
FLT_MIN = float(np.finfo(np.float32).tiny)
MARGIN = 32           # over the float32 restatement's own distance from float64 (the margin tests/test_gpu_batch_edges.py gives the
                      # device over the oracle's own noise): fma contraction, another order of the division and square root — ulps each


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _net(sd, opt, A, B, dt="float32", seed=1201, **kw):
    net = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=opt, datatype=dt, **kw))
    net.set_weights(xavier_weights(A, seed + 1), 1)
    net.set_weights(xavier_weights(A, seed), 0)
    return net


def _read(net, opt):
    """(weights, first state, second state or None) in Neon layout"""
    return ([net.get_layer(i, 0) for i in range(5)], [net.get_layer(i, 2) for i in range(5)],
            [net.get_layer(i, 4) for i in range(5)] if opt != "rmsprop" else None)


def formula(opt, dtype, before, g, B, epoch):
    """one optimizer step of oracle/dqn_numpy.py in `dtype` from (weights, first state, second state) and the gradient SUMS g"""
    W, S, S2 = before
    o = OracleDQN(W[4].shape[0], batch_size=B, dtype=dtype, weights=[np.asarray(w, dtype) for w in W], optimizer=opt)
    o.S = [np.asarray(s, dtype) for s in S]
    if S2 is not None:
        o.S2 = [np.asarray(s, dtype) for s in S2]
    o.optimize([np.asarray(x, dtype) for x in g], B, epoch)
    return o.W, o.S, (o.S2 if S2 is not None else None)


def second_moments(opt, res):
    """the accumulators of squares of a formula() result: RMSProp's state, Adam's v, Adadelta's E[g^2] and E[dx^2]"""
    _, S, S2 = res
    return [S] if opt == "rmsprop" else ([S2] if opt == "adam" else [S, S2])


def isolation_distances(opt, before, g, B, epoch, device=None):
    """Per layer and per quantity (weights, first state, second state): r = the float32 restatement's largest distance from the float64
    result relative to the layer's largest update, [the device's the same way,] over the elements whose float64 second moments are
    normal float32 numbers or exactly zero (a dead unit's gradient is exactly zero in every sample: nothing denormal about it, and the
    update must then leave the element alone — only 0 < moment < FLT_MIN, where denormal handling decides, is left out); and the share
    of a layer left out.  -> list over layers of dict(name -> (r, d)), list of shares."""
    r32, r64 = formula(opt, np.float32, before, g, B, epoch), formula(opt, np.float64, before, g, B, epoch)
    out, shares = [], []
    for i in range(5):
        keep = np.ones(before[0][i].shape, bool)
        for m in second_moments(opt, r64):
            keep &= ~((m[i] > 0) & (m[i] < FLT_MIN))
        shares.append(1.0 - float(keep.mean()))
        row = {}
        for k, name in enumerate(("weights", "state", "state2")):
            if r64[k] is None:
                continue
            ref, base = r64[k][i], np.asarray(before[k][i], np.float64)
            upd = np.abs(ref - base)[keep].max()
            r = np.abs(r32[k][i] - ref)[keep].max() / upd
            d = np.abs(device[k][i] - ref)[keep].max() / upd if device is not None else None
            row[name] = (float(r), None if d is None else float(d))
        out.append(row)
    return out, shares


def check_isolation(opt, before, g, B, epoch, device, label):
    rows, shares = isolation_distances(opt, before, g, B, epoch, device)
    worst = {}
    for i, row in enumerate(rows):
        assert shares[i] <= 1e-3, (label, i, shares[i])
        for name, (r, d) in row.items():
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], r), max(w[1], d)
    print("%s: %s" % (label, "; ".join("%s r %.2e device %.2e" % (n, w[0], w[1]) for n, w in worst.items())))
    for i, row in enumerate(rows):
        for name, (r, d) in row.items():
            assert r > 0 and d <= MARGIN * r, (label, "layer %d" % i, name, r, d)


# name: (datatype, B, A)
ISO = {"fp32_b32": ("float32", 32, 4), "fp32_b128": ("float32", 128, 4), "fp32_b256_a3": ("float32", 256, 3),
       "fp16_b32": ("float16", 32, 4), "fp16_b256": ("float16", 256, 4)}
ISO_CASES = [(o, 0) for o in OPTS] + [("adam", e) for e in (1, 5, 200)]


@pytest.mark.parametrize("opt,epoch", ISO_CASES)
@pytest.mark.parametrize("name", list(ISO))
def test_update_in_isolation(sd, name, opt, epoch):
    """Two steps; the second is the one under test, so that it starts from the non-zero state the first left.  From the device's own
    gradient sums of step 2 (which = 3) and its weights and state before it, the oracle's formula in float32 and in float64: the device's
    new weights, first and second state lie within 32 r of the float64 result, r the float32 restatement's own distance (both relative
    to the layer's largest update).  Adam at epochs 0, 1, 5, 200: the bias-corrected step size is lr sqrt(1 - b2^t) / (1 - b1^t) with
    t = epoch + 1 (t = epoch would divide by zero at epoch 0 and be 1.34 x the step at epoch 1).  B >= 128 walks more than 32
    split-K slabs in the reduction in front of the update; float16 refreshes both half copies behind it.

    Measured on MI355X (largest layer; r / device): DESIGN.md, section "Optimizers other than RMSProp"."""
    dt, B, A = ISO[name]
    net = _net(sd, opt, A, B, dt)
    net.set_option("keep_gradients", 1)
    net.train(random_minibatch(B, A, 1210), epoch)
    before = _read(net, opt)
    net.train(random_minibatch(B, A, 1211), epoch)
    g = [net.get_layer(i, 3) for i in range(5)]
    assert all(np.abs(x).max() > 0 for x in g)
    check_isolation(opt, before, g, B, epoch, _read(net, opt), "%s %s epoch %d" % (name, opt, epoch))


@pytest.mark.parametrize("dt", ["float32", "float16"])
@pytest.mark.parametrize("opt", OPTS)
def test_derived_copies_follow_the_master_weights(sd, opt, dt):
    """After three steps, a fresh net given the trained net's online and target weights computes the same bits: the half copies wh / wht
    (float16) and conv1's three bf16 planes (float32, conv1 on the bf16 MFMA: the default) were refreshed by the update kernel from the
    new master weights, exactly as set_weights derives them."""
    A, B = 4, 32
    net = _net(sd, opt, A, B, dt)
    for s in range(3):
        net.train(random_minibatch(B, A, 1220 + s), s)
    twin = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=opt, datatype=dt))
    for i in range(5):
        twin.set_layer(i, net.get_layer(i, 1), 1)
        twin.set_layer(i, net.get_layer(i, 0), 0)
    st = random_minibatch(B, A, 1229)[0]
    q, qt = net.predict(st), twin.predict(st)
    assert np.abs(q).max() > 0 and np.array_equal(q, qt)
    assert np.array_equal(net.predict_one(st[3]), twin.predict_one(st[3]))                 # the one-launch acting forward
    for n in (net, twin):
        n.set_option("act_kernel", 0)
    assert np.array_equal(net.predict_one(st[3]), twin.predict_one(st[3]))                 # and the five-launch one


@pytest.mark.parametrize("dt", ["float32", "float16"])
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_five_free_running_steps(sd, opt, dt):
    """Five steps (epochs 0, 0, 1, 1, 2) against OracleDQN(optimizer=...) without re-synchronisation, at the bounds of the RMSProp
    multi-step tests: float32 1e-4 on Q (test_multi_step_q_parity_free_running), float16 5e-2 against the half oracle
    (test_fp16_training_tracks_oracle_and_fused_path)."""
    A, B = 4, 32
    half = dt == "float16"
    net = _net(sd, opt, A, B, dt, seed=1231)
    o = OracleDQN(A, batch_size=B, weights=xavier_weights(A, 1231), optimizer=opt, half_activations=half)
    o.Wt = [w.copy() for w in xavier_weights(A, 1232)]
    hold = random_minibatch(B, A, 1239)[0]
    for s, epoch in enumerate((0, 0, 1, 1, 2)):
        mb = random_minibatch(B, A, 1233 + s, p_term=0.05, reward_range=(-1, 2))
        net.train(mb, epoch)
        o.train(mb, epoch)
    err = np.abs(net.predict(hold) - o.predict(hold)).max()
    print("%s %s: Q max abs err after 5 steps %.3e" % (dt, opt, err))
    assert err < (5e-2 if half else Q_TOL)


def _ring(sd, B, A=4, size=5000, **kw):
    mem = sd.ReplayMemory(size, make_args(batch_size=B, **kw))
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    return mem


def _same_state(n1, n2, opt):
    for i in range(5):
        for which in (0, 2) + ((4,) if opt != "rmsprop" else ()):
            assert np.array_equal(n1.get_layer(i, which), n2.get_layer(i, which)), (i, which)


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("opt,epoch", [("adam", 0), ("adam", 3), ("adadelta", 0)])
def test_library_loop_equals_single_steps(sd, opt, epoch, B):
    """train_from_memory(mem, 4) after set_epoch(e) — the loop reads the handle's epoch — against four train(mem.getMinibatch(), e) of a
    twin from the same random state: weights and both states bit for bit."""
    A, n = 4, 4
    mem = _ring(sd, B)
    n1, n2 = _net(sd, opt, A, B), _net(sd, opt, A, B)
    random.seed(7)
    st = random.getstate()
    n1.set_epoch(epoch)
    n1.train_from_memory(mem, n)
    after = random.getstate()
    random.setstate(st)
    for _ in range(n):
        n2.train(mem.getMinibatch(), epoch)
    assert random.getstate() == after
    _same_state(n1, n2, opt)
    if opt == "adam" and epoch:                                         # the epoch reached the loop: epoch 0 ends elsewhere
        n3 = _net(sd, opt, A, B)
        random.setstate(st)
        n3.train_from_memory(mem, n)
        assert not np.array_equal(n1.get_layer(4, 0), n3.get_layer(4, 0))


@pytest.mark.parametrize("opt,epoch", [("adam", 0), ("adam", 3), ("adadelta", 0)])
def test_prioritized_loop_equals_single_steps(sd, opt, epoch):
    """the same through --prioritized_replay (B = 32): two rings with the same content and priorities, one driven by the library's loop,
    one step by step through the tuple API; the priorities written back agree too"""
    A, B, n = 4, 32, 4
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_beta_steps=1000, priority_epsilon=1e-6)
    raw = (10.0 ** np.random.RandomState(5).uniform(-2, 1, 3000)).astype(np.float32)
    mems = []
    for _ in range(2):
        m = _ring(sd, B, size=3000, **kw)
        m.set_priorities(0, raw)
        mems.append(m)
    n1, n2 = _net(sd, opt, A, B), _net(sd, opt, A, B)
    random.seed(8)
    st = random.getstate()
    n1.set_epoch(epoch)
    n1.train_from_memory(mems[0], n)
    after = random.getstate()
    random.setstate(st)
    for _ in range(n):
        n2.train(mems[1].getMinibatch(), epoch)
    assert random.getstate() == after
    _same_state(n1, n2, opt)
    assert np.array_equal(mems[0].priorities(), mems[1].priorities())


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_dp_single_rank_rccl(sd, opt, overlap):
    """test_dp_single_rank_rccl of tests/test_gpu_dqn.py for the other optimizers: with one rank the all-reduce is the identity, so the
    reduce -> all-reduce -> apply split (the second state applied in the apply pass, mode 2) reproduces the single-GPU update bit for
    bit, weights, target weights and both states, in both overlap settings, through train() and the library's loop."""
    from bench import fill_ring
    from simple_dqn_amd.deepqnetwork import dp_unique_id
    A, B = 4, 32
    n1, n2 = _net(sd, opt, A, B, seed=1271), _net(sd, opt, A, B, seed=1271)
    n2.set_option("dp_overlap", overlap)
    n2.dp_init(dp_unique_id(), 0, 1)
    for s in range(4):
        mb = random_minibatch(B, A, 1272 + s)
        n1.train(mb, s // 2)
        n2.train(mb, s // 2)
        if s % 2:
            assert np.array_equal(n1.predict(mb[0]), n2.predict(mb[0]))
        if s == 1:
            n1.update_target_network(); n2.update_target_network()
    _same_state(n1, n2, opt)
    for i in range(5):
        assert np.array_equal(n1.get_layer(i, 1), n2.get_layer(i, 1)), i
    mem = sd.ReplayMemory(3000, make_args(batch_size=B)); fill_ring(mem, 5, A)
    lib = sd.load()
    costs = []
    for n in (n1, n2):
        n.set_epoch(2)
        mt = (C.c_uint32 * 625)(); lib.sdqn_mt_seed(mt, 23)
        costs.append([n.train_from_memory(mem, 5, mt_state=mt, want_cost=True) for _ in range(2)])
    assert costs[0] == costs[1]
    _same_state(n1, n2, opt)
    n2.dp_shutdown()
    n1.train(mb, 2); n2.train(mb, 2)
    _same_state(n1, n2, opt)


@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_second_state_at_the_api(sd, opt, tmp_path):
    """which = 4 is the second optimizer state (Adam's v, Adadelta's E[dx^2]): zero in a new net, set_weights / get_layer round-trip it
    bit for bit in Neon layout, and the step uses what was set.  save_weights writes it into the .npz snapshot (keys S2<layer>, next to
    the first state's S<layer>) for adam and adadelta and load_weights restores it, so a reloaded net continues bit for bit; a Neon-style
    pickle (.prm / .pkl) carries optimizer state for rmsprop only — a net loaded from one starts Adam / Adadelta from zero states.  An
    rmsprop net has no second state: which = 4 is refused by name, for reading and for writing."""
    A, B = 4, 8
    net = _net(sd, opt, A, B)
    assert all(np.all(net.get_layer(i, 4) == 0) for i in range(5))
    rng = np.random.RandomState(1281)
    s2 = [rng.uniform(1e-9, 1e-6, net.get_layer(i, 0).shape).astype(np.float32) for i in range(5)]
    net.set_weights(s2, 4)
    for i in range(5):
        assert np.array_equal(net.get_layer(i, 4), s2[i]), i
        assert np.array_equal(net.get_layer(i, 2), np.zeros_like(s2[i])), i                # (the first state is another buffer)
    mb = random_minibatch(B, A, 1282)
    net.set_option("keep_gradients", 1)
    before = _read(net, opt)
    net.train(mb, 1)
    check_isolation(opt, before, [net.get_layer(i, 3) for i in range(5)], B, 1, _read(net, opt), "set state2, %s" % opt)
    p = str(tmp_path / "snap.npz")
    net.save_weights(p)
    with np.load(p) as f:
        assert all("S2%d" % i in f for i in range(5))
    net2 = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=opt))
    net2.load_weights(p)
    for which in (0, 1, 2, 4):
        for a, b in zip(net.get_weights(which), net2.get_weights(which)):
            assert np.array_equal(a, b)
    net.train(mb, 1); net2.train(mb, 1)
    _same_state(net, net2, opt)
    pk = str(tmp_path / "snap_1.prm")
    net.save_weights(pk)
    net3 = sd.DeepQNetwork(A, make_args(batch_size=B, optimizer=opt))
    net3.load_weights(pk)
    for i in range(5):
        assert np.array_equal(net3.get_layer(i, 0), net.get_layer(i, 0)), i
        assert np.all(net3.get_layer(i, 2) == 0) and np.all(net3.get_layer(i, 4) == 0), i
    rms = _net(sd, "rmsprop", A, B)
    with pytest.raises(Exception, match="this optimizer has no second state"):
        rms.get_layer(0, 4)
    with pytest.raises(Exception, match="this optimizer has no second state"):
        rms.set_layer(0, s2[0], 4)
    rms.save_weights(p)
    with np.load(p) as f:
        assert "S0" in f and "S20" not in f
