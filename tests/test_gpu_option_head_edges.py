"""--munchausen, --advantage_learning / --persistent_advantage and --bootstrap_heads at the edges tests/test_gpu_head_edges.py (the
action-count buckets A <= 4, <= 8, <= 18) and tests/test_gpu_batch_edges.py (every dispatch edge in the batch size) map for the standard
head.  Everything is built from the helpers of tests/test_gpu_munchausen.py (TM), tests/test_gpu_advantage_learning.py (TA),
tests/test_gpu_bootstrap.py (TB), tests/test_gpu_nstep.py (TN) and tests/test_gpu_batch_edges.py (TE), which take this file's configurations
themselves (_Cfg) where they take a name of their own tables.  Every bound
is the one the existing one-step test of the same datatype and regime uses (cited where it is taken); the reference of a float32 net is
the float64 oracle (TA's docstring gives the reason), of a float16 net the half oracle.

  A. head instantiations.  munchausen_head_kernel / advantage_head_kernel<AMAX, PER, NSTEP> at AMAX = 8 (A = 5, 8) and 18 (A = 9, 18)
     with n_step 3, prioritized replay and both (PAL: prioritized replay only), float16 composed with both, the generic path's head code
     composed with both — TM / TA's _composed (three teacher-forced ring steps, B = 8).  bootstrap_head_kernel at 5, 2, 9, 18, 18 rows
     ((K, A) = (5, 1), (2, 1), (3, 3), (2, 9), (9, 2)), with n_step 3 and with masks drawn at P = 0.5.
  B. the extra forward (run_extra_forward: qbar(s) into q slot 2) at a batch size of every regime: one step against the oracle at float32 B = 33, 65,
     127, 129, 257 and float16 B = 33, 48, 127, 257, and TE's position invariance at float32 129 / 257 and float16 257 — a slot-2 row read
     at another sample's n moves that sample's target by alpha x gap, which the permuted twin does not reproduce.
  C. train_from_memory with the extra forward against the tuple API above B = 32, bit for bit.

CPU-side facts behind the constants (numpy oracles, this file's seeds):
  * part A, TM / TA's 600-slot ring, sampling seed 17 (AL with n_step alone: TA._ring_seed's walk also stops at 17), B = 8: terminals per
    minibatch, steps 1 / 2 / 3 — n_step 3: 3 / 1 / 0; prioritized: 3 / 0 / 0; both: 2 / 1 / 0, the same for every A of 5, 8, 9, 18 and for
    Munchausen, AL and PAL (the indexes do not depend on A; the prioritized rows are simulated with the oracle's priorities).  No cell needed
    a larger B for its terminal.  float16 B = 32: Munchausen both 7 / 4 / 3 (A = 4), 7 / 6 / 5 (A = 9); PAL prioritized 2 / 1 / 1.
    f64_b8: 2 / 1 / 0 (PAL 3 / 0 / 0); f32_generic (B = 7): 1 / 1 / 0 (PAL 0 / 1 / 0).  Smallest |fc4 pre-activation| over the three steps of a
    cell: 1.2e-6 at the least (TA._ring_seed asks for 1e-6).
  * part A, bootstrap: TB's 300-slot ring, mask seed 123 (make_args' random_seed), P = 0.5 — the batch seeds SEED_MASK give, of 32 samples,
    (K, A) = (3, 3): 1 with every head masked and 8 with every head live; (2, 9): 3 / 11 (asserted again before the device
    runs); the n_step 3 batches (seed 7, TB.test_n_step_3's) hold terminals and non-terminals.
  * part B: the walk over Xavier seeds (TM / TA's _discriminates on the oracle alone; float32 below B = 128 also MARGINS) starts at SEEDS,
    found on the CPU, so a cell costs one oracle pass: 11, but Munchausen float16 B = 127 12 and float32 B = 33 / 65 13 / 27 (smallest
    |pre-activation| per layer there 2.8e-6, 2.0e-6, 3.0e-6, 9.1e-6 / 3.4e-6, 1.9e-6, 1.2e-6, 5.5e-5; of seeds 11 .. 71 ten clear MARGINS at
    B = 33, of 11 .. 37 one at B = 65).  At B = 127 none of 11 .. 199 does: every seed whose smallest pre-activation exceeds 5e-7 has a
    conv1 unit below 2e-6 (the best, 107: 8.1e-7).  With seed 11 throughout, terminals in the
    minibatches: B = 33: 2, 48: 4, 65: 3, 127: 8, 129: 13, 257: 23 (A = 6) / 14 (A = 3); Munchausen's bonus is clipped on 27 of 33, 45 of 65,
    116 of 127, 92 of 129, 208 of 257 samples (float16: 27 / 33, 41 / 48, 115 / 127, 168 / 257); PAL takes the poststate's gap on 12, 16, 57,
    40, 86 samples (float16: 12, 20, 57, 85) and has 5, 18, 9, 37, 44 (float16: 5, 6, 9, 83) gaps of exactly zero.  The bootstrap
    tuples (TB._random_minibatch, seed 100) hold 1 / 2 / 16 terminals at B = 33 / 127 / 257.
  * the ill-conditioned reference (float32 B = 65 and 127 with seed 11).  The float64 oracle holds a conv3 unit (sample 58, position 37,
    channel 12) at -2.6e-8.  Forcing that one gate the other way in the oracle moves the conv1 / conv2 / conv3 gradients by 3.65e-3 /
    4.41e-3 / 1.94e-2 (largest element; 5.459e-3 of conv1's norm with PAL at B = 65) and fc4 / fc5 not at all; forcing the conv1 unit
    nearest zero (sample 45, position 189, channel 27, +8.4e-7) moves conv1 by 5.44e-3 (3.63e-3 of its norm) and nothing else.  The MI355X
    step stood 3.648e-3 (largest element) and 5.459e-3 (norm, PAL) from the oracle in conv1, where the comparison stops: the conv3 flip to
    four digits, not the conv1 one.  B = 33 (without sample 58) stood 2.2e-7, B = 129 / 257 (with it, on the other kernels) 4.1e-7 / 5.9e-7.
    Hence MARGINS.  The two float32 B = 127 cells keep seed 11: Q, V / max-Q and the fc4 / fc5 gradients are held to the oracle as every
    cell's, the conv gradients to the oracle with that one gate forced (predicted difference to the oracle as it stands at B = 127, conv1:
    3.652e-3 / 2.749e-3 largest element, 3.108e-3 / 2.149e-3 of the norm for Munchausen / PAL — the figures the step showed), and the
    comparison of the conv gradients with the oracle as it stands ends as an expected failure (test_conv_gradients_b127).
  * reorder noise: none had to be measured — every configuration of part B stays within TE.P_BOUND (see test_position_invariance).
"""
import random

import numpy as np
import pytest

import bootstrap_oracle as BO
import test_gpu_advantage_learning as TA
import test_gpu_batch_edges as TE
import test_gpu_bootstrap as TB
import test_gpu_munchausen as TM
import test_gpu_nstep as TN
from oracle.dqn_numpy import CONV, _im2col, xavier_weights
from test_gpu_double_dqn import _minibatch
from util import make_args

pytestmark = pytest.mark.gpu

CFG = TM.CONFIGS                                             # (TA.CONFIGS is the same table)
G84 = (4, 84, 84)
F16 = dict(datatype="float16")


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


class _Cfg(tuple):
    """a configuration of TM.CONFIGS' form (TB.REGIMES' for bootstrap) that prints as its label: the helpers of TM, TA, TN and TB take
    it in the place of a name of their tables"""
    def __new__(cls, label, cfg):
        self = super().__new__(cls, cfg)
        self.label = label
        return self

    def __str__(self):
        return self.label

    __repr__ = __str__


def _half(name):
    return TM._cfg(name)[3].get("datatype") == "float16"


# ---- part A ---------------------------------------------------------------------------------------------------------------------------
MODES = {"nstep": (3, False), "per": (1, True), "both": (3, True)}
BUCKET_EDGES = [5, 8, 9, 18]                                 # first and last action count of AMAX = 8 and of AMAX = 18
# float32 B = 8: the bounds of fp32_b32 (TM.CONFIGS; its a5_b3 takes the same); float16 A = 9: those of fp16_b32
A_B8 = {_A: _Cfg("a%d_b8" % _A, (_A, 8, G84, {}) + CFG["fp32_b32"][4:]) for _A in BUCKET_EDGES}
FP16_B32 = ["fp16_b32", _Cfg("fp16_a9_b32", (9, 32, G84, F16) + CFG["fp16_b32"][4:])]
GENERIC = ["f64_b8", _Cfg("f32_generic", CFG["f32_generic"])]      # (TN's table has no ring of the second geometry: passed as itself)
assert TN.CONFIGS["fp16_b32"] == CFG["fp16_b32"] and TN.CONFIGS["f64_b8"] == CFG["f64_b8"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("A", BUCKET_EDGES)
def test_munchausen_head_instantiations(sd, A, mode):
    """munchausen_head_kernel<8 / 18, PER, NSTEP>: Q(pre), the soft value, five gradients, priorities, as TM._composed holds <4, ., .>"""
    n, per = MODES[mode]
    TM._composed(sd, n, per, name=A_B8[A], dtype=np.float64)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("A", BUCKET_EDGES)
def test_advantage_head_instantiations(sd, A, mode):
    n, per = MODES[mode]
    TA._composed(sd, n, per, False, name=A_B8[A])


@pytest.mark.parametrize("A", BUCKET_EDGES)
def test_persistent_advantage_head_instantiations(sd, A):
    TA._composed(sd, 1, True, True, name=A_B8[A])


def test_persistent_advantage_refuses_n_step_at_a9(sd):
    kw = dict(batch_size=8, advantage_learning=TA.ALPHA, persistent_advantage=True)
    with pytest.raises(ValueError, match=r"--persistent_advantage cannot be combined with --n_step 3 \(--advantage_learning alone can\)"):
        sd.DeepQNetwork(9, make_args(n_step=3, **kw))
    net = sd.DeepQNetwork(9, make_args(**kw))
    with pytest.raises(Exception, match=r"n_step 3 cannot be combined with persistent_advantage: it repeats the action in the NEXT state"):
        net.set_option("n_step", 3)                          # the library's own refusal
    assert net.train_iterations == 0


@pytest.mark.parametrize("name", FP16_B32, ids=str)
@pytest.mark.parametrize("opt", ["munchausen", "pal"])
def test_float16_composed(sd, opt, name):
    """the half h_d4 store through loss_scale with the importance weight in front of it, at the float16 bounds of TM.CONFIGS"""
    if opt == "munchausen":
        TM._composed(sd, 3, True, name=name)
    else:
        TA._composed(sd, 1, True, True, name=name)


@pytest.mark.parametrize("name", GENERIC, ids=str)
@pytest.mark.parametrize("opt", ["munchausen", "al", "pal"])
def test_generic_path_composed(sd, opt, name):
    """generic_net.hip's own head code with n_step 3 and prioritized replay (PAL: prioritized replay) at TM.CONFIGS' bounds: float64 1e-9 on
    Q, 1e-11 relative on every gradient"""
    if opt == "munchausen":
        TM._composed(sd, 3, True, name=name, dtype=np.float64)
    else:
        TA._composed(sd, 1 if opt == "pal" else 3, True, opt == "pal", name=name)


@pytest.mark.parametrize("K,A", [(5, 1), (2, 1), (3, 3), (2, 9), (9, 2)])
def test_bootstrap_rows(sd, K, A):
    """5, 2, 9, 18, 18 rows: the first row count of buckets 1 and 2, and A = 1, where the per-head max loop runs zero times"""
    TB.test_one_step_parity(sd, "fp32_b32", A, K)


SEED_MASK = {(3, 3): 6, (2, 9): 6}                           # batch seeds of the P = 0.5 cells (module docstring)


def _boot_step(sd, regime, K, A, n=1, P=1.0):
    B, half = TB._regime(regime)[0], TB._regime(regime)[2].get("datatype") == "float16"
    net, o, mem, om, valid = TB._setup(sd, regime, A, K, n=n, **(dict(bootstrap_mask_probability=P) if P < 1 else {}))
    net.set_option("keep_gradients", 1)
    idx, mb = TB._batch(om, valid, B, SEED_MASK[(K, A)] if P < 1 else 7, n=n)
    if n > 1:
        assert np.asarray(mb[4]).any() and not np.asarray(mb[4]).all()
    if P < 1:                                                # chosen on the CPU: a sample with every head masked, one with every head live
        live = np.stack([BO.mask(o.mask_seed, P, K, i) for i in idx]).sum(axis=1)
        dead = np.nonzero(live == 0)[0]
        assert len(dead) > 0 and (live == K).any(), live
    o.indexes = idx
    g, cost_ref, deltas, preq = o.gradients(mb)
    cost = net.train_indexes(mem, idx, want_cost=True)
    if P < 1:                                                # TB.test_masks' assertions
        assert np.array_equal(o.last_masks.sum(axis=1), live)
        dq = net.debug_read("dq", B * K * A).reshape(B, K * A)
        terms = net.debug_read("cost_terms", B)
        want = np.zeros((B, K * A), bool)
        for i in range(B):
            for k in range(K):
                want[i, k * A + int(mb[1][i])] = bool(o.last_masks[i, k])
        assert np.array_equal(dq != 0, want & (deltas != 0)) and (want & (deltas != 0)).sum() > B
        assert not dq[dead].any() and not terms[dead].any()
        if not half:
            assert np.abs(dq - deltas).max() < 1e-4
            d4 = net.debug_read("d4", B * 512).reshape(B, 512)
            assert not d4[dead].any()
            assert np.abs(d4).max() > 0 and np.abs(d4 - o.last_d4).max() < 1e-4 * max(1.0, np.abs(o.last_d4).max())
            assert np.abs(terms - o.last_cost_terms).max() < 1e-3 * max(1.0, float(o.last_cost_terms.max()))
    TB._check_step(net, o, regime, g, cost_ref, preq, cost)


@pytest.mark.parametrize("regime,K,A", [("fp32_b32", 3, 3), ("fp32_b32", 2, 9), ("fp16_b32", 2, 9)])
def test_bootstrap_rows_n_step_3(sd, regime, K, A):
    _boot_step(sd, regime, K, A, n=3)


@pytest.mark.parametrize("regime,K,A", [("fp32_b32", 3, 3), ("fp32_b32", 2, 9), ("fp16_b32", 3, 3)])
def test_bootstrap_rows_masked(sd, regime, K, A):
    _boot_step(sd, regime, K, A, P=0.5)


@pytest.mark.parametrize("K,A,prefer", [(18, 1, [0] * 18), (2, 9, [7, 4])])
def test_bootstrap_acting_rule(sd, K, A, prefer):
    """The vote and the per-episode head at 18 rows.  evaluate() and collect() cannot run here — every device game has three actions, and
    a net of another action count is refused by name (asserted) — so the rule is held through the single-environment path, as
    TB.test_single_environment_acting does: the vote's tie goes to the lowest action (TB.test_evaluate_votes_and_breaks_ties_low), while
    collecting the episode's head decides, the library's counter and Python's agree, and both equal tests/bootstrap_oracle.py's."""
    seed = 9
    args = TB._cargs(bootstrap_heads=K, random_seed=seed)
    net = sd.DeepQNetwork(A, args)
    TB._disagreeing_heads(net, K, A, prefer)
    buf = sd.DeviceStateBuffer(args)
    rng = np.random.RandomState(1)
    for _ in range(4):
        buf.add(rng.randint(1, 256, (84, 84), dtype=np.uint8))
    raw = net.predict_state(buf)
    assert raw.shape == (K * A,) and raw.max() > 0
    assert [int(np.argmax(BO.head_slice(raw, K, A, k))) for k in range(K)] == prefer
    net.set_acting(True)
    action, counts = BO.vote(raw, K, A)
    assert action == min(prefer) and counts[action] == prefer.count(action)           # (2, 9): one vote each, the tie goes low
    assert net.act_greedy(buf) == action == net.acting_action(raw)
    net.set_acting(False)
    net.next_episode(reset=True)
    seen = set()
    for ep in range(8):
        k = BO.head_of(seed, K, 0, ep)
        seen.add(k)
        assert net.act_greedy(buf) == prefer[k] == net.acting_action(raw), ep
        net.next_episode()
    assert len(seen) >= 2
    with pytest.raises(Exception, match=r"the network has \d+ actions"):
        net.evaluate(sd.CatchEnvironment(args, seed=1), 4, 5, epsilon=0.0, seed=5)


# ---- part B ---------------------------------------------------------------------------------------------------------------------------
PART_B = {}
for _B, _A in ((33, 3), (65, 6), (127, 18), (129, 3), (257, 6)):   # TM.CONFIGS' fp32_b32 / fp32_b128 bounds (every float32 regime: 1e-4)
    PART_B["fp32_b%d" % _B] = _Cfg("fp32_b%d" % _B, (_A, _B, G84, {}) + CFG["fp32_b128" if _B >= 128 else "fp32_b32"][4:])
for _B, _A in ((33, 3), (48, 6), (127, 18), (257, 3)):              # TM.CONFIGS' fp16_b32 / fp16_b128 bounds (3e-3)
    PART_B["fp16_b%d" % _B] = _Cfg("fp16_b%d" % _B, (_A, _B, G84, F16) + CFG["fp16_b128" if _B >= 128 else "fp16_b32"][4:])
PART_B_INVARIANCE = ["fp32_b129", "fp32_b257", "fp16_b257"]
# (option, name): where the walk over Xavier seeds starts (module docstring); 11 otherwise
SEEDS = {("munchausen", "fp16_b127"): 12}
for _opt in ("munchausen", "pal"):
    SEEDS.update({(_opt, "fp32_b33"): 13, (_opt, "fp32_b65"): 27})
# float32 below B = 128 is held to an element bound, and a Rectlin unit whose pre-activation lies within float32 rounding of zero is gated
# by summation order, its whole delta coming or going with it (TA._ring_seed).  Those cells ask for a reference that
# decides every gate clear of that rounding, per layer (conv1, conv2, conv3, fc4): the largest |float32 - float64| pre-activation of the
# numpy oracle itself on these minibatches (seeds 11 .. 18: 1.89e-6, 1.09e-6, 8.6e-7, 5.5e-7), rounded up.
MARGINS = (2e-6, 1.2e-6, 1e-6, 6e-7)
# B = 127 (2.7e6 units): no seed of 11 .. 199 reaches MARGINS (module docstring).  Its float32 cells keep seed 11, whose reference decides
# one conv3 gate by rounding: Q, V / max-Q and the fc4 / fc5 gradients, which that gate does not reach, are held like every other cell's;
# the conv gradients are held in test_conv_gradients_b127
ILL_CONDITIONED = ("the float64 reference of seed 11 holds a conv3 unit (sample 58, position 37, channel 12) 2.6e-8 from zero, which the "
                   "float32 step gates the other way: conv1 / conv2 / conv3 gradients move by 4.5e-3 / 5.3e-3 / 2.4e-2 of their largest "
                   "element; no seed of 11 .. 199 gives a reference clear of float32 rounding at B = 127")
PART_B_CELLS = [(opt, name) for opt in ("munchausen", "pal") for name in PART_B]


def _opt_oracle(opt, name, ws, wt):
    if opt == "munchausen":
        return TM._oracle(name, ws, wt, dtype=None if _half(name) else np.float64)
    return TA._oracle(name, ws, wt, True)


def _opt_net(sd, opt, name, ws, wt):
    net = TM._net(sd, name, ws, wt) if opt == "munchausen" else TA._net(sd, name, ws, wt, True)
    net.set_option("keep_gradients", 1)
    return net


def _weights(name, s):
    A, _, geom, _, _, _ = TM._cfg(name)
    return xavier_weights(A, s, np.float32, *geom), xavier_weights(A, s + 100, np.float32, *geom)


def _margins(o, mb):
    """smallest |pre-activation| of the Rectlin of each layer (conv1, conv2, conv3, fc4) of the online net on mb's prestates"""
    a = o._normalize(mb[0])
    out = []
    for li, (R, S, K, st) in enumerate(CONV):
        z = _im2col(a, R, S, st)[0] @ o.W[li]
        out.append(float(np.abs(z).min()))
        a = np.ascontiguousarray(np.maximum(z, 0).transpose(0, 2, 1)).reshape(a.shape[0], K, *_out_hw(a, R, S, st))
    return out + [TA._fc4_margin(o, mb)]


def _out_hw(a, R, S, st):
    return (a.shape[2] - R) // st + 1, (a.shape[3] - S) // st + 1


def _cell(opt, key):
    """(seed, minibatch, weights, oracle after its gradient pass, gradients, Q(pre)) of the first draw on which the minibatch discriminates
    and (float32 below B = 128) the reference clears MARGINS — the walk of TM / TA's _setup, begun at the seed found on the CPU"""
    name = PART_B[key]
    A, B, geom, kw, tol, _ = name
    mb = _minibatch(B, A, geom, 5)
    start = SEEDS.get((opt, key), 11)
    for s in range(start, start + 20):
        ws, wt = _weights(name, s)
        o = _opt_oracle(opt, name, ws, wt)
        g, _, _, preq = o.gradients(mb)
        ok = TM._discriminates(o, mb, max(tol, 1e-6)) if opt == "munchausen" else TA._discriminates(o, mb, max(tol, 1e-6), True, B)
        if ok and not _half(name) and B < 128 and key != "fp32_b127":
            ok = all(m > least for m, least in zip(_margins(o, mb), MARGINS))
        if ok:
            return s, mb, ws, wt, o, g, preq
    pytest.fail("no pair of draws on which the targets discriminate")


def _device_step(sd, opt, key):
    s, mb, ws, wt, o, g, preq = _cell(opt, key)
    print("%s %s: discriminates at seed %d" % (opt, PART_B[key], s))
    net = _opt_net(sd, opt, PART_B[key], ws, wt)
    net.train(mb)
    return net, mb, ws, wt, o, g, preq


@pytest.mark.parametrize("opt,key", PART_B_CELLS)
def test_extra_forward_one_step(sd, opt, key):
    """One whole step at a batch size of each regime: Q(pre), V or max-Q (TM / TA's _check_q) and the five gradients under the regime's
    rule in TM._check_grads.  float32 B = 127: the fc4 and fc5 gradients here — they carry every sample's target and delta, and the one
    gate its reference decides by rounding lies below them — and the three conv gradients in test_conv_gradients_b127."""
    name = PART_B[key]
    net, mb, ws, wt, o, g, preq = _device_step(sd, opt, key)
    if opt == "munchausen":
        TM._check_q(net, o, preq, name[4])
    else:
        TA._check_q(net, preq, o.last_post_target_q.max(1), name[4])
    TM._check_grads(net, name, g, layers=(3, 4) if key == "fp32_b127" else range(5))


def _nearest_unit(o, mb, li):
    """(sample, channel, position, pre-activation) of the Rectlin unit of conv layer li of the online net that stands nearest zero"""
    a = o._normalize(mb[0])
    for l, (R, S, K, st) in enumerate(CONV):
        z = _im2col(a, R, S, st)[0] @ o.W[l]
        if l == li:
            n, pos, k = np.unravel_index(np.abs(z).argmin(), z.shape)
            return int(n), int(k), int(pos), float(z[n, pos, k])
        a = np.ascontiguousarray(np.maximum(z, 0).transpose(0, 2, 1)).reshape(a.shape[0], K, *_out_hw(a, R, S, st))


def _gradients_with_gate_forced(opt, name, ws, wt, mb, li, unit):
    """the oracle's gradients with the gate of one unit of conv layer li decided the other way (its activation, |z| < 1e-6, moves by less
    than that; its delta comes or goes whole)"""
    o = _opt_oracle(opt, name, ws, wt)
    fprop = o.fprop
    n, k, pos, _ = unit

    def forced(W, x, keep=False):
        r = fprop(W, x, keep=keep)
        if keep:                                             # (the online net on the prestates: the pass whose gates the backward reads)
            v = r[1][0][li + 1][n].reshape(r[1][0][li + 1].shape[1], -1)
            v[k, pos] = 0.0 if v[k, pos] > 0 else 1e-30
        return r
    o.fprop = forced
    return o.gradients(mb)[0]


@pytest.mark.parametrize("opt", ["munchausen", "pal"])
def test_conv_gradients_b127(sd, opt):
    """float32 B = 127, the three conv gradients.  The float64 reference of seed 11 holds one conv3 unit 2.6e-8 from zero — 40 times
    nearer than float32 rounding of that sum (MARGINS) — and no seed of 11 .. 199 gives a reference without such a unit.  Held here without
    a mark: the step's conv gradients equal, within the element bound, the oracle's with that ONE gate decided the other way.  Then
    the comparison with the oracle as it stands, which the step is expected to miss by exactly that flip (conv1 3.65e-3 of 1.0): the
    test ends as an expected failure with the cause, or passes if a later kernel rounds that sum to the oracle's side."""
    key = "fp32_b127"
    name = PART_B[key]
    net, mb, ws, wt, o, g, _ = _device_step(sd, opt, key)
    unit = _nearest_unit(o, mb, 2)
    assert unit[:3] == (58, 12, 37) and abs(unit[3]) < 0.04 * MARGINS[2], unit
    TM._check_grads(net, name, _gradients_with_gate_forced(opt, name, ws, wt, mb, 2, unit), layers=(0, 1, 2))
    try:
        TM._check_grads(net, name, g, layers=(0, 1, 2))
    except AssertionError:
        pytest.xfail(ILL_CONDITIONED)


# TB.REGIMES' form, the bounds of the regime in TM.CONFIGS
BOOT_B = [_Cfg(k, (PART_B[k][1], G84, PART_B[k][3]) + PART_B[k][4:]) for k in ("fp32_b33", "fp32_b127", "fp32_b257", "fp16_b127")]


@pytest.mark.parametrize("regime", BOOT_B, ids=str)
def test_bootstrap_one_step_through_train(sd, regime):
    """(K, A) = (3, 6) fed as TB.test_three_free_running_steps feeds float32 B = 128: uniform-pixel tuples through train(), mask
    probability 1; one step, TB._check_step's comparisons against the float64 oracle (float16: the half oracle)"""
    K, A = 3, 6
    B, geom, kw = regime[:3]
    net, o, _, _, _ = TB._setup(sd, regime, A, K)
    if not kw:
        o64 = BO.BootstrapOracle(A, K, batch_size=B, dtype=np.float64, weights=[w.astype(np.float64) for w in o.W])
        o64.Wt = [w.astype(np.float64) for w in o.Wt]
        o = o64
    net.set_option("keep_gradients", 1)
    mb = TB._random_minibatch(B, A, geom, 100)
    assert mb[4].any() and not mb[4].all()
    g, cost_ref, _, preq = o.gradients(mb)
    net.callback = type("CB", (), dict(on_train=lambda self, c: setattr(self, "cost", c)))()
    net.train(mb)
    TB._check_step(net, o, regime, g, cost_ref, preq, net.callback.cost)


def _perms(key):
    """roll by one and a fixed random permutation; B = 257: TE's, repaired so that every sample past 256 lands below 256"""
    B = PART_B[key][1]
    if key in TE.CONFIGS:
        assert TE.CONFIGS[key][1] == B
        return TE._perms(key)
    return {"roll": np.roll(np.arange(B), 1), "perm": np.random.RandomState(1000 + B).permutation(B)}


@pytest.mark.parametrize("key", PART_B_INVARIANCE)
@pytest.mark.parametrize("opt", ["munchausen", "pal"])
def test_position_invariance(sd, opt, key):
    """Instrument 2 of tests/test_gpu_batch_edges.py on the steps with the extra forward: the same minibatch rolled by one and permuted
    gives the permuted Q rows and V / max-Q values (1e-6 of the largest, TE._invariance's bound) and every layer's gradient within
    TE.P_BOUND in relative norm.  The extra term is per sample and computed by one thread in double: it adds no reorder noise, and a slot-2
    row read at another n would move a layer's gradient by ~ 1 / sqrt(B) of its norm (TE's reasoning), 6e-2 here.  The draw is _cell's:
    both branches of PAL's max, clipped and unclipped Munchausen bonuses are in the minibatch."""
    name = PART_B[key]
    _, mb, ws, wt, _, _, _ = _cell(opt, key)
    out = {}
    for which, perm in [("base", None)] + list(_perms(key).items()):
        net = _opt_net(sd, opt, name, ws, wt)
        net.train(mb if perm is None else tuple(np.ascontiguousarray(x[perm]) for x in mb))
        q, mq = net.last_q()
        out[which] = (q, mq, [np.array(net.get_layer(i, 3)) for i in range(5)], perm)
    q, mq, g, _ = out["base"]
    bound = TE.P_BOUND["float16" if _half(name) else "float32"]
    for which in ("roll", "perm"):
        qp, mqp, gp, perm = out[which]
        assert np.abs(qp - q[perm]).max() <= 1e-6 * max(1.0, float(np.abs(q).max()))
        assert np.abs(mqp - mq[perm]).max() <= 1e-6 * max(1.0, float(np.abs(mq).max()))
        rels = [TE._rel(gp[i], g[i]) for i in range(5)]
        print("%s %s %s: Q rows bit-identical: %s; gradient rel norm of the difference per layer %s (P = %.3e)" % (
            opt, name, which, bool(np.array_equal(qp, q[perm])), " ".join("%.3e" % r for r in rels), bound))
        for i in range(5):
            assert rels[i] < bound, (which, i, rels[i])


# ---- part C ---------------------------------------------------------------------------------------------------------------------------
OPT_KW = {"munchausen": TM.MU, "pal": TA._kw(True)}


PART_C = [(opt, dt, B, 1) for opt in OPT_KW for dt, B in (("float32", 33), ("float32", 129), ("float32", 257), ("float16", 48), ("float16", 257))]
PART_C.append(("munchausen", "float32", 129, 3))             # (the persistent form is refused with n_step: part A asserts it)


@pytest.mark.parametrize("opt,dt,B,n", PART_C)
def test_fused_loop_equals_tuple_api(sd, opt, dt, B, n):
    """TM / TA.test_fused_loop_equals_tuple_api above B = 32 on TE's 5000-slot ring: three times one train(getMinibatch()) against one
    train_from_memory(mem, 1), then train_from_memory(mem, 4) against four tuple steps — the weights bit-identical, as
    TE.test_train_from_ring_equals_tuple_api holds the standard step at B = 257 (it compares bits too); a standard net on the same fused
    loop ends elsewhere."""
    A = 4
    mem, _ = TE._mems(sd, dt, B, n, A=A)
    ws, wt = xavier_weights(A, 61), xavier_weights(A, 161)
    nets = []
    for k in range(3):
        net = sd.DeepQNetwork(A, make_args(batch_size=B, datatype=dt, n_step=n, **(OPT_KW[opt] if k < 2 else {})))
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        nets.append(net)
    n1, n2, n3 = nets
    assert n1.munchausen if opt == "munchausen" else n1.persistent_advantage
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
    for i, (a, b) in enumerate(zip(TM._layers(n1), TM._layers(n2))):
        assert np.array_equal(a, b), i
    random.seed(6)                                           # and the option is honoured on the fused loop: a standard net moves elsewhere
    n3.train_from_memory(mem, 3)
    n3.train_from_memory(mem, 4)
    assert np.isfinite(n1.get_layer(4)).all() and not np.array_equal(n1.get_layer(4), n3.get_layer(4))


def test_prioritized_replay_refuses_batch_257_with_munchausen(sd):
    """TE.test_prioritized_replay_refuses_batch_257's refusal holds with the option set"""
    kw = dict(TM.MU, **TN._per_kw())
    with pytest.raises(Exception, match=r"batch sizes up to 256 \(got 257\)"):
        sd.ReplayMemory(600, make_args(batch_size=257, **kw))
    assert sd.ReplayMemory(600, make_args(batch_size=256, **kw)).prioritized
