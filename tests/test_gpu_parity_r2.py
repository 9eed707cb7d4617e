"""Round-2 parity additions (VERDICT r1 "next round" item 1): the BASELINE.json configs that round 1 only touched at
other shapes — fp16 at A=6 (configs[4]), B=256 at A=6 and in the fused train_from_memory loop (configs[2]) — and the
data-parallel arithmetic on ONE GPU in a form that is not the identity (two learners' gradient sums added on the host,
applied through the library's apply-only update with divisor 2B, against the oracle on the concatenated batch).
Tolerances are stated next to each assert; fp32 Q-values are held to BASELINE.json's 1e-4."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.dqn_numpy import OracleDQN, xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu
Q_TOL = 1e-4
H_TOL = 3e-3          # fp16 mode vs its own (half-rounding) oracle: a few half ulps through 5 layers


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _net(sd, A, B, seed, **kw):
    args = make_args(batch_size=B, **kw)
    net = sd.DeepQNetwork(A, args)
    ws, wt = xavier_weights(A, seed), xavier_weights(A, seed + 1)
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    return net, ws, wt


# ---- configs[4]: float16 activations at A = 6, B = 32 ---------------------------------------------------------------
def _rel_fro(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(1e-12, np.linalg.norm(b.ravel())))



def _fp64_yardstick(A, B, ws, wt, mb, g_hip, g_half_oracle, what):
    """the float16 semantics are the builder's own, so 'HIP == half oracle within X' is self-referential.
    The yardstick that is not: the SAME step in fp64 (no half rounding anywhere).  Per layer, the HIP gradient must be no
    further from the fp64 gradient than 1.5 x the half oracle's own distance (Frobenius norm) — 'not worse than the
    restatement's own half error', the form of the 100-step chaos budget in tests/test_gpu_dqn.py."""
    o64 = OracleDQN(A, batch_size=B, weights=[w.astype(np.float64) for w in ws], dtype=np.float64)
    o64.Wt = [w.astype(np.float64) for w in wt]
    g64, _, _, _ = o64.gradients(mb)
    for i in range(5):
        e_hip = float(np.linalg.norm((g_hip[i] - g64[i]).ravel()))
        e_or = float(np.linalg.norm((g_half_oracle[i] - g64[i]).ravel()))
        n64 = float(np.linalg.norm(g64[i].ravel()))
        print("%s layer %d: |g_hip - g_fp64| = %.3e, |g_half_oracle - g_fp64| = %.3e (ratio %.2f), |g_fp64| = %.3e"
              % (what, i, e_hip, e_or, e_hip / max(e_or, 1e-30), n64))
        assert e_hip <= 1.5 * e_or + 1e-6 * n64, (what, i, e_hip, e_or)


def test_fp16_a6_one_step_and_five_step_tracking(sd):
    """configs[4] shape (A = 6, B = 32).  Two different kinds of check, because half precision makes ReLU-gate flips
    (a pre-activation within half round-off of 0 gates the delta in one implementation and not in the other) ~1000x more
    frequent than in fp32, and one flipped fc4 unit moves a whole gradient row by O(|W5 delta|):
      * kernel correctness, strict: the packed-fp16-MFMA weight gradients (gemm_tile_hw) against the round-1 routine (fp32
        MFMA on the same half operands) — identical inputs, both accumulate exact products in fp32: <= 1e-5 of max|g|
        (conv1: 1e-3, its input is now half(x/255) like the forward pass instead of fp32 x/255);
      * precision contract vs the half oracle: Q and cost at half round-off, gradients in relative Frobenius norm < 5e-2
        (max-norm errors of single rows are seed-dependent: 4e-4 ... 1.6e-1 measured over seeds, old and new routine alike)."""
    A, B = 6, 32
    mb = random_minibatch(B, A, 612, reward_range=(-2, 3))
    grads = {}
    for mode in (0, 1):
        net, ws, wt = _net(sd, A, B, 611, datatype="float16")
        net.set_option("keep_gradients", 1)
        net.set_option("h16_wgrad_mfma", mode)
        costs = []
        net.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
        net.train(mb)
        grads[mode] = [net.get_layer(i, which=3) for i in range(5)]
        q, _ = net.last_q()
    o = OracleDQN(A, batch_size=B, weights=ws, half_activations=True)
    o.Wt = [w.copy() for w in wt]
    g, cost, _, preq = o.gradients(mb)
    assert np.abs(q - preq).max() < H_TOL
    assert abs(costs[0] - float(cost)) < 5e-3 * max(1.0, float(cost))
    for i in range(5):
        sc = max(1e-6, np.abs(g[i]).max())
        d = np.abs(grads[1][i] - grads[0][i]).max() / sc
        print("fp16 A=6 grad layer %d: f16-MFMA vs fp32-MFMA routine %.2e of max|g|; vs half oracle: rel Frobenius %.2e, max %.2e"
              % (i, d, _rel_fro(grads[1][i], g[i]), np.abs(grads[1][i] - g[i]).max() / sc))
        assert d < (1e-3 if i == 0 else 1e-5), i
        assert _rel_fro(grads[1][i], g[i]) < 5e-2, i
    _fp64_yardstick(A, B, ws, wt, mb, grads[1], g, "fp16 A=6 B=32")
    # 5 free-running steps (fused fc4 update) against the half oracle; fused == unfused bit for bit
    n1, _, _ = _net(sd, A, B, 621, datatype="float16")
    n2, ws2, wt2 = _net(sd, A, B, 621, datatype="float16")
    n2.set_option("keep_gradients", 1)
    o2 = OracleDQN(A, batch_size=B, weights=ws2, half_activations=True)
    o2.Wt = [w.copy() for w in wt2]
    hold = random_minibatch(B, A, 622)[0]
    for s in range(5):
        mb = random_minibatch(B, A, 623 + s, p_term=0.05, reward_range=(-1, 2))
        n1.train(mb); n2.train(mb); o2.train(mb)
    q1, q2, qo = n1.predict(hold), n2.predict(hold), o2.predict(hold)
    print("fp16 A=6, 5 steps: Q max abs err vs half oracle %.3e (|Q| max %.2f)" % (np.abs(q1 - qo).max(), np.abs(qo).max()))
    assert np.array_equal(q1, q2)
    assert np.abs(q1 - qo).max() < 5e-2                        # 5 free-running steps of a half-precision net (measured 1.4e-2 ... 2.7e-2)


def test_fp16_batch256_one_step(sd):
    """float16 mode in the throughput regime (B = 256: other waves-per-tile choices for conv1 / conv3 / fc4 forward, 8-wave
    K-split packed-fp16 weight gradients): Q and cost vs the half oracle, gradients in relative Frobenius norm, and the
    packed-fp16 wgrad routine against the fp32-MFMA one on the same half operands."""
    A, B = 3, 256
    mb = random_minibatch(B, A, 732, reward_range=(-2, 3))
    grads = {}
    for mode in (0, 1):
        net, ws, wt = _net(sd, A, B, 731, datatype="float16")
        net.set_option("keep_gradients", 1)
        net.set_option("h16_wgrad_mfma", mode)
        costs = []
        net.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
        net.train(mb)
        grads[mode] = [net.get_layer(i, which=3) for i in range(5)]
        q, _ = net.last_q()
    o = OracleDQN(A, batch_size=B, weights=ws, half_activations=True)
    o.Wt = [w.copy() for w in wt]
    g, cost, _, preq = o.gradients(mb)
    assert np.abs(q - preq).max() < H_TOL
    assert abs(costs[0] - float(cost)) < 5e-3 * max(1.0, float(cost))
    for i in range(5):
        sc = max(1e-6, np.abs(g[i]).max())
        d = np.abs(grads[1][i] - grads[0][i]).max() / sc
        print("fp16 B=256 grad layer %d: f16-MFMA vs fp32-MFMA routine %.2e of max|g|; vs half oracle rel Frobenius %.2e" % (i, d, _rel_fro(grads[1][i], g[i])))
        assert d < (1e-3 if i == 0 else 1e-5), i
        assert _rel_fro(grads[1][i], g[i]) < 5e-2, i
    _fp64_yardstick(A, B, ws, wt, mb, grads[1], g, "fp16 A=3 B=256")


@pytest.mark.parametrize("B", [128, 160])
def test_fp16_blocked_forward_ragged_batches(sd, B):
    """float16, B >= 128: the forward stages run on the register-blocked packed-fp16 routine (64-row blocks per wave).  B = 160 leaves
    half-filled blocks in every stage (fc4: 160 = 2.5 blocks per net); online Q of a train step and `predict` vs the half oracle, and
    vs the unblocked routine forced through the `nw:<kernel id>` tuning hook (other K-split, so not bit-identical)."""
    A = 4
    mb = random_minibatch(B, A, 742, reward_range=(-2, 3))
    qs, ps = [], []
    for unblocked in (0, 1):
        net, ws, wt = _net(sd, A, B, 741, datatype="float16")
        if unblocked:
            for kid in (0, 1, 2, 3):
                net.set_option("nw:%d" % kid, 8)
        ps.append(net.predict(mb[0]).copy())
        net.train(mb)
        qs.append(net.last_q()[0].copy())
    o = OracleDQN(A, batch_size=B, weights=ws, half_activations=True)
    o.Wt = [w.copy() for w in wt]
    _, _, _, preq = o.gradients(mb)
    print("fp16 B=%d: blocked vs oracle %.2e, unblocked vs oracle %.2e, blocked vs unblocked %.2e" % (
        B, np.abs(qs[0] - preq).max(), np.abs(qs[1] - preq).max(), np.abs(qs[0] - qs[1]).max()))
    for q in qs + ps:
        assert np.abs(q - preq).max() < H_TOL
    assert np.abs(qs[0] - qs[1]).max() < H_TOL


@pytest.mark.parametrize("B", [128, 131, 256])
def test_fp16_conv1_forward_on_exact_bytes(sd, B):
    """float16, B >= 128: conv1 forward keeps the frame bytes exact (half(1024 + b) is the bit pattern 0x6400 | b; - 1024 is exact; the
    1 / 255 of deepqnetwork.py:100 multiplies the fp32 sum) — conv1_hb_kernel, with write-through (default) and plain output stores —
    against the first form's half(b / 255) operands (bt:0 = 1).  Each form is held to the oracle of ITS input semantics more tightly than
    the two semantics differ, the two store kinds are bit-identical, and the result is run-to-run stable."""
    A = 3
    mb = random_minibatch(B, A, 750 + B, reward_range=(-2, 3))
    qs = {}
    for name, menu in (("exact", 0), ("exact_plain", 2), ("first", 1)):
        net, ws, wt = _net(sd, A, B, 749, datatype="float16")
        net.set_option("bt:0", menu)
        qs[name] = net.predict(mb[0]).copy()
        assert np.array_equal(qs[name], net.predict(mb[0]))
    o_exact = OracleDQN(A, batch_size=B, weights=ws, half_activations=True, exact_conv1_input=True)
    o_half = OracleDQN(A, batch_size=B, weights=ws, half_activations=True, exact_conv1_input=False)
    qe, qh = o_exact.predict(mb[0]), o_half.predict(mb[0])
    print("fp16 B=%d conv1: exact form vs its oracle %.2e, first form vs its oracle %.2e, the two semantics apart %.2e (library) / %.2e (oracles)" % (
        B, np.abs(qs["exact"] - qe).max(), np.abs(qs["first"] - qh).max(), np.abs(qs["exact"] - qs["first"]).max(), np.abs(qe - qh).max()))
    assert np.array_equal(qs["exact"], qs["exact_plain"])
    assert np.abs(qs["exact"] - qe).max() < 1.5e-4 and np.abs(qs["first"] - qh).max() < 1.5e-4
    assert np.abs(qs["exact"] - qs["first"]).max() < H_TOL
    # conv1's weight gradient with the same two input semantics (c1w_h_kernel<true> / <false>: bt:18 = 0 / 1) behind the SAME forward pass
    # (another forward semantics flips Rectlin gates through the net: 2-4e-2 of the gradient, tools/exp/c1w_h_iso.py): the two differ by
    # the half rounding of the inputs only, and the default pair is held to the oracle of its semantics
    g0 = {}
    for name, menu in (("exact", 0), ("first", 1)):
        net, ws, wt = _net(sd, A, B, 749, datatype="float16")
        net.set_option("keep_gradients", 1); net.set_option("bt:18", menu)
        net.train(mb)
        g0[name] = net.get_layer(0, which=3)
    o_exact.Wt = [w.copy() for w in wt]
    ge = o_exact.gradients(mb)[0][0]
    print("fp16 B=%d conv1 wgrad: exact vs first (same forward) %.2e, exact vs the oracle %.2e (rel Frobenius)" % (B, _rel_fro(g0["exact"], g0["first"]), _rel_fro(g0["exact"], ge)))
    assert _rel_fro(g0["exact"], g0["first"]) < 2e-3 and _rel_fro(g0["exact"], ge) < 5e-2


# ---- configs[2]: B = 256 --------------------------------------------------------------------------------------------
def test_batch256_a6_one_step(sd):
    A, B = 6, 256
    net, ws, wt = _net(sd, A, B, 631)
    o = OracleDQN(A, batch_size=B, weights=ws)
    o.Wt = [w.copy() for w in wt]
    net.set_option("keep_gradients", 1)
    mb = random_minibatch(B, A, 632, reward_range=(-2, 3))
    g, cost, _, preq = o.gradients(mb)
    costs = []
    net.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
    net.train(mb)
    q, _ = net.last_q()
    assert np.abs(q - preq).max() < Q_TOL
    assert abs(costs[0] - float(cost)) < 1e-5 * max(1.0, float(cost))
    for i in range(5):
        rel = np.abs(net.get_layer(i, 3) - g[i]).max() / max(1e-3, np.abs(g[i]).max())
        assert rel < 2e-4, (i, rel)                            # K = B*400 = 102400-long fp32 sums in conv1 wgrad


def test_batch256_train_from_memory_five_steps(sd):
    """The fused loop (native sampler -> gather fused into conv1 -> step) at B = 256, A = 3, five consecutive steps from
    a ring.  Indexes bit-exact (the native sampler consumes exactly the reference's draws).  Each step starts from the
    oracle's exact (theta, theta-, s) — teacher-forced like test_100_step_q_parity_teacher_forced, because free-running
    fp32 implementations of this algorithm separate through ReLU / clip-boundary mask flips, and a B = 256
    step has 8x the activations of a B = 32 one (measured free-running after 5 steps: 2.3e-3).  Per step: cost to
    round-off, Q of a held-out batch within 1e-4 on at least 4 of the 5 steps, median at round-off level, none > 2e-3."""
    A, B, size = 3, 256, 6000
    args = make_args(batch_size=B)
    mem, omem = sd.ReplayMemory(size, args), ReplayOracle(size, batch_size=B)
    synthetic_fill(mem, 641, num_actions=A)
    synthetic_fill(omem, 641, num_actions=A)
    mem.sync_mirror()
    net, ws, wt = _net(sd, A, B, 642)
    o = OracleDQN(A, batch_size=B, weights=ws)
    o.Wt = [w.copy() for w in wt]
    hold = random_minibatch(B, A, 644)[0]
    random.seed(643)
    errs = []
    for s in range(5):
        net.set_weights(o.W, 0); net.set_weights(o.Wt, 1); net.set_weights(o.S, 2)
        st = random.getstate()
        c = net.train_from_memory(mem, 1, want_cost=True)
        after = random.getstate()
        random.setstate(st)
        co = float(o.train(omem.getMinibatch()))
        assert random.getstate() == after, s                   # the native sampler consumed exactly the reference's draws
        assert abs(c - co) < 1e-5 * max(1.0, co), (s, c, co)
        errs.append(float(np.abs(net.predict(hold) - o.predict(hold)).max()))
    errs = np.array(errs)
    print("B=256 fused loop, 5 teacher-forced steps: Q max-abs err per step %s" % ["%.2e" % e for e in errs])
    assert np.median(errs) < 1e-5
    assert (errs < Q_TOL).sum() >= 4
    assert errs.max() < 2e-3


# ---- data-parallel arithmetic, not the identity ---------------------------------------------------------------------
@pytest.mark.parametrize("datatype", ["float32"])
def test_dp_arithmetic_two_learners_one_gpu(sd, datatype):
    """What two data-parallel ranks compute, on one GPU without RCCL: each learner stops after its LOCAL gradient sums
    (option grad_only = update mode 1), the host adds the two flat gradients (the all-reduce), and the library's
    apply-only update (mode 2) runs with divisor R*B = 2B on both — the result must equal the oracle trained on the
    concatenated 2B batch (Neon semantics: gradient SUM over the batch, then grad / be.bsz, deepqnetwork.py:162-165),
    and both learners must end bit-identical."""
    A, B = 4, 32
    n1, ws, wt = _net(sd, A, B, 651, datatype=datatype)
    n2, _, _ = _net(sd, A, B, 651, datatype=datatype)
    o = OracleDQN(A, batch_size=2 * B, weights=ws)
    o.Wt = [w.copy() for w in wt]
    for n in (n1, n2):
        n.set_option("grad_only", 1)
    for s in range(3):
        mb1 = random_minibatch(B, A, 652 + 2 * s, reward_range=(-2, 3))
        mb2 = random_minibatch(B, A, 653 + 2 * s, reward_range=(-2, 3))
        w_before = n1.get_weights(0)
        n1.train(mb1); n2.train(mb2)
        for a, b in zip(n1.get_weights(0), w_before):
            assert np.array_equal(a, b)                        # grad_only really applied nothing
        gsum = [n1.get_layer(i, 3) + n2.get_layer(i, 3) for i in range(5)]      # the all-reduce (sum), on the host
        both = tuple(np.concatenate([x, y]) for x, y in zip(mb1, mb2))
        g, _, _, _ = o.gradients(both)
        for i in range(5):
            # the two learners + host add accumulate in a different order than the oracle's single 64-sample sum, and a
            # ReLU pre-activation within round-off of 0 gates one learner's unit and not the oracle's (a finite, local
            # difference — DESIGN.md §2; one flipped conv1 unit touches 16 taps x 64 maps = 3 % of conv2's gradient): at least
            # 98 % of the weights within 1e-4 of max|g| (measured 99.5-100 %), none beyond 2e-3 (measured 5.7e-4).  A wrong
            # divisor, a lost half batch or a layout slip would put every element at O(1).
            err = np.abs(gsum[i] - g[i]) / max(1e-3, np.abs(g[i]).max())
            assert (err < 1e-4).mean() >= 0.98 and err.max() < 2e-3, ("grad", s, i, float(err.max()), float((err < 1e-4).mean()))
        for n in (n1, n2):
            for i in range(5):
                n.set_layer(i, gsum[i], 3)
            n.apply_update(2 * B)
        o.rmsprop(g, 2 * B)
        for i in range(5):
            assert np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)), i
            assert np.array_equal(n1.get_layer(i, 2), n2.get_layer(i, 2)), i
            big = np.abs(g[i]) / (2 * B) > 1e-6
            assert np.abs(n1.get_layer(i, 0) - o.W[i])[big].max() < 2e-5, ("weights", s, i)
            assert np.abs(n1.get_layer(i, 2) - o.S[i]).max() < 1e-6 + 1e-3 * np.abs(o.S[i]).max(), ("state", s, i)
        # keep the three in lock-step for the next round (the comparison above is per step, not free-running)
        for n in (n1, n2):
            n.set_weights(o.W, 0); n.set_weights(o.S, 2)
    hold = random_minibatch(B, A, 660)[0]
    assert np.abs(n1.predict(hold) - o.predict(np.concatenate([hold, hold]))[:B]).max() < Q_TOL


def test_dp_divisor_is_ranks_times_batch(sd):
    """apply_update(bsz) with bsz = B reproduces the ordinary single-learner step bit for bit; with 2B it does not."""
    A, B = 4, 32
    ref, _, _ = _net(sd, A, B, 671)
    ref.set_option("keep_gradients", 1)
    n, _, _ = _net(sd, A, B, 671)
    n.set_option("grad_only", 1)
    mb = random_minibatch(B, A, 672)
    ref.train(mb); n.train(mb)
    n.apply_update(B)
    for i in range(5):
        assert np.array_equal(ref.get_layer(i, 0), n.get_layer(i, 0)), i
        assert np.array_equal(ref.get_layer(i, 2), n.get_layer(i, 2)), i
    n2, _, _ = _net(sd, A, B, 671)
    n2.set_option("grad_only", 1)
    n2.train(mb); n2.apply_update(2 * B)
    assert not np.array_equal(ref.get_layer(3, 2), n2.get_layer(3, 2))


def test_fp16_dp_half_payload_and_overflow_skip(sd):
    """SURVEY.md §8e, configs[4]: under data parallel the float16 mode all-reduces the gradient as IEEE half (x 2^6) and
    accumulates in fp32.  1-rank RCCL communicator on the one GPU (the all-reduce is the identity, the half round trip is
    not): (a) weights track the single-GPU float16 path to half-rounding of the gradient; the fp32-payload option
    reproduces the single-GPU path exactly like the float32 test does; (b) a payload scale that overflows half makes
    every value inf -> the step is skipped: parameters and optimizer state untouched, skipped-step counter counts."""
    from simple_dqn_amd.deepqnetwork import dp_unique_id
    A, B = 4, 32
    ref, _, _ = _net(sd, A, B, 691, datatype="float16")
    ref.set_option("keep_gradients", 1)
    nh, _, _ = _net(sd, A, B, 691, datatype="float16")
    nh.dp_init(dp_unique_id(), 0, 1)
    mbs = [random_minibatch(B, A, 692 + s) for s in range(3)]
    ref.train(mbs[0]); nh.train(mbs[0])
    for i in range(5):                                          # one step: exactly the half round trip of g, nothing else
        g0, g1 = ref.get_layer(i, 3), nh.get_layer(i, 3)
        ok = np.abs(g1 - g0) <= 4.9e-4 * np.abs(g0) + 1e-10     # 2^-11 relative (round to nearest half of g x 2^10)
        dw = np.abs(nh.get_layer(i, 0) - ref.get_layer(i, 0)).max()
        print("fp16 DP half payload layer %d: %.4f of the gradient within 2^-11, max |dW| after one step %.2e" % (i, ok.mean(), dw))
        assert ok.mean() > 0.999 and dw < 1e-6, i
    for mb in mbs[1:]:
        ref.train(mb); nh.train(mb)
    assert nh.overflow_steps() == 0
    for i in range(5):                                          # three free-running half-precision steps: gate flips (see the A=6 test) -> loose
        assert np.abs(nh.get_layer(i, 0) - ref.get_layer(i, 0)).max() < 3e-3, i
    nh.dp_shutdown()
    # fp32 payload option: bit-identical to the single-GPU (materialised-gradient) float16 path
    nf, _, _ = _net(sd, A, B, 691, datatype="float16")
    nf.set_option("dp_half", 0)
    nf.dp_init(dp_unique_id(), 0, 1)
    for mb in mbs:
        nf.train(mb)
    for i in range(5):
        assert np.array_equal(nf.get_layer(i, 0), ref.get_layer(i, 0)), i
    nf.dp_shutdown()
    # overflow: 2^30 x gradient does not fit half -> inf after the all-reduce -> skipped
    no, _, _ = _net(sd, A, B, 691, datatype="float16")
    no.set_option("dp_half_scale_log2", 30)
    no.dp_init(dp_unique_id(), 0, 1)
    w0, s0 = no.get_weights(0), no.get_weights(2)
    for mb in mbs[:2]:
        no.train(mb)
    assert no.overflow_steps() == 2
    for a, b in zip(no.get_weights(0), w0):
        assert np.array_equal(a, b)
    for a, b in zip(no.get_weights(2), s0):
        assert np.array_equal(a, b)
    no.set_option("dp_half_scale_log2", -1)                     # back to the dynamic scale
    no.train(mbs[0])                                            # and training resumes once the scale fits again
    assert no.overflow_steps() == 2 and not np.array_equal(no.get_layer(3, 0), w0[3])
    no.dp_shutdown()
    # (c) the device-side dynamic scale (halve per overflow, double after 200 clean steps) is driven through its own entry points in
    #     tests/test_gpu_dp_multiproc.py::test_fp16_dynamic_payload_scale_state_machine


# ---- boundary: --device_id, ring-action validation, error text ------------------------------------------------------
def test_device_id_is_honoured_or_refused(sd):
    """src/deepqnetwork.py:29-34 passes args.device_id to the backend.  Here: the drop-in classes bind it; the bound
    device is reported; a second object asking for ANOTHER device is refused instead of silently running on this one."""
    lib = sd.load()
    dev = C.c_int(-1)
    assert lib.sdqn_get_device(C.byref(dev)) == 0
    assert dev.value == 0
    net = sd.DeepQNetwork(4, make_args(batch_size=8, device_id=0))       # same device again: fine
    assert net.dp_info()["bound_device"] == 0 and net.dp_info()["comm_ranks"] == -1
    n = C.c_int(0)
    assert lib.sdqn_device_count(C.byref(n)) == 0
    other = 1 if n.value > 1 else 7
    with pytest.raises(RuntimeError) as ei:
        sd.DeepQNetwork(4, make_args(batch_size=8, device_id=other))
    assert "already bound to device 0" in str(ei.value)
    with pytest.raises(RuntimeError):
        sd.ReplayMemory(100, make_args(batch_size=8, device_id=other))
    assert lib.sdqn_set_device(0) == 0                                    # C ABI: re-asking for the bound device is a no-op
    assert lib.sdqn_set_device(other) == -4                               # SDQN_ERR_STATE


def test_untracked_writes_cannot_go_stale_silently(sd):
    """VERDICT r3 weak #10 / ADVICE r3: (1) an alias of the ring that escapes the write tracking is READ-ONLY — `np.asarray(mem.screens)[5] = 7`
    raises instead of training on a stale mirror; (2) slots that a direct assignment of count / current newly exposes are uploaded before the
    next device use even when they were filled behind the tracking's back (raw pointers)."""
    import ctypes as C
    B, size, A = 8, 400, 4
    args = make_args(batch_size=B)
    mem, omem = sd.ReplayMemory(size, args), ReplayOracle(size, batch_size=B)
    synthetic_fill(mem, 7, num_actions=A); synthetic_fill(omem, 7, num_actions=A)
    mem.getMinibatch()
    for alias in (np.asarray(mem.screens), mem.screens.view(np.ndarray), np.asarray(mem.rewards), np.asarray(mem.prestates)):
        with pytest.raises(ValueError):
            alias[5] = 7
    x = mem.screens[5]; x[...] = 7; omem.screens[5] = 7                  # the tracked door: a view of a view
    assert mem.mirror_dirty[0] == [(5, 6)]
    idx = np.array([6, 7, 8, 9, 20, 21, 22, 23])
    assert np.array_equal(mem.gather(idx)[0], np.stack([omem.getState(i - 1) for i in idx]))
    # a fill through raw pointers (what the tracking cannot see), then count moves over it: the backstop uploads the exposed slots
    mem2 = sd.ReplayMemory(size, args)
    synthetic_fill(mem2, 7, num_actions=A)
    mem2.count = 100; mem2.current = 100
    mem2.getMinibatch()
    assert mem2.mirror_dirty == (None, None)
    ps = C.cast(mem2._raw["screens"].ctypes.data, C.POINTER(C.c_uint8))
    frame = 84 * 84
    for i in range(100 * frame, 130 * frame, 97):
        ps[i] = (ps[i] + 1) % 256                                          # bytes of slots 100..129 change in the pinned master only
    assert mem2.mirror_dirty == (None, None)
    mem2.count = 130                                                      # newly exposed: [100, 130)
    assert mem2.mirror_dirty[0] == [(100, 130)]
    idx2 = np.array([104, 110, 115, 120, 125, 127, 128, 129])
    pre = mem2.gather(idx2)[0]
    assert np.array_equal(pre, np.stack([np.asarray(mem2.screens[i - 4:i]) for i in idx2]))
    mem2.current = 10                                                     # moved across the wrap: [130 .. size) and [0, 10) exposed
    d = mem2.mirror_dirty[0]
    assert d[0][0] == 0 and d[0][1] >= 10 and d[-1][1] == size


def test_ring_action_out_of_range_is_rejected(sd):
    """the ring paths took actions unchecked (the tuple API checks them, sdqn_api_step.hip: sdqn_net_train_host)."""
    A, B, size = 4, 8, 300
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.actions[:] = A                                                    # every slot holds an action the net lacks
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    random.seed(1)
    with pytest.raises(AssertionError) as ei:
        net.train_from_memory(mem, 2)
    assert "actions" in str(ei.value)
    idx = np.arange(10, 10 + B)
    with pytest.raises(AssertionError):
        net.train_indexes(mem, idx)
    mem.count = 100
    with pytest.raises(AssertionError):
        mem.gather(np.full(B, 150))                                       # beyond count (was: only beyond size)


def test_writes_through_the_numpy_views_reach_the_mirror(sd):
    """VERDICT r2 item 8 (was: a heuristic that refused bulk fills only).  The reference has ONE copy of the ring
    (replay_memory.py:10-13); here the numpy attributes are tracked views of the pinned master and every in-place write marks
    the slots it touched, which are uploaded to the HBM mirror before the next device use: a bulk fill needs no sync_mirror(),
    and an in-place edit of frames / metadata AFTER training is what the next gather returns — never stale frames."""
    B, size, A = 8, 300, 4
    args = make_args(batch_size=B)
    mem, omem = sd.ReplayMemory(size, args), ReplayOracle(size, batch_size=B)
    synthetic_fill(mem, 5, num_actions=A)                                 # writes the views, assigns count / current: NO sync_mirror()
    synthetic_fill(omem, 5, num_actions=A)
    assert mem.mirror_dirty[0] is not None
    net = sd.DeepQNetwork(A, args)
    random.seed(1); st = random.getstate()
    got = [x.copy() for x in mem.getMinibatch()]
    assert mem.mirror_dirty == (None, None)
    random.setstate(st)
    for a, b in zip(got, omem.getMinibatch()):
        assert np.array_equal(a, b)
    net.train_from_memory(mem, 2)
    # in-place edits without any sync: a frame range, single metadata entries, an out= ufunc on a slice
    for m in (mem, omem):
        m.screens[40:60] = 255 - m.screens[40:60]
        m.rewards[45] = 7; m.actions[50] = 3; m.terminals[52] = True; m.terminals[40:48] = False
        np.bitwise_xor(m.screens[100:130], np.uint8(0x5A), out=m.screens[100:130])
    assert mem.mirror_dirty[0] == [(40, 60), (100, 130)] and mem.mirror_dirty[1] == [(40, 48), (50, 51), (52, 53)]
    idx = np.array([44, 46, 50, 53, 58, 105, 120, 129])
    pre, act, rew, post, term = [x.copy() for x in mem.gather(idx)]
    opre = np.stack([omem.getState(i - 1) for i in idx]); opost = np.stack([omem.getState(i) for i in idx])
    assert np.array_equal(pre, opre) and np.array_equal(post, opost)
    assert np.array_equal(act, omem.actions[idx]) and np.array_equal(rew, omem.rewards[idx]) and np.array_equal(term, omem.terminals[idx])
    # the fused train path reads the same mirror: identical to training on the oracle-gathered minibatch
    n1, n2 = sd.DeepQNetwork(A, args), sd.DeepQNetwork(A, args)
    ws = xavier_weights(A, 6)
    for n in (n1, n2):
        n.set_weights(ws, 0); n.update_target_network()
    mem.screens[200:210] = 9                                              # one more edit right before the fused step
    omem.screens[200:210] = 9
    idx2 = np.array([203, 205, 207, 209, 44, 46, 120, 129])
    n1.train_indexes(mem, idx2)
    n2.train((np.stack([omem.getState(i - 1) for i in idx2]), omem.actions[idx2], omem.rewards[idx2],
              np.stack([omem.getState(i) for i in idx2]), omem.terminals[idx2]))
    for i in range(5):
        assert np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)), i
    scr = np.full((84, 84), 3, np.uint8)
    mem.add(1, 0, scr, False)                                             # add() keeps the mirror current by itself
    assert mem.mirror_dirty == (None, None)
    mem.getMinibatch()
    # zero-copy ring: the kernels read the pinned FRAMES themselves, but the metadata they read is the packed MetaRec array,
    # which only an upload_meta re-packs from the actions / rewards / terminals views — so frames are never dirty there, metadata is
    zc, ozc = sd.ReplayMemory(size, args, flags=2), ReplayOracle(size, batch_size=B)
    synthetic_fill(zc, 5, num_actions=A); synthetic_fill(ozc, 5, num_actions=A)
    assert zc.mirror_dirty[0] is None and zc.mirror_dirty[1] is not None
    zc.getMinibatch()
    assert zc.mirror_dirty == (None, None)
    for m in (zc, ozc):
        m.rewards[45] = -9; m.actions[50] = 2; m.terminals[40:60] = False; m.terminals[53] = True; m.screens[44] = 17
    assert zc.mirror_dirty[0] is None and zc.mirror_dirty[1] == [(40, 60)]
    _, act, rew, _, term = zc.gather(idx)
    assert np.array_equal(act, ozc.actions[idx]) and np.array_equal(rew, ozc.rewards[idx]) and np.array_equal(term, ozc.terminals[idx])
    _, _, rew2, _, term2 = zc.gather(np.array([45, 46, 50, 53, 58, 105, 120, 129]))
    assert rew2[0] == -9 and bool(term2[3]) is True


def test_minibatch_small_arrays_are_copies(sd):
    """replay_memory.py:76-79: prestates/poststates alias the preallocated buffers, actions/rewards/terminals are fresh."""
    B, size = 8, 400
    mem = sd.ReplayMemory(size, make_args(batch_size=B))
    synthetic_fill(mem, 5, num_actions=4)
    mem.sync_mirror()
    random.seed(2)
    p1, a1, r1, q1, t1 = mem.getMinibatch()
    a1c, r1c, t1c = a1.copy(), r1.copy(), t1.copy()
    p2, a2, r2, q2, t2 = mem.getMinibatch()
    assert p1 is p2 and q1 is q2
    assert np.array_equal(a1, a1c) and np.array_equal(r1, r1c) and np.array_equal(t1, t1c)
    assert a1.dtype == np.uint8 and r1.dtype == np.int64 and t1.dtype == np.bool_


def test_on_train_called_per_step_with_callback(sd):
    """deepqnetwork.py:168-172: every step reports its cost; the fused n-step loop keeps that when a callback is set."""
    A, B, size = 4, 16, 800
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 7, num_actions=A)
    mem.sync_mirror()
    n1, _, _ = _net(sd, A, B, 681)
    n2, _, _ = _net(sd, A, B, 681)
    c1, c2 = [], []
    n1.callback = type("CB", (), {"on_train": lambda self, c: c1.append(c)})()
    n2.callback = type("CB", (), {"on_train": lambda self, c: c2.append(c)})()
    random.seed(4); st = random.getstate()
    n1.train_from_memory(mem, 4)
    random.setstate(st)
    for _ in range(4):
        n2.train(mem.getMinibatch())
    assert len(c1) == 4 and c1 == c2 and n1.train_iterations == 4
    for i in range(5):
        assert np.array_equal(n1.get_layer(i), n2.get_layer(i)), i


def test_tuple_api_is_asynchronous_and_safe(sd):
    """DeepQNetwork.train(minibatch) no longer synchronises the stream: pageable arrays are copied into a pinned double buffer
    first, so the caller may overwrite them the moment train() returns (deepqnetwork.py:94-100 copies too); the pinned
    prestates / poststates of this library's ReplayMemory are uploaded in place (their next overwrite is stream-ordered)."""
    A, B, size = 4, 32, 1500
    args = make_args(batch_size=B)
    clean, _, _ = _net(sd, A, B, 711)
    dirty, _, _ = _net(sd, A, B, 711)
    for s in range(6):                                          # > 2 steps: both staging slots are reused
        mb = random_minibatch(B, A, 712 + s)
        clean.train(mb)
        scratch = [x.copy() for x in mb]
        dirty.train(tuple(scratch))
        for x in scratch:
            x[...] = 0 if x.dtype != np.uint8 else 255          # clobber the caller's arrays right after the call returned
    for i in range(5):
        assert np.array_equal(clean.get_layer(i, 0), dirty.get_layer(i, 0)), i
    # the library's own pinned minibatch buffers, interleaved gathers
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 713, num_actions=A)
    mem.sync_mirror()
    n1, _, _ = _net(sd, A, B, 714)
    n2, _, _ = _net(sd, A, B, 714)
    random.seed(9); st = random.getstate()
    for _ in range(4):
        n1.train(mem.getMinibatch())                            # H2D straight from the pinned buffers, no sync; next gather overwrites them
    random.setstate(st)
    n2.train_from_memory(mem, 4)
    for i in range(5):
        assert np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)), i
    # ... and the caller may WRITE those pinned views the moment train() has returned (the upload is waited for
    # before the call returns): clobbering mem.prestates / mem.poststates after every step must not change the training
    n3, _, _ = _net(sd, A, B, 714)
    random.setstate(st)
    for _ in range(4):
        mb = mem.getMinibatch()
        n3.train(mb)
        mem.prestates[...] = 255; mem.poststates[...] = 0       # same memory as mb[0] / mb[3]
    for i in range(5):
        assert np.array_equal(n3.get_layer(i, 0), n2.get_layer(i, 0)), i


def test_tuple_api_lazy_states_read_write_alias_and_stale_generation(sd):
    """Round 5: getMinibatch() enqueues the gather and returns at once; prestates / poststates of the tuple are lazy
    views of the aliased buffers (replay_memory.py:21-22,76-79) whose host copy is fetched on first access, the three small arrays are
    ring[indexes].  Cases: read-after-return (bytes = the reference's gather), untouched tuple -> train reads the device copy,
    read-then-train, write-then-train (the written host data is what trains), Statistics-style aliasing (statistics.py:85-86), and a
    tuple whose device minibatch has been replaced by a later gather (trains on the aliased buffers' CURRENT content like the reference)."""
    from oracle.replay_numpy import ReplayOracle
    from simple_dqn_amd._lazy import LazyMinibatchArray
    A, B, size = 4, 32, 1500
    args = make_args(batch_size=B)
    mem, omem = sd.ReplayMemory(size, args), ReplayOracle(size, batch_size=B)
    synthetic_fill(mem, 813, num_actions=A); synthetic_fill(omem, 813, num_actions=A)
    mem.sync_mirror()
    # read after return
    random.seed(21); st = random.getstate()
    mb = mem.getMinibatch()
    assert isinstance(mb[0], LazyMinibatchArray) and isinstance(mb[3], LazyMinibatchArray) and mem._mb_pending
    assert mb[0].shape == (B, 4, 84, 84) and mb[1].shape == mb[2].shape == mb[4].shape == (B,) and mem._mb_pending      # no fetch for metadata
    random.setstate(st); omb = omem.getMinibatch()
    for a, b in zip(mb, omb):
        assert np.array_equal(np.asarray(a), b)
    assert not mem._mb_pending and np.shares_memory(np.asarray(mb[0]), np.asarray(mem.prestates)) and mb[0] is mem.prestates and mb[1].flags.writeable and mb[1].base is None
    after_one = random.getstate()
    random.setstate(st); omem.getMinibatch(); assert random.getstate() == after_one                                  # same stream position

    def fresh():
        return _net(sd, A, B, 814)[0]

    def same(n1, n2):
        for i in range(5):
            assert np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)), i

    # untouched tuple == explicit arrays == read-then-train
    n_dev, n_host, n_read = fresh(), fresh(), fresh()
    random.seed(22)
    for s in range(3):
        st = random.getstate()
        mb = mem.getMinibatch(); n_dev.train(mb)
        assert mem._mb_pending                                                  # nobody looked: the states never came to the host
        random.setstate(st); mb = mem.getMinibatch(); n_host.train(tuple(np.array(x) for x in mb))
        random.setstate(st); mb = mem.getMinibatch(); assert int(np.asarray(mb[0]).sum()) > 0; n_read.train(mb)
    same(n_dev, n_host); same(n_dev, n_read)
    # ... and how the library served them: the untouched tuple uploaded NOTHING (states in place, small arrays equal to what the gather
    # left on the device); arrays from elsewhere are uploaded whole; a host read of the states changes nothing about that
    assert n_dev.tuple_counters() == (3, 3, 3) and n_host.tuple_counters() == (3, 0, 0) and n_read.tuple_counters() == (3, 3, 3)
    # write-then-train: what the caller wrote is what trains
    n_w, n_ref = fresh(), fresh()
    mb = mem.getMinibatch()
    mb[0][:, 0] = 7; mb[3][5] = 0                                                # through the lazy views (fetch, then tracked writes)
    expect = tuple(np.array(x) for x in mb)
    assert (expect[0][:, 0] == 7).all() and (expect[3][5] == 0).all()
    n_w.train(mb); n_ref.train(expect)
    same(n_w, n_ref)
    # the small arrays are the caller's own copies: edits are honoured, the ring is untouched
    n_w, n_ref = fresh(), fresh()
    mb = mem.getMinibatch()
    mb[2][:] = 1; mb[4][:] = False
    n_w.train(mb)
    n_ref.train((np.array(mem.prestates), mb[1], np.ones(B, np.int64), np.array(mem.poststates), np.zeros(B, bool)))
    same(n_w, n_ref)
    assert n_w.tuple_counters() == (1, 1, 0)                                     # states in place, the edited small arrays uploaded
    # one edited element is enough (the comparison is by value over all 10 x B bytes); a ring slot rewritten between the gather and the
    # step changes nothing: the tuple's arrays and the device copy both hold the gather-time values
    for which, val in ((1, None), (2, 5), (4, None)):
        n_w, n_ref = fresh(), fresh()
        mb = mem.getMinibatch()
        if which == 1: mb[1][B - 1] = (int(mb[1][B - 1]) + 1) % A
        elif which == 2: mb[2][0] += val
        else: mb[4][3] = not mb[4][3]
        n_w.train(mb)
        n_ref.train(tuple(np.array(x) for x in mb))
        same(n_w, n_ref); assert n_w.tuple_counters() == (1, 1, 0), which
    n_w, n_ref = fresh(), fresh()
    mb = mem.getMinibatch()
    expect = tuple(np.array(x) for x in mb)
    slot = int(mem.last_indexes[0])
    keep = (int(mem.actions[slot]), int(mem.rewards[slot]), bool(mem.terminals[slot]))
    mem.actions[slot] = (keep[0] + 1) % A; mem.rewards[slot] = keep[1] + 3; mem.terminals[slot] = not keep[2]    # the ring moves on ...
    n_w.train(mb); n_ref.train(expect)                                          # ... the tuple and the device minibatch do not
    same(n_w, n_ref); assert n_w.tuple_counters() == (1, 1, 1)
    mem.actions[slot], mem.rewards[slot], mem.terminals[slot] = keep            # put the ring back for the cases below
    # Statistics-style aliasing: the array kept from one call shows the next call's states (the reference's aliased buffers)
    keep = mem.getMinibatch()[0]
    first = np.array(keep)
    mb2 = mem.getMinibatch()
    assert np.array_equal(np.asarray(keep), np.asarray(mb2[0])) and keep is mem.prestates and not np.array_equal(first, np.asarray(keep))
    # stale generation: the device minibatch was replaced by a later gather before train() -> the buffers' current content trains
    n_s, n_ref = fresh(), fresh()
    mb1 = mem.getMinibatch()
    mb2 = mem.getMinibatch()
    n_s.train(mb1)
    n_ref.train((np.array(mb2[0]), mb1[1], mb1[2], np.array(mb2[3]), mb1[4]))
    same(n_s, n_ref)


def test_train_iterations_and_device_sync_at_the_c_abi(sd):
    """deepqnetwork.py:168 for a C caller: sdqn_net_train_iterations counts every step whichever entry point ran it (tuple, ring,
    n-step loop); sdqn_device_sync returns once the library stream has drained (the cost of the last step is then final)."""
    import ctypes as C
    from simple_dqn_amd import _lib
    A, B = 4, 32
    mem = sd.ReplayMemory(900, make_args(batch_size=B))
    synthetic_fill(mem, 921, num_actions=A); mem.sync_mirror()
    net = _net(sd, A, B, 922)[0]
    n = C.c_int64(-1)

    def iters():
        _lib.check(net._lib.sdqn_net_train_iterations(net._h, C.byref(n)))
        return n.value

    assert iters() == 0
    random.seed(5)
    net.train(mem.getMinibatch())                                   # sdqn_net_train_host
    net.train(random_minibatch(B, A, 923))
    assert iters() == 2
    net.train_from_memory(mem, 5)                                   # sdqn_net_train_many
    assert iters() == 7 == net.train_iterations
    idx = mem.sample_indexes()
    _lib.check(net._lib.sdqn_net_train_replay(net._h, mem._h, _lib.ptr(idx, C.c_int64), None))      # not waited for ...
    assert iters() == 8
    assert net._lib.sdqn_device_sync() == 0                         # ... until here
    w = [net.get_layer(i) for i in range(5)]
    assert net._lib.sdqn_device_sync() == 0 and all(np.array_equal(a, net.get_layer(i)) for i, a in enumerate(w))
    with pytest.raises(Exception):
        _lib.check(net._lib.sdqn_net_train_iterations(net._h, None))


def test_minibatch_generations_at_the_c_abi(sd):
    """sdqn_replay_minibatch_gen / sdqn_replay_declare_minibatch_on_device with an EXPLICIT generation (what a host binding that keeps
    several tuples alive would pass; DeepQNetwork.train passes 0 = 'whatever the aliased buffers show now'): every gather launch bumps the
    device generation, a fetch brings the host generation level, the current generation is honoured (nothing uploaded), a stale one is
    not — the host buffers' content trains, as for any caller that never declared anything."""
    import ctypes as C
    from simple_dqn_amd import _lib
    A, B, size = 4, 32, 1200
    mem = sd.ReplayMemory(size, make_args(batch_size=B))
    synthetic_fill(mem, 913, num_actions=A); mem.sync_mirror()
    lib, h = mem._lib, mem._h

    def gens():
        d, g = C.c_uint64(), C.c_uint64()
        _lib.check(lib.sdqn_replay_minibatch_gen(h, C.byref(d), C.byref(g)))
        assert d.value == mem._device_minibatch_gen()
        return d.value, g.value

    def train_raw(net, small):
        act, rew, term = (np.ascontiguousarray(x) for x in small)
        pre_p, post_p = mem._mb_ptrs
        _lib.check(net._lib.sdqn_net_train_host(net._h, pre_p, _lib.ptr(act, C.c_uint8), _lib.ptr(rew, C.c_int64), post_p,
                                                _lib.ptr(term.view(np.uint8), C.c_uint8), None))

    random.seed(31)
    d0, _ = gens()
    mb1 = mem.getMinibatch()
    d1, g1 = gens()
    assert d1 == d0 + 1 and g1 != d1                             # gathered, not fetched
    small1 = (mb1[1], mb1[2], mb1[4])
    n_cur, n_ref = _net(sd, A, B, 914)[0], _net(sd, A, B, 914)[0]
    _lib.check(lib.sdqn_replay_declare_minibatch_on_device(h, d1))
    train_raw(n_cur, small1)
    assert n_cur.tuple_counters() == (1, 1, 1)                   # the current generation, named explicitly: the device copy trains
    host1 = (np.array(mb1[0]), np.array(mb1[3]))                 # (the fetch)
    assert gens() == (d1, d1)
    n_ref.train((host1[0], small1[0], small1[1], host1[1], small1[2]))
    for i in range(5):
        assert np.array_equal(n_cur.get_layer(i, 0), n_ref.get_layer(i, 0)), i
    # a later gather replaces the device minibatch; the host buffers still hold generation d1 (nobody has looked at the new one)
    mb2 = mem.getMinibatch()
    d2, g2 = gens()
    assert d2 == d1 + 1 and g2 == d1 and mem._mb_pending
    n_stale, n_ref = _net(sd, A, B, 915)[0], _net(sd, A, B, 915)[0]
    _lib.check(lib.sdqn_replay_declare_minibatch_on_device(h, d1))          # stale: not honoured
    train_raw(n_stale, small1)
    assert n_stale.tuple_counters() == (1, 0, 0)                 # uploaded from the host buffers = generation d1's states
    n_ref.train((host1[0], small1[0], small1[1], host1[1], small1[2]))
    for i in range(5):
        assert np.array_equal(n_stale.get_layer(i, 0), n_ref.get_layer(i, 0)), i
    # the declaration is one-shot: the next call without one uploads again even though nothing changed
    train_raw(n_stale, small1)
    assert n_stale.tuple_counters() == (2, 0, 0)
    assert np.array_equal(np.asarray(mb2[0]), np.asarray(mem.prestates)) and gens() == (d2, d2)


# ---- multi-GPU readiness that a 1-GPU box can check --------------------------------------------------------------------
def test_bench_dry_run_dp_two_ranks(sd):
    """bench.py under torch.distributed.run with 2 ranks sharing the one GPU (control plane only: gloo id exchange,
    barriers, max-reduce of the time; no RCCL communicator): the JSON line is the LAST stdout line and says n_gpus = 2."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "30", "--warmup", "10",
           "--replay-size", "20000", "--no-cpu-baseline", "--dry-run-dp", "--full"]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    out = json.loads(lines[-1])
    assert out["n_gpus"] == 2 and out["steps"] == 30 and out["value"] > 0
    assert out["dp"]["ranks"] == 2 and len(out["dp"]["per_rank"]) == 2
    # (round 5) an N-rank record carries the throughput regime too: configs[2]'s shape per learner, timed like the headline
    b = out["config_b256"]
    assert "error" not in b, b
    assert b["n_gpus"] == 2 and b["global_batch"] == 512 and b["value"] > 0 and b["dry_run"] is True and b["scaling"] == "weak"


def _run_bench(extra, timeout=900):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])


def test_bench_bare_gpus2_spawns_its_own_ranks(sd):
    """`python bench.py --gpus 2` launched WITHOUT torch.distributed.run (WORLD_SIZE unset) spawns its two
    ranks itself instead of exiting with a usage message; one JSON line, last on stdout, n_gpus = 2."""
    out = _run_bench(["--gpus", "2", "--steps", "20", "--warmup", "5", "--replay-size", "20000", "--no-cpu-baseline", "--dry-run-dp"])
    assert out["n_gpus"] == 2 and out["steps"] == 20 and out["value"] > 0
    assert out["dp"]["ranks"] == 2 and out["dp"]["dry_run"] is True


def test_bench_driver_form_brackets_the_timed_region(sd):
    """in the driver's short form (--steps 20 --warmup 5) the roofline of the dominant kernel is measured
    by a live HIP-event bracket INSIDE the timed region (launch 0 is bracketed after profile_reset), not replayed from the
    warm-up pass; the parity leg reports explicit checks."""
    out = _run_bench(["--steps", "20", "--warmup", "5", "--replay-size", "50000", "--no-cpu-baseline", "--full"])
    r = out["roofline"]
    assert r["measured_in"].startswith("timed region"), r["measured_in"]
    assert r["launches_bracketed"] >= 1 and 0 < r["frac"] <= 1.0
    q = out["q_mae_vs_cpu_ref"]
    assert q["mode"] == "free-running" and set(q["checks"]) and q["pass"] is True, q
    assert q["teacher_forced"]["mae"] < 1e-4


def test_bench_plain_run_and_dumped_outputs(sd, tmp_path):
    """A plain run (no --full) prints the headline line only and times exactly --steps steps; --dump-outputs writes the last step's
    Q-values, weights, RMSProp state and sampler state as float32 / float64 .npy files within 64 MB, and two runs with the same
    arguments write the same arrays (identical inputs: seeded ring, weights and sampler)."""
    import glob, os
    dumps = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        out = _run_bench(["--steps", "7", "--warmup", "3", "--replay-size", "20000", "--dump-outputs", d])
        assert out["steps"] == 7 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert abs(out["ms_per_step"] - 1e3 / out["value"]) <= 1e-3 * out["ms_per_step"] + 1e-4
        assert {"metric", "unit", "dtype"} <= set(out)
        assert not {"roofline", "kernels_us", "q_mae_vs_cpu_ref", "config_fp16", "config_b256", "cpu_baseline", "replay_gather"} & set(out)
        files = sorted(glob.glob(os.path.join(d, "*.npy")))
        arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
        assert {"q_online_last_minibatch", "max_q_target_last_minibatch", "sampler_state", "online_fc4", "rmsprop_s_conv1"} <= set(arrays)
        assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert sum(os.path.getsize(f) for f in files) <= 64 << 20
        assert arrays["q_online_last_minibatch"].shape == (32, 4) and np.isfinite(arrays["q_online_last_minibatch"]).all()
        dumps.append(arrays)
    assert set(dumps[0]) == set(dumps[1])
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


# ---- tuning hooks must not change the arithmetic ----------------------------------------------------------------------
@pytest.mark.parametrize("datatype", ["float32", "float16"])
def test_dispatch_order_and_slab_options_keep_the_numbers(sd, datatype):
    """`bwd_order` (which problem's workgroups of the fused bwd3 launch are dispatched first) must be bit-neutral: same tiles, same
    K split, other block indexes.  `tps:<layer>` (split-K slab size of a conv weight gradient) and `s4` (fc4 forward K-splits) change
    the summation order only: weights after 3 steps agree to fp32 round-off (float16: to the half oracle's own tolerance)."""
    A, B, size = 4, 32, 4000
    args = make_args(batch_size=B, datatype=datatype)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 801, num_actions=A)
    mem.sync_mirror()
    lib = sd.load()

    def run(opts):
        n, _, _ = _net(sd, A, B, 802, datatype=datatype)
        for k, v in opts: n.set_option(k, v)
        mt = (C.c_uint32 * 625)(); lib.sdqn_mt_seed(mt, 803)
        cost = [n.train_from_memory(mem, s, mt_state=mt, want_cost=True) for s in (1, 2)]
        return n, cost
    base, cb = run([])
    tol = 2e-6 if datatype == "float32" else 2e-3
    for opts in ([("tps:2", 14)], [("tps:1", 10), ("tps:3", 7)], [("s4", 4)]):
        n, c = run(opts)
        assert abs(c[-1] - cb[-1]) <= 1e-5 * max(1.0, abs(cb[-1])) if datatype == "float32" else True
        for i in range(5):
            d = np.abs(base.get_layer(i) - n.get_layer(i)).max()
            assert d < tol, (opts, i, d)


def test_bench_gather_with_index_sets(sd):
    """sdqn_replay_bench_gather_sets: a different index set per launch; the last launch's minibatch is the last set's, bit for bit;
    an index outside [history_length, count) is refused."""
    A, B, size = 4, 32, 3000
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 811, num_actions=A)
    mem.sync_mirror()
    o = ReplayOracle(size, batch_size=B); synthetic_fill(o, 811, num_actions=A)
    rng = np.random.RandomState(3)
    sets = rng.randint(4, mem.count, size=(5, B)).astype(np.int64)
    ms = mem.bench_gather(sets, iters=9)                      # launches: warm(set 0), then sets 1,2,3,4,0,1,2,3,4
    assert ms > 0
    assert sd.load().sdqn_replay_minibatch_to_host(mem._h) == 0          # (synchronises the library stream)
    pre = np.stack([o.getState(int(i) - 1) for i in sets[4]])
    assert np.array_equal(mem.prestates, pre)
    bad = sets.copy(); bad[2, 7] = mem.count
    with pytest.raises(AssertionError):
        mem.bench_gather(bad, iters=2)


def test_batched_slot_release_survives_interleaved_gathers(sd):
    """The train paths release their pinned index slots in batches of 16 (one event record instead of 16).  A slot released by a train
    call and not yet covered by an event must not be handed out again unflushed: 1 fused step, then > 64 getMinibatch() calls (each takes
    a slot of the 64-slot ring), then more training — numbers identical to a learner that did the same training without the gathers."""
    A, B, size = 4, 32, 3000
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 821, num_actions=A)
    mem.sync_mirror()
    lib = sd.load()
    nets = []
    for interleave in (0, 1):
        n, _, _ = _net(sd, A, B, 822)
        mt = (C.c_uint32 * 625)(); lib.sdqn_mt_seed(mt, 823)
        random.seed(5)
        for rounds in range(3):
            n.train_from_memory(mem, 1, mt_state=mt, want_cost=False)
            if interleave:
                for _ in range(70):
                    mem.getMinibatch()
            n.train_from_memory(mem, 5, mt_state=mt, want_cost=False)
        nets.append(n)
    for which in (0, 2):
        for i in range(5):
            assert np.array_equal(nets[0].get_layer(i, which), nets[1].get_layer(i, which)), (which, i)


@pytest.mark.gpu
def test_profile_modes_packet_timestamps_against_event_markers(sd):
    """The live per-kernel timing of bench.py's roofline leg: with profile_mode 1 (default) the launch itself records its
    dispatch packet's begin / end timestamps (hipExtLaunchKernel), with 0 hipEventRecord markers bracket it.  Both must
    see every launch of the step; the packet figure is the smaller one (a marker pair adds its own packet processing) and
    must be a plausible kernel time."""
    import simple_dqn_amd as S
    B, A = 32, 4
    args = make_args(batch_size=B)
    mem = S.ReplayMemory(20000, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    net = S.DeepQNetwork(A, args)
    net.update_target_network()
    mt = (C.c_uint32 * 625)(); S.load().sdqn_mt_seed(mt, 11)
    net.train_from_memory(mem, 100, mt_state=mt, want_cost=False); net.sync()
    per = {}
    for mode in (1, 0):
        net.set_option("profile_mode", mode); net.set_option("profile_every", 1)
        net.profile(True, -1); net.profile_reset()
        net.train_from_memory(mem, 200, mt_state=mt, want_cost=False); net.sync()
        per[mode] = {p["name"]: (p["total_ms"] / p["launches"] * 1e3, p["launches"]) for p in net.profile_read() if p["launches"] > 0}
        net.profile(False)
    net.set_option("profile_mode", 1)
    step = [k for k, (us, n) in per[0].items() if n >= 200]
    assert len(step) >= 10, per[0]
    for k in step:
        assert k in per[1] and per[1][k][1] == per[0][k][1], (k, per[1].get(k), per[0][k])
        us1, us0 = per[1][k][0], per[0][k][0]
        assert 1.0 < us1 < 40.0, (k, us1)
        assert us1 < us0 + 0.5, (k, us1, us0)
    assert sum(per[1][k][0] for k in step) < sum(per[0][k][0] for k in step) - 5.0


@pytest.mark.gpu
def test_fp16_write_through_epilogues_keep_the_numbers(sd):
    """float16 mode: the write-through (sc1) epilogue variants of every launch (option wt, default on) store the same values as the
    plain ones — weights, RMSProp state and half copies bit-identical after five steps from a ring, at A = 6."""
    A, B, size = 6, 32, 3000
    args = make_args(batch_size=B, datatype="float16")
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 808, num_actions=A)
    mem.sync_mirror()
    nets = []
    for wt in (511, 0):
        net = sd.DeepQNetwork(A, args)
        net.set_weights(xavier_weights(A, 809), 0)
        net.update_target_network()
        net.set_option("wt", wt)
        mt = (C.c_uint32 * 625)(); sd.load().sdqn_mt_seed(mt, 17)
        net.train_from_memory(mem, 5, mt_state=mt, want_cost=False)
        net.sync()
        nets.append(net)
    for l in range(5):
        assert np.array_equal(nets[0].get_layer(l, 0), nets[1].get_layer(l, 0)), l
        assert np.array_equal(nets[0].get_layer(l, 2), nets[1].get_layer(l, 2)), l
    held = random_minibatch(B, A, 3)[0]
    assert np.array_equal(nets[0].predict(held), nets[1].predict(held))          # (reads the half copies the epilogues refreshed)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(4, 84, 84, "float32"), (3, 60, 52, "float64")])
def test_tuple_api_reuses_the_device_minibatch_only_while_it_is_the_same_data(sd, geom):
    """net.train(mem.getMinibatch()): the gathered states are still on the device, so the step reads them in place instead of uploading
    them again — but only while the host arrays ARE the memory's buffers, nobody has written into them (tracked views) and no other
    gather has replaced the device copy.  Every case must train exactly like a network fed plain copies of the same tuple."""
    hist, H, W, dtype = geom
    A, B, size = 4, 8, 600
    args = make_args(batch_size=B, history_length=hist, screen_height=H, screen_width=W, datatype=dtype)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 901, num_actions=A)
    mem.sync_mirror()
    n1, n2 = sd.DeepQNetwork(A, args), sd.DeepQNetwork(A, args)
    n2.set_weights(n1.get_weights(0), 0); n2.set_weights(n1.get_weights(1), 1)

    def same():
        return all(np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)) for i in range(5))
    random.seed(31)
    mb = mem.getMinibatch()                                       # untouched: device copy reused
    assert not mem._mb_dirty
    ref = tuple(np.array(x) for x in mb)
    n1.train(mb); n2.train(ref)
    assert same()
    mb = mem.getMinibatch()                                       # written through the view before train(): must be uploaded
    mb[0][2, 1] ^= 0x3C
    mem.poststates[5] = 7
    assert mem._mb_dirty
    ref = tuple(np.array(x) for x in mb)
    n1.train(mb); n2.train(ref)
    assert same()
    mb = mem.getMinibatch()                                       # another gather replaces the device copy behind the host arrays' back
    ref = tuple(np.array(x) for x in mb)
    other = np.array([mem.sample_indexes().copy()])
    if (hist, H, W) == (4, 84, 84):
        mem.bench_gather(other, iters=1)
    else:
        sd._lib.check(mem._lib.sdqn_replay_gather(mem._h, sd._lib.ptr(other[0], C.c_int64)))      # device gather without the D2H
    assert not mem._mb_dirty
    n1.train(mb); n2.train(ref)
    assert same()
    mb = mem.getMinibatch()                                       # small arrays are the caller's copies: edits there always count
    mb[2][:] = 3
    ref = tuple(np.array(x) for x in mb)
    n1.train(mb); n2.train(ref)
    assert same()


@pytest.mark.gpu
def test_untouched_tuple_moves_nothing_across_pcie_and_the_bench_legs_report_it(sd):
    """the reference's own loop body net.train(mem.getMinibatch(), epoch) (src/agent.py:112-114) performs ZERO host-to-
    device / device-to-host copies per iteration while the tuple is untouched — sdqn_net_tuple_counters: every call served with the
    states in place on the device AND nothing uploaded — and bench.py's `tuple_api` / `agent_loop` legs (the driver line's keys) report
    exactly that."""
    import random
    import bench
    A, B = 4, 32
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(3000, args)
    synthetic_fill(mem, 77, num_actions=A)
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    random.seed(5)
    for _ in range(25):
        net.train(mem.getMinibatch(), 0)
    assert net.tuple_counters() == (25, 25, 25)
    mb = mem.getMinibatch()
    _ = np.asarray(mb[0])[0, 0, 0, 0]                      # LOOKING at the states fetches them (one D2H) — they are still clean: in place, nothing up
    net.train(mb, 0)
    assert net.tuple_counters() == (26, 26, 26)
    mb = mem.getMinibatch()
    mb[2][0] += 1                                          # an edited reward: the small arrays are uploaded, the states stay in place
    net.train(mb, 0)
    assert net.tuple_counters() == (27, 27, 26)
    leg = bench.tuple_api_leg(sd, make_args, 1, iters=200, warmup=20, ring=3000)
    assert leg["tuple_counters"] == {"calls": 200, "states_in_place_on_device": 200, "nothing_uploaded": 200}
    assert leg["h2d_d2h_copies_per_iteration"] == 0.0 and 10.5 <= leg["launches_per_iteration"] <= 11.5 and leg["value"] > 1000
    ag = bench.agent_loop_leg(sd, make_args, 1, train_steps=800, test_steps=400, random_steps=300)
    assert ag["train_env_steps_per_s"] > 1000 and ag["test_env_steps_per_s"] > 1000


@pytest.mark.gpu
def test_a_pending_minibatch_survives_the_generic_paths_own_gathers(sd):
    """getMinibatch() leaves its states ONLY in the device minibatch until somebody looks.  The generic path (other
    screen geometries, float64) gathers a fused step's states into that very buffer — so train_from_memory / train_indexes / bench_gather
    fetch a pending minibatch to the host first: the tuple still shows, and trains on, its OWN states.  And the C-ABI backstop: declaring
    'the last gather, not fetched' after something overwrote the device minibatch is SDQN_ERR_STATE, never a silent step."""
    import simple_dqn_amd._lib as L
    A, B, size = 4, 8, 500
    args = make_args(batch_size=B, history_length=3, screen_height=60, screen_width=52, datatype="float32")
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 31, num_actions=A)
    mem.sync_mirror()
    net, ref = sd.DeepQNetwork(A, args), sd.DeepQNetwork(A, args)
    assert net.step_structure()[0] == "generic"
    ref.set_weights(net.get_weights(0), 0); ref.set_weights(net.get_weights(1), 1)
    random.seed(9)
    mb = mem.getMinibatch()
    idx = mem.last_indexes.copy()
    screens = np.asarray(mem.screens)
    want_pre = np.stack([screens[i - 3:i] for i in idx])
    step_idx = np.random.RandomState(3).randint(10, 400, size=B).astype(np.int64)
    net.train_indexes(mem, step_idx)                       # the generic path's gather goes through the device minibatch
    ref.train_indexes(mem, step_idx)
    assert np.array_equal(np.asarray(mb[0]), want_pre)     # ... and the pending tuple still shows its own states
    net.train(mb, 0)
    ref.train((want_pre, mb[1].copy(), mb[2].copy(), np.stack([screens[i - 2:i + 1] for i in idx]), mb[4].copy()), 0)
    for i in range(5):
        assert np.array_equal(net.get_layer(i, 0), ref.get_layer(i, 0)), i
    # the backstop at the C ABI: gather, overwrite (another gather launch through the same buffers), then claim the first one unfetched
    lib = sd.load()
    tmem = sd.ReplayMemory(600, make_args(batch_size=B))
    synthetic_fill(tmem, 32, num_actions=A)
    tmem.sync_mirror()
    i1 = np.random.RandomState(4).randint(10, 500, size=B).astype(np.int64)
    L.check(lib.sdqn_replay_gather(tmem._h, L.ptr(i1, C.c_int64)))
    ms = C.c_float()
    L.check(lib.sdqn_replay_bench_gather(tmem._h, L.ptr(i1, C.c_int64), 2, C.byref(ms)))
    assert lib.sdqn_replay_declare_minibatch_on_device(tmem._h, C.c_uint64(0xFFFFFFFFFFFFFFFF)) != 0
    assert b"overwritten" in lib.sdqn_last_error()
