"""Dormant-neuron recycling (--redo_interval) on the device, against tests/redo_oracle.py and the library's host
restatement.  Dormancy is planted without rounding: the incoming weights of chosen units are all negative and every layer's inputs are
non-negative (pixels, ReLU outputs; the net has no biases), so those units' activations are exactly 0 on any state.

Shapes: the smallest batch of each launch regime (float32 B = 32 and B = 128, float16 B = 32) and float32 B = 33, where no row count of the
score reduction is a multiple of a chunk; A = 4."""
import random

import numpy as np
import pytest

import redo_oracle as O
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

A = 4
PLANTED = ((0, 5, 17, 31), (0, 9, 40, 63), (0, 21, 63), (0, 100, 255, 256, 511))      # per layer; the first and last unit of each among them
ROWS = (400, 81, 49, 1)
CASES = {"f32_b32": ("float32", 32, {}), "f32_b33_adam": ("float32", 33, dict(optimizer="adam")), "f32_b128": ("float32", 128, {}),
         "f16_b32": ("float16", 32, {})}
FP16_BOUND = 3e-3          # the project's float16 parity bound on forward outputs (TM.CONFIGS fp16_b32: Q within 3e-3)


def planted_weights(seed, num_outputs=A):
    """Xavier draws whose incoming weights per unit are moved to a small positive mean (k / 20), so that on the tests' random-noise frames —
    where a unit with a negative weight sum is silent on every patch — every unit fires, except the planted ones"""
    ws = xavier_weights(num_outputs, seed)
    for l in range(4):
        axis = 0 if l < 3 else 1
        k = np.float32(np.sqrt(3.0 / ws[l].shape[axis]))
        ws[l] = (ws[l] - ws[l].mean(axis=axis, keepdims=True) + k / np.float32(20.0)).astype(np.float32)
    for l in range(3):
        for j in PLANTED[l]:
            ws[l][:, j] = -np.abs(ws[l][:, j]) - np.float32(1e-3)
    for j in PLANTED[3]:
        ws[3][j, :] = -np.abs(ws[3][j, :]) - np.float32(1e-3)
    return ws


def planted_mask():
    m = np.zeros(672, bool)
    for l in range(4):
        m[[O.EDGES[l] + j for j in PLANTED[l]]] = True
    return m


def make_net(datatype, B, seed=11, num_outputs=A, **kw):
    import simple_dqn_amd as sd
    net = sd.DeepQNetwork(kw.pop("num_actions", A), make_args(batch_size=B, datatype=datatype, **kw))
    net.set_weights(planted_weights(seed, num_outputs), 0)
    net.set_weights(xavier_weights(num_outputs, seed + 1), 1)
    return net


def read_acts(net, B):
    """the online net's prestate half of a1..a4 as [rows][units] float32 (float32 nets)"""
    out = []
    for l, name in enumerate(("a1", "a2", "a3", "a4")):
        n = B * ROWS[l] * O.UNITS[l]
        out.append(net.debug_read(name, n).reshape(B * ROWS[l], O.UNITS[l]))
    return out


def flat_scores(net):
    return np.concatenate(list(net.dormant_scores().values()))


def snapshot(net):
    which = [0, 1, 2] + ([4] if net.optimizer != "rmsprop" else [])
    return {w: net.get_weights(w) for w in which}


_RUNS = {}


def run_case(name):
    """one train step, the read-outs, one recycle event with tau = 0 — once per case, shared by the tests below"""
    if name in _RUNS:
        return _RUNS[name]
    datatype, B, kw = CASES[name]
    net = make_net(datatype, B, **kw)
    mb = random_minibatch(B, A, 5)
    net.train(mb)
    r = {"net": net, "B": B, "mb": mb}
    r["scores"] = flat_scores(net)
    r["scores_again"] = flat_scores(net)
    if datatype == "float32":
        r["acts"] = read_acts(net, B)
    r["before"] = snapshot(net)
    net.set_redo(0, 0.0, seed=77)                              # (interval 0: only redo_now recycles; tau = 0: exactly silent units)
    net.redo_now()
    r["last"] = net.last_redo()
    r["after"] = snapshot(net)
    r["q_after"] = net.predict(mb[0]).copy()
    net.set_weights(r["before"][0], 0)                         # the online weights as they were: the same forward before the event
    r["q_before"] = net.predict(mb[0]).copy()
    _RUNS[name] = r
    return r


# ---- scores -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32_b32", "f32_b33_adam", "f32_b128"])
def test_scores_match_the_oracle(name):
    """rows * 2^-52 relative: the bound on an fp64 sum of `rows` terms in any order.  The library hands the score out as float32, so the
    bound is applied before that rounding: float32(s (1 - tol)) <= score <= float32(s (1 + tol)) with the oracle's float64 s."""
    r = run_case(name)
    want = O.scores64(r["acts"])
    worst = 0.0
    for l in range(4):
        got = r["scores"][O.EDGES[l]:O.EDGES[l + 1]]
        tol = r["B"] * ROWS[l] * 2.0 ** -52
        lo, hi = (want[l] * (1.0 - tol)).astype(np.float32), (want[l] * (1.0 + tol)).astype(np.float32)
        err = np.abs(got.astype(np.float64) - want[l]) / np.maximum(want[l], 1e-300)
        worst = max(worst, float(err[want[l] > 0].max()))
        print("%s layer %d: rows %d, tol %.3e, largest relative distance of the float32 score from the float64 oracle %.3e"
              % (name, l + 1, r["B"] * ROWS[l], tol, float(err[want[l] > 0].max())))
        assert ((got >= lo) & (got <= hi)).all(), (l, np.nonzero(~((got >= lo) & (got <= hi)))[0][:8])
    assert worst < 2.0 ** -23                                  # (float32 rounding of the hand-out itself)
    assert not r["scores"][planted_mask()].any()               # planted units: exactly 0
    for l in range(4):                                         # a layer's scores average 1
        assert abs(float(r["scores"][O.EDGES[l]:O.EDGES[l + 1]].astype(np.float64).mean()) - 1.0) < 1e-6


@pytest.mark.parametrize("name", list(CASES))
def test_scores_are_bit_equal_between_runs(name):
    r = run_case(name)
    assert np.array_equal(r["scores"].view(np.uint32), r["scores_again"].view(np.uint32))
    datatype, B, kw = CASES[name]
    net2 = make_net(datatype, B, **kw)                         # a second net, the same step: the same bits
    net2.train(r["mb"])
    assert np.array_equal(flat_scores(net2).view(np.uint32), r["scores"].view(np.uint32))


def test_float16_scores_follow_the_float32_run():
    h, f = run_case("f16_b32"), run_case("f32_b32")
    assert not h["scores"][planted_mask()].any()
    live = ~planted_mask()
    rel = np.abs(h["scores"][live].astype(np.float64) - f["scores"][live]) / f["scores"][live]
    print("float16 vs float32 scores: largest relative difference %.3e (bound %.1e)" % (float(rel.max()), FP16_BOUND))
    assert (f["scores"][live] > 0).all() and float(rel.max()) <= FP16_BOUND


# ---- recycle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_recycle_event(name):
    from simple_dqn_amd.deepqnetwork import redo_apply_host
    r = run_case(name)
    net, before, after = r["net"], r["before"], r["after"]
    d = np.concatenate(O.dormant(r["scores"], 0.0))
    assert np.array_equal(d, planted_mask())                   # the recycled set is exactly the planted set
    assert r["last"] == {"event": 1, "step": 1, "dormant": tuple(len(p) for p in PLANTED)}
    # the host restatement on the same scores, in the internal layouts
    theta, state = O.to_internal(before[0]), O.to_internal(before[2])
    state2 = O.to_internal(before[4]) if 4 in before else None
    counts = redo_apply_host(r["scores"], 0.0, 77, 1, A, theta, state, state2)
    assert tuple(int(c) for c in counts) == r["last"]["dormant"]
    host = O.from_internal(theta, A)
    want_w, want_s, masks = O.apply(r["scores"], 0.0, 77, 1, before[0], [before[w] for w in sorted(before) if w >= 2])
    for l in range(5):
        red, zer = masks[l]["redrawn"], masks[l]["zeroed"]
        kept = ~(red | zer)
        assert np.array_equal(after[0][l].view(np.uint32), host[l].view(np.uint32)), l          # incoming draws: the host's, bit for bit
        assert np.array_equal(after[0][l].view(np.uint32), want_w[l].view(np.uint32)), l          # ... and the oracle's
        assert not after[0][l].view(np.uint32)[zer].any(), l                                      # outgoing entries: +0.0
        assert np.array_equal(after[0][l].view(np.uint32)[kept], before[0][l].view(np.uint32)[kept]), l
        assert np.array_equal(after[1][l].view(np.uint32), before[1][l].view(np.uint32)), l       # the target net: untouched
        for k, w in enumerate(w for w in sorted(before) if w >= 2):
            assert not after[w][l].view(np.uint32)[~kept].any(), (w, l)                           # optimizer state: fresh
            assert np.array_equal(after[w][l].view(np.uint32)[kept], before[w][l].view(np.uint32)[kept]), (w, l)
            assert np.array_equal(after[w][l].view(np.uint32), want_s[k][l].view(np.uint32)), (w, l)
    assert masks[0]["redrawn"].sum() == 256 * len(PLANTED[0]) and masks[4]["zeroed"].sum() == A * len(PLANTED[3])
    # a silent unit contributed 0 and a zeroed fan-out contributes 0: the same Q-values, bit for bit
    assert np.array_equal(r["q_after"].view(np.uint32), r["q_before"].view(np.uint32))


def test_read_outs_need_the_last_steps_activations():
    import simple_dqn_amd as sd
    net = make_net("float32", 32)
    with pytest.raises((AssertionError, sd.SdqnError)):
        net.dormant_scores()                                   # before any train step
    with pytest.raises((AssertionError, sd.SdqnError)):
        net.redo_now()
    assert net.last_redo() == {"event": 0, "step": 0, "dormant": (0, 0, 0, 0)}
    mb = random_minibatch(32, A, 5)
    net.train(mb)
    net.predict(mb[0])                                         # a forward of its own overwrites them
    with pytest.raises((AssertionError, sd.SdqnError)):
        net.dormant_scores()
    net.train(mb)
    assert len(net.dormant_fraction(0.0)) == 4 and net.dormant_fraction(0.0)[0] == len(PLANTED[0]) / 32.0


# ---- schedule -----------------------------------------------------------------------------------------------------------------------------
def _ring(B, **kw):
    import simple_dqn_amd as sd
    args = make_args(batch_size=B, replay_size=64, **kw)
    mem = sd.ReplayMemory(64, args)
    synthetic_fill(mem, 5, num_actions=A)
    mem.sync_mirror()
    return mem, args


def test_schedule_inside_a_multi_step_call():
    mem, _ = _ring(32)
    nets = [make_net("float32", 32, redo_interval=3, redo_threshold=0.1), make_net("float32", 32, redo_interval=3, redo_threshold=0.1),
            make_net("float32", 32)]
    random.seed(3)
    nets[0].train_from_memory(mem, 7)
    assert nets[0].last_redo()["event"] == 2 and nets[0].last_redo()["step"] == 6
    random.seed(3)
    for t in range(7):
        nets[1].train_from_memory(mem, 1)
        assert nets[1].last_redo()["event"] == (t + 1) // 3
    random.seed(3)
    nets[2].train_from_memory(mem, 7)
    w = [n.get_weights(0) for n in nets]
    for l in range(5):
        assert np.array_equal(w[0][l].view(np.uint32), w[1][l].view(np.uint32)), l
    assert not np.array_equal(w[0][0], w[2][0])                # the events did something: the planted conv1 columns were redrawn
    for j in PLANTED[0]:
        assert (w[2][0][:, j] < 0).all() and not (w[0][0][:, j] < 0).all()


# ---- composition --------------------------------------------------------------------------------------------------------------------------
def test_composes_with_dueling():
    net = make_net("float32", 32, num_outputs=A + 1, dueling=True)
    net.train(random_minibatch(32, A, 5))
    net.set_redo(0, 0.0, seed=77)
    net.redo_now()
    assert net.last_redo()["dormant"] == tuple(len(p) for p in PLANTED)
    w5 = net.get_layer(4, 0)
    assert w5.shape == (A + 1, 512)
    assert not w5[0, 256:].view(np.uint32).any() and not w5[1:, :256].view(np.uint32).any()      # the mask's entries are still +0.0
    for j in PLANTED[3]:
        assert not w5[:, j].view(np.uint32).any()              # column j of the V row and of the advantage rows
    assert w5[0, :256].any() and w5[1:, 256:].any()


def test_composes_with_prioritized_n_step():
    kw = dict(prioritized_replay=True, n_step=3, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000)
    mem, _ = _ring(32, **kw)
    net = make_net("float32", 32, redo_interval=1, redo_threshold=0.0, **kw)
    random.seed(3)
    net.train_from_memory(mem, 1)
    plain_mem, _ = _ring(32)
    plain = make_net("float32", 32, redo_interval=1, redo_threshold=0.0)
    random.seed(3)
    plain.train_from_memory(plain_mem, 1)
    assert net.last_redo() == plain.last_redo() == {"event": 1, "step": 1, "dormant": tuple(len(p) for p in PLANTED)}


def test_setters_refuse_in_either_order():
    import simple_dqn_amd as sd
    net = make_net("float32", 32)
    net.set_redo(5)
    with pytest.raises((AssertionError, sd.SdqnError), match="redo_interval"):
        sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
    net.set_redo(0)
    sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
    with pytest.raises((AssertionError, sd.SdqnError), match="noisy_nets"):
        net.set_redo(5)
    for kw, word in ((dict(batch_norm=True), "batch_norm"), (dict(datatype="float64"), "generic"), (dict(screen_height=42, screen_width=42), "generic")):
        other = sd.DeepQNetwork(A, make_args(batch_size=8, **kw))
        with pytest.raises((AssertionError, sd.SdqnError), match=word):
            other.set_redo(5)
        with pytest.raises((AssertionError, sd.SdqnError), match=word):
            other.dormant_scores()
    with pytest.raises((AssertionError, sd.SdqnError), match="redo_threshold"):
        make_net("float32", 32).set_redo(5, 1.0)


# ---- interval 0 ---------------------------------------------------------------------------------------------------------------------------
def _profiled_step(net, mem):
    net.profile(True, -1); net.profile_reset()
    random.seed(3)
    net.train_from_memory(mem, 1)
    got = {p["id"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return got


def test_interval_zero_leaves_the_launch_trace_alone():
    """the profiled launches of a default step (what tests/test_gpu_launch_route.py holds to the resolver) are the same on a net that was
    never told about recycling, on one whose interval went back to 0, and between events; an event adds its three launches to the update slot"""
    UPDATE = 12
    mem, _ = _ring(32)
    plain, back, on = make_net("float32", 32), make_net("float32", 32), make_net("float32", 32)
    back.set_redo(3); back.set_redo(0)
    on.set_redo(2, 0.1)
    want = _profiled_step(plain, mem)
    assert want == {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 16: 1, 17: 1, 18: 1, UPDATE: 1, 15: 1}
    assert _profiled_step(back, mem) == want
    assert _profiled_step(on, mem) == want                     # step 1 of interval 2: nothing
    event = dict(want); event[UPDATE] += 3
    assert _profiled_step(on, mem) == event                    # step 2: two score launches and the apply launch
    assert on.last_redo()["event"] == 1 and back.last_redo()["event"] == 0
