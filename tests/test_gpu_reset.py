"""Periodic resets with shrink-and-perturb (--reset_interval) on the device, against the library's host restatement
(sdqn_reset_apply_host, itself held to tests/reset_oracle.py in tests/test_reset.py) and the oracle, bit for bit.

Shapes: B = 32 and 4 actions throughout — the kernel walks the flat weight buffers and never sees the batch — and what it does depend on is
varied instead: datatype (the derived copies), optimizer (one or two states), fc5's rows (4, 5 with --dueling, 6 with --bootstrap_heads 2),
with and without a target net, and the two shapes of the walked tail: (layers 2, alpha 1) = fc4 and fc5 only, alpha < 1 or layers 5 = everything."""
import random

import numpy as np
import pytest

import redo_oracle as RO
import reset_oracle as O
from oracle.dqn_numpy import OracleDQN, xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

A, B, SEED = 4, 32, 77
CASES = {"f32_rmsprop": ("float32", "rmsprop"), "f32_adam": ("float32", "adam"), "f16_adadelta": ("float16", "adadelta")}
# run one behind the other on one net, events 1, 2, 3: fc4 and fc5 redrawn; fc5 redrawn and the rest shrunk (at layers 5 no layer is left to
# shrink, so the fused multiply-add meets the two nets' different conv weights here); everything redrawn
RULES = ((2, 1.0), (1, 0.25), (5, 0.5))
DORMANT_FC4 = (0, 100, 511)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def make_net(datatype="float32", optimizer="rmsprop", seed=11, num_actions=A, num_outputs=None, dormant=False, **kw):
    import simple_dqn_amd as sd
    net = sd.DeepQNetwork(num_actions, make_args(batch_size=B, datatype=datatype, optimizer=optimizer, **kw))
    n_out = num_actions if num_outputs is None else num_outputs
    ws = xavier_weights(n_out, seed)
    if dormant:                                                # fc4 units that never fire (negative weights on ReLU outputs): ReDo recycles them
        for j in DORMANT_FC4:
            ws[3][j, :] = -np.abs(ws[3][j, :]) - np.float32(1e-3)
    net.set_weights(ws, 0)
    net.set_weights(xavier_weights(n_out, seed + 1), 1)
    return net


def ring(num_actions=A, **kw):
    import simple_dqn_amd as sd
    args = make_args(batch_size=B, replay_size=64, **kw)
    mem = sd.ReplayMemory(64, args)
    synthetic_fill(mem, 5, num_actions=num_actions)
    mem.sync_mirror()
    return mem


def snapshot(net):
    """theta, theta_t, state (, state2) in the flat internal layout"""
    which = [0, 1, 2] + ([4] if net.optimizer != "rmsprop" else [])
    return {w: RO.to_internal(net.get_weights(w)) for w in which}


def host_event(net, before, layers, alpha, event, n_out=A, target=True):
    from simple_dqn_amd.deepqnetwork import reset_apply_host
    got = {w: b.copy() for w, b in before.items()}
    reset_apply_host(layers, alpha, SEED, event, n_out, net.optimizer, got[0], got[1] if target else None, got[2], got.get(4))
    if not target:
        got[1] = got[0]
    return got


_RUNS = {}


def run_case(name):
    """seeded weights, 2 train steps on a 64-slot ring, then the three events — once per case, shared by the tests below"""
    if name in _RUNS:
        return _RUNS[name]
    datatype, optimizer = CASES[name]
    net = make_net(datatype, optimizer)
    random.seed(3)
    net.train_from_memory(ring(), 2)
    r = {"net": net, "snaps": [snapshot(net)], "last": [net.last_reset()]}
    for layers, alpha in RULES:
        net.set_reset(0, layers, alpha, seed=SEED)             # (interval 0: only reset_now resets)
        net.reset_now()
        r["last"].append(net.last_reset())
        r["snaps"].append(snapshot(net))
    r["mb"] = random_minibatch(B, A, 5)
    r["q"] = net.predict(r["mb"][0]).copy()
    r["weights"] = [net.get_weights(0), net.get_weights(1)]
    net.train(r["mb"])
    r["last_q"] = [x.copy() for x in net.last_q()]
    _RUNS[name] = r
    return r


# ---- the event ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2], ids=["layers2_alpha1", "layers1_alpha0.25", "layers5_alpha0.5"])
@pytest.mark.parametrize("name", list(CASES))
def test_event_matches_the_host_restatement(name, k):
    r = run_case(name)
    net, before, after = r["net"], r["snaps"][k], r["snaps"][k + 1]
    layers, alpha = RULES[k]
    assert r["last"][0] == (0, 0) and r["last"][k + 1] == (k + 1, 2)                         # events are numbered; both followed train step 2
    host = host_event(net, before, layers, alpha, k + 1)
    want_w, want_t, want_s = O.apply(layers, alpha, SEED, k + 1, A, before[0], before[1], [before[w] for w in sorted(before) if w >= 2])
    oracle = dict(zip(sorted(before), [want_w, want_t] + want_s))
    m = O.touched(layers, alpha, A)
    assert m.sum() == (3136 * 512 + 512 * A if k == 0 else O.size(A))
    for w in sorted(before):
        assert np.array_equal(bits(after[w]), bits(host[w])), w
        assert np.array_equal(bits(after[w]), bits(oracle[w])), w
        assert np.array_equal(bits(after[w])[~m], bits(before[w])[~m]), w                    # alpha_l == 1: never written
        if w >= 2:
            assert not bits(after[w])[m].any(), w                                            # +0.0 again, sign bit included
            assert k == 2 or bits(before[w])[m].any(), w                                     # (and the optimizer had moved them; event 2 left none moved)
    assert (after[0][m] != before[0][m]).mean() > 0.999                                      # the event did something
    e = O.edges(A)
    first = e[5 - layers]
    assert np.array_equal(bits(after[0][first:]), bits(after[1][first:]))                    # fully reset layers: identical in both nets
    if k < 2:                                                                                # kept or shrunk ones keep their difference
        assert (after[0][:e[3]] != after[1][:e[3]]).mean() > 0.99


@pytest.mark.parametrize("name", ["f32_rmsprop", "f16_adadelta"])
def test_derived_copies_follow(name):
    """what the forward actually reads — conv1's bf16 planes (float32), the half copies (float16), of both nets — was rebuilt: a fresh net
    that is handed the read-back weights through set_weights predicts the same bits, and its target net values the same poststates"""
    r = run_case(name)
    datatype, optimizer = CASES[name]
    fresh = make_net(datatype, optimizer, seed=50)
    fresh.set_weights(r["weights"][0], 0)
    fresh.set_weights(r["weights"][1], 1)
    assert np.array_equal(bits(fresh.predict(r["mb"][0])), bits(r["q"]))
    fresh.train(r["mb"])
    preq, maxq = fresh.last_q()
    assert np.array_equal(bits(preq), bits(r["last_q"][0])) and np.array_equal(bits(maxq), bits(r["last_q"][1]))
    if datatype == "float32":                                  # and the reset net is a net: the numpy forward on the read-back weights
        want = OracleDQN(A, batch_size=B, weights=r["weights"][0]).predict(r["mb"][0])
        err = float(np.abs(r["q"] - want).max())
        print("predict of the reset net against the numpy oracle: max abs error %.3e (bound 1e-4)" % err)
        assert err < 1e-4


def test_without_a_target_net_the_formula_is_applied_once():
    net = make_net(target_steps=0)
    random.seed(3)
    net.train_from_memory(ring(target_steps=0), 2)
    before = snapshot(net)
    assert np.array_equal(bits(before[0]), bits(before[1]))    # which = 1 reads the one buffer
    net.set_reset(0, 1, 0.25, seed=SEED)
    net.reset_now()
    after = snapshot(net)
    host = host_event(net, before, 1, 0.25, 1, target=False)
    for w in (0, 1, 2):
        assert np.array_equal(bits(after[w]), bits(host[w])), w
    want_w, _, _ = O.apply(1, 0.25, SEED, 1, A, before[0])
    assert np.array_equal(bits(after[0]), bits(want_w))
    mb = random_minibatch(B, A, 5)
    fresh = make_net(target_steps=0, seed=50)
    fresh.set_weights(net.get_weights(0), 0)
    assert np.array_equal(bits(fresh.predict(mb[0])), bits(net.predict(mb[0])))


def test_dueling_mask_survives_in_both_nets():
    net = make_net(num_outputs=A + 1, dueling=True)
    net.train(random_minibatch(B, A, 5))
    net.set_reset(0, 2, 1.0, seed=SEED)
    net.reset_now()
    phi = O.draws(SEED, 1, np.arange(O.edges(A + 1)[4], O.edges(A + 1)[5]), 5).reshape(A + 1, 512)
    for which in (0, 1):
        w5 = net.get_layer(4, which)
        assert w5.shape == (A + 1, 512)
        assert not bits(w5[0, 256:]).any() and not bits(w5[1:, :256]).any(), which             # +0.0, sign bit included
        assert np.array_equal(bits(w5[0, :256]), bits(phi[0, :256])) and np.array_equal(bits(w5[1:, 256:]), bits(phi[1:, 256:])), which
    assert (phi[0, 256:] != 0).all() and (np.signbit(phi[0, 256:])).any()                       # the draws there were not zeros: the mask ran


def test_every_fc5_row_of_a_bootstrap_net_is_redrawn():
    net = make_net(num_actions=3, num_outputs=6, bootstrap_heads=2)
    random.seed(3)
    net.train_from_memory(ring(num_actions=3, bootstrap_heads=2), 1)
    before = [net.get_layer(4, w) for w in (0, 1)]
    net.set_reset(0, 2, 1.0, seed=SEED)
    net.reset_now()
    e = O.edges(6)
    phi = O.draws(SEED, 1, np.arange(e[4], e[5]), 5).reshape(6, 512)
    for which in (0, 1):
        w5 = net.get_layer(4, which)
        assert w5.shape == (6, 512) and np.array_equal(bits(w5), bits(phi)), which
        assert all((w5[row] != before[which][row]).mean() > 0.99 for row in range(6)), which


# ---- schedule -----------------------------------------------------------------------------------------------------------------------------
def test_schedule_inside_a_multi_step_call_and_its_place_behind_redo():
    kw = dict(redo_interval=3, redo_threshold=0.1, random_seed=9, dormant=True)
    sched = make_net(reset_interval=3, **kw)
    byhand = make_net(**kw)
    byhand.set_reset(0, 2, 1.0)                                # the same rule and seed, no schedule
    redo_found = []
    assert sched.get_reset() == (3, 2, 1.0, 9) and byhand.get_reset() == (0, 2, 1.0, 9)
    mem = ring()
    random.seed(3)
    sched.train_from_memory(mem, 7)
    assert sched.last_reset() == (2, 6) and sched.last_redo()["event"] == 2
    random.seed(3)
    for t in range(1, 8):
        byhand.train_from_memory(mem, 1)                       # (its ReDo event rides inside steps 3 and 6)
        if t % 3 == 0:
            redo_found.append(byhand.last_redo()["dormant"][3])
            byhand.reset_now()
    assert byhand.last_reset() == (2, 6) and byhand.last_redo()["event"] == 2
    assert redo_found[0] >= len(DORMANT_FC4)                   # ReDo had work in fc4 at step 3: the other order would leave its draws there
    for which in (0, 1, 2):
        a, b = sched.get_weights(which), byhand.get_weights(which)
        for l in range(5):
            assert np.array_equal(bits(a[l]), bits(b[l])), (which, l)


@pytest.mark.parametrize("datatype,optimizer", [("float32", "rmsprop"), ("float16", "adadelta")], ids=["float32", "float16"])
def test_everything_behind_a_step_equals_the_same_calls_by_hand(datatype, optimizer):
    """the order behind an applied step — regulariser, soft target update, ReDo, reset — and the derived copies each of them leaves: a net
    with all four on against one with all off that makes the same calls by hand, on a dueling net with a target net"""
    wd, lam, tau = 0.1, 0.01, 0.01
    kw = dict(num_outputs=A + 1, dueling=True, random_seed=9, dormant=True, learning_rate=0.01)
    P, Q = make_net(datatype, optimizer, **kw), make_net(datatype, optimizer, **kw)
    P.set_regularizer(wd, lam); P.set_target_tau(tau); P.set_redo(1, 0.1); P.set_reset(1, 2, 1.0)
    Q.anchor_now(); Q.set_redo(0, 0.1); Q.set_reset(0, 2, 1.0)     # the same rules and seeds, nothing scheduled
    mem = ring()
    random.seed(3)
    P.train_from_memory(mem, 2)
    random.seed(3)
    for t in (1, 2):
        Q.train_from_memory(mem, 1)
        Q.regularize_now(wd, lam)
        Q.soft_update_target_network(tau)
        Q.redo_now()
        Q.reset_now()
    assert P.last_redo() == Q.last_redo() and P.last_redo()["event"] == 2 and P.last_redo()["step"] == 2
    assert P.last_reset() == Q.last_reset() == (2, 2)
    p, q = snapshot(P), snapshot(Q)
    assert sorted(p) == ([0, 1, 2] if optimizer == "rmsprop" else [0, 1, 2, 4])
    for w in sorted(p):
        assert np.array_equal(bits(p[w]), bits(q[w])), w
    assert (p[0] != p[1]).any()                                    # (the target net is a net of its own: the blend had something to do)
    states = random_minibatch(B, A, 5)[0]
    assert np.array_equal(bits(P.predict(states)), bits(Q.predict(states)))


# ---- off means off ------------------------------------------------------------------------------------------------------------------------
def _profiled_step(net, mem):
    net.profile(True, -1); net.profile_reset()
    random.seed(3)
    net.train_from_memory(mem, 1)
    got = {p["id"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return got


def test_interval_zero_leaves_the_launch_trace_alone():
    """the profiled launches of a default step are the same on a net that was never told about resets, on one whose interval went back to 0,
    and between events; an event adds its one launch to the update slot (the derived-copy launches are set_weights' own, which the profiler
    brackets there as little as here)"""
    UPDATE = 12
    mem = ring()
    plain, back, on = make_net(), make_net(), make_net()
    back.set_reset(3); back.set_reset(0)
    on.set_reset(5)
    assert plain.get_reset()[0] == 0 and back.get_reset()[0] == 0 and on.get_reset()[:3] == (5, 2, 1.0)
    want = _profiled_step(plain, mem)
    assert want[UPDATE] == 1 and sum(want.values()) == 11
    assert _profiled_step(back, mem) == want
    for t in range(1, 5):
        assert _profiled_step(on, mem) == want, t              # steps 1..4 of interval 5: nothing
    event = dict(want); event[UPDATE] += 1
    assert _profiled_step(on, mem) == event                    # step 5: reset_apply_kernel
    assert on.last_reset() == (1, 5) and back.last_reset() == (0, 0) and plain.last_reset() == (0, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_setters_refuse_in_either_order():
    import simple_dqn_amd as sd
    err = (AssertionError, sd.SdqnError)
    net = make_net()
    net.set_reset(5)
    with pytest.raises(err, match="reset_interval"):
        sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
    with pytest.raises(err, match="reset_interval"):          # refused before a communicator is built: the second rank need not exist
        sd._lib.check(net._lib.sdqn_dp_init(net._h, None, bytes(128), 0, 2))
    net.set_reset(0)
    sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
    with pytest.raises(err, match="noisy_nets"):
        net.set_reset(5)
    with pytest.raises(err, match="noisy_nets"):
        net.reset_now()
    for kw, word in ((dict(batch_norm=True), "batch_norm"), (dict(datatype="float64"), "generic"), (dict(screen_height=96, screen_width=96), "generic")):
        other = sd.DeepQNetwork(A, make_args(batch_size=8, **kw))
        with pytest.raises(err, match=word):
            other.set_reset(5)
        with pytest.raises(err, match=word):
            other.reset_now()
    net = make_net()
    for args, word in (((5, 0, 1.0), "reset_layers 0"), ((5, 6, 0.5), "reset_layers"), ((5, 2, 1.5), "shrink_perturb"), ((5, 2, float("nan")), "shrink_perturb"),
                       ((-1, 2, 0.5), "reset_interval")):
        with pytest.raises(err, match=word):
            net.set_reset(*args)
    assert net.get_reset()[0] == 0
    net.set_reset(0, 0, 1.0)                                   # allowed while off ...
    with pytest.raises(err, match="resets nothing"):
        net.reset_now()                                        # ... but an event of it is not
