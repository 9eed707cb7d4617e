"""Decoupled weight decay and L2-init regularisation (--weight_decay, --l2_init) on the device, against the library's host
restatement (sdqn_regularize_apply_host, itself held to tests/regularize_oracle.py in tests/test_regularize.py), bit for bit.

Shapes: B = 4 throughout — the kernels walk the flat weight buffers and never see the batch — and what they do depend on is varied instead:
datatype (which layers go through the tile workgroups, which derived copies are written), fc5's rows (1, 4, 18: the element-wise part's
length), the coefficients (the anchor loads present or not), with and without --target_tau (the fused form).  learning_rate 0.01 so that
kf = 0.999 and cf = 1e-4 move every weight's bits."""
import math
import random

import numpy as np
import pytest

import redo_oracle as RO
import regularize_oracle as O
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

B, LR, SEED = 4, 0.01, 9
COEFFS = [(0.1, 0.0), (0.0, 0.01), (0.1, 0.01)]
UPDATE = 12


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def make_net(datatype="float32", A=4, optimizer="rmsprop", seed=11, num_outputs=None, **kw):
    import simple_dqn_amd as sd
    net = sd.DeepQNetwork(A, make_args(batch_size=B, datatype=datatype, optimizer=optimizer, learning_rate=LR, random_seed=SEED, **kw))
    n_out = A if num_outputs is None else num_outputs
    net.set_weights(xavier_weights(n_out, seed), 0)
    net.set_weights(xavier_weights(n_out, seed + 1), 1)
    return net


def ring(A=4, **kw):
    import simple_dqn_amd as sd
    args = make_args(batch_size=B, replay_size=64, **kw)
    mem = sd.ReplayMemory(64, args)
    synthetic_fill(mem, 5, num_actions=A)
    mem.sync_mirror()
    return mem


def flat(net, which=0):
    return RO.to_internal(net.get_weights(which))


def state_ids(net):
    return [2] + ([4] if net.optimizer != "rmsprop" else [])


def assert_same(p, q, whichs, what=""):
    for w in whichs:
        a, b = p.get_weights(w), q.get_weights(w)
        for l in range(5):
            assert np.array_equal(bits(a[l]), bits(b[l])), (what, w, l)


# ---- 1. regularize_now() against the host restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,lam", COEFFS)
@pytest.mark.parametrize("A", [1, 4, 18])
@pytest.mark.parametrize("datatype", ["float32", "float16"])
def test_regularize_now_matches_the_host_restatement(datatype, A, wd, lam):
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    net = make_net(datatype, A)
    net.set_regularizer(wd, lam)                               # (l2_init > 0: the anchor is taken here ...)
    assert net.last_regularizer() == (wd, lam)
    anchor = flat(net)
    net.set_weights(xavier_weights(A, 30), 0)                  # ... and the weights move away from it
    before, target, state = flat(net), flat(net, 1), flat(net, 2)
    if lam > 0:
        assert np.array_equal(bits(RO.to_internal(net.get_anchor())), bits(anchor))
    net.regularize_now()
    got = flat(net)
    want = before.copy()
    regularize_apply_host(wd, lam, LR, want, anchor if lam > 0 else None)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), bits(O.apply(wd, lam, LR, before, anchor)))
    assert (bits(got) != bits(before)).mean() > 0.99           # every weight's bits moved (up to the odd exact product)
    assert np.array_equal(bits(flat(net, 1)), bits(target)) and np.array_equal(bits(flat(net, 2)), bits(state))      # nothing else did
    # the derived copies the forward reads were rebuilt in the same launch: a fresh net handed the weights predicts the same bits
    states = random_minibatch(B, A, 5)[0]
    fresh = make_net(datatype, A, seed=50)
    fresh.set_weights(net.get_weights(0), 0)
    assert np.array_equal(bits(net.predict(states)), bits(fresh.predict(states)))


# ---- 2. the hook's place --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam", "adadelta"])
def test_the_hook_runs_behind_every_applied_step(optimizer):
    wd, lam = 0.1, 0.01
    P, Q = make_net(optimizer=optimizer), make_net(optimizer=optimizer)
    P.set_regularizer(wd, lam)
    Q.anchor_now()                                             # the same anchor, the flags off
    assert Q.last_regularizer() == (0.0, 0.0)
    mem = ring()
    whichs = [0, 1] + state_ids(P)
    for t in range(3):
        random.seed(100 + t); P.train_from_memory(mem, 1)
        random.seed(100 + t); Q.train_from_memory(mem, 1)
        Q.regularize_now(wd, lam)
        assert_same(P, Q, whichs, t)
    # and inside a multi-step call
    random.seed(7); P.train_from_memory(mem, 3)
    random.seed(7)
    for t in range(3):
        Q.train_from_memory(mem, 1)
        Q.regularize_now(wd, lam)
    assert_same(P, Q, whichs, "multi")


# ---- 3. the fused form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("datatype", ["float32", "float16"])
def test_the_fused_launch_equals_the_two_it_replaces(datatype):
    wd, lam, tau = 0.1, 0.01, 0.05
    P, Q = make_net(datatype, target_tau=tau), make_net(datatype)
    P.set_regularizer(wd, lam)
    Q.anchor_now()
    mem = ring()
    states = random_minibatch(B, 4, 5)[0]
    for t in range(3):
        random.seed(100 + t); P.train_from_memory(mem, 1)
        random.seed(100 + t); Q.train_from_memory(mem, 1)
        Q.regularize_now(wd, lam)
        Q.soft_update_target_network(tau)
        assert_same(P, Q, [0, 1, 2], t)
        assert np.array_equal(bits(P.predict(states)), bits(Q.predict(states))), t
    # the target's derived copies: the next step's targets come from them, so one more plain step on both must agree as well
    P.set_regularizer(0.0, 0.0); P.set_target_tau(0.0)
    random.seed(5); P.train_from_memory(mem, 1)
    random.seed(5); Q.train_from_memory(mem, 1)
    assert_same(P, Q, [0, 1, 2], "after")


# ---- 4. launch counts -----------------------------------------------------------------------------------------------------------------------
def _profiled_step(net, mem):
    net.profile(True, -1); net.profile_reset()
    random.seed(3)
    net.train_from_memory(mem, 1)
    got = {p["id"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return got


def test_launch_counts():
    mem = ring()
    plain, back, on = make_net(), make_net(), make_net()
    back.set_regularizer(0.1, 0.01); back.set_regularizer(0.0, 0.0)
    on.set_regularizer(0.1, 0.01)
    want = _profiled_step(plain, mem)
    assert want[UPDATE] == 1
    assert _profiled_step(back, mem) == want                   # flags at 0: exactly the default step
    step = dict(want); step[UPDATE] += 1
    assert _profiled_step(on, mem) == step                     # on: one launch more, in the update slot
    plain_tau, on_tau = make_net(target_tau=0.05), make_net(target_tau=0.05)
    on_tau.set_regularizer(0.1, 0.01)
    want_tau, got_tau = _profiled_step(plain_tau, mem), _profiled_step(on_tau, mem)
    assert sum(want_tau.values()) == sum(want.values()) + 1    # the blend
    assert sum(got_tau.values()) == sum(want_tau.values())     # the fused launch replaces it: + 0
    assert got_tau == step                                      # (it counts in the update slot; the blend's slot is empty)


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------------
def test_dueling_mask_stays_plus_zero():
    A = 4
    net = make_net(num_outputs=A + 1, dueling=True, target_tau=0.05)
    net.set_regularizer(0.1, 0.01)
    mem = ring()
    random.seed(3)
    net.train_from_memory(mem, 3)
    for which in (0, 1):
        w5 = net.get_layer(4, which)
        assert w5.shape == (A + 1, 512)
        assert not bits(w5[0, 256:]).any() and not bits(w5[1:, :256]).any(), which      # +0.0, sign bit included
        assert w5[0, :256].all() and w5[1:, 256:].all(), which


def test_order_regulariser_blend_redo_reset():
    """P runs everything inside its steps; Q runs plain steps and is handed, after each, what the chain of the host restatements makes of
    its buffers: regulariser -> soft target update -> (step 2) ReDo event -> reset event"""
    from simple_dqn_amd.deepqnetwork import redo_apply_host, regularize_apply_host, reset_apply_host
    wd, lam, tau, A = 0.1, 0.01, 0.05, 4
    P = make_net(target_tau=tau, redo_interval=2, redo_threshold=0.1, reset_interval=2, reset_layers=1, shrink_perturb=0.5)
    Q = make_net()
    P.set_regularizer(wd, lam)
    anchor = flat(Q)
    mem = ring()
    for t in (1, 2):
        random.seed(100 + t); P.train_from_memory(mem, 1)
        random.seed(100 + t); Q.train_from_memory(mem, 1)
        theta, theta_t, state = flat(Q), flat(Q, 1), flat(Q, 2)
        regularize_apply_host(wd, lam, LR, theta, anchor)
        theta_t = O.blend(theta, theta_t, tau)
        if t == 2:
            scores = np.concatenate(list(Q.dormant_scores().values()))
            redo_apply_host(scores, 0.1, SEED, 1, A, theta, state, None)
            reset_apply_host(1, 0.5, SEED, 1, A, "rmsprop", theta, theta_t, state, None)
        for which, buf in ((0, theta), (1, theta_t), (2, state)):
            Q.set_weights(RO.from_internal(buf, A), which)
        assert_same(P, Q, [0, 1, 2], t)
    assert P.last_reset() == (1, 2) and P.last_redo()["event"] == 1
    assert np.array_equal(bits(RO.to_internal(P.get_anchor())), bits(anchor))      # the events did not move the anchor


@pytest.mark.parametrize("kw,memkw", [(dict(clip_grad_norm=10.0), dict()), (dict(n_step=3), dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, n_step=3))],
                         ids=["clip_grad_norm", "per_n_step"])
def test_one_step_with_other_options(kw, memkw):
    wd, lam = 0.1, 0.01
    P, Q = make_net(**kw), make_net(**kw)
    P.set_regularizer(wd, lam)
    Q.anchor_now()
    mp, mq = ring(**memkw), ring(**memkw)
    random.seed(3); P.train_from_memory(mp, 1)
    random.seed(3); Q.train_from_memory(mq, 1)
    Q.regularize_now(wd, lam)
    assert_same(P, Q, [0, 1, 2])


# ---- 6. weight_norms() ----------------------------------------------------------------------------------------------------------------------
def test_weight_norms():
    A = 4
    net = make_net(A=A)
    e = O.edges(A)
    counts = [e[l + 1] - e[l] for l in range(5)]

    def check(got, want):
        for l in range(5):
            rel = abs(got[l] - want[l]) / want[l] if want[l] else abs(got[l])
            print("layer %d: n %d, device %.17g, fsum %.17g, relative difference %.3e (bound %.3e)" % (l + 1, counts[l], got[l], want[l], rel, (counts[l] - 1) * 2.0 ** -53))
            assert rel <= (counts[l] - 1) * 2.0 ** -53, l

    n1, d1 = net.weight_norms(squared=True)
    n2, d2 = net.weight_norms(squared=True)
    assert np.array_equal(n1.view(np.uint64), n2.view(np.uint64))      # the same weights, the same bits
    assert np.isnan(d1).all() and np.isnan(d2).all()                    # no anchor yet
    want_n, _ = O.sums(flat(net), None, A)
    check(n1, want_n)
    norms, dists = net.weight_norms()
    assert np.array_equal(norms, np.sqrt(n1)) and np.isnan(dists).all()
    net.anchor_now()
    anchor = flat(net)
    n3, d3 = net.weight_norms(squared=True)
    assert np.array_equal(n3.view(np.uint64), n1.view(np.uint64)) and not d3.view(np.uint64).any()      # distances exactly +0.0
    net.regularize_now(0.1, 0.0)
    n4, d4 = net.weight_norms(squared=True)
    n5, d5 = net.weight_norms(squared=True)
    assert np.array_equal(n4.view(np.uint64), n5.view(np.uint64)) and np.array_equal(d4.view(np.uint64), d5.view(np.uint64))
    want_n, want_d = O.sums(O.apply(0.1, 0.0, LR, anchor), anchor, A)
    check(n4, want_n)
    check(d4, want_d)
    assert all(x > 0 for x in d4) and all(math.isfinite(x) for x in d4)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_setters_refuse_in_either_order():
    import simple_dqn_amd as sd
    err = (AssertionError, sd.SdqnError)
    for coeffs, word in (((0.1, 0.0), "weight_decay"), ((0.0, 0.01), "l2_init")):
        net = make_net()
        net.set_regularizer(*coeffs)
        with pytest.raises(err, match=word):
            sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
        with pytest.raises(err, match=word):                   # refused before a communicator is built: the second rank need not exist
            sd._lib.check(net._lib.sdqn_dp_init(net._h, None, bytes(128), 0, 2))
        net.set_regularizer(0.0, 0.0)
        sd._lib.check(net._lib.sdqn_net_set_noisy(net._h, 1, 0.5, 0))
        with pytest.raises(err, match="noisy_nets"):
            net.set_regularizer(*coeffs)
        with pytest.raises(err, match="noisy_nets"):
            net.regularize_now(*coeffs)
        assert net.last_regularizer() == (0.0, 0.0)
    for kw, word in ((dict(batch_norm=True), "batch_norm"), (dict(datatype="float64"), "generic"), (dict(screen_height=96, screen_width=96), "generic")):
        other = sd.DeepQNetwork(4, make_args(batch_size=8, **kw))
        for call in (lambda: other.set_regularizer(0.1, 0.0), lambda: other.set_regularizer(0.0, 0.01), lambda: other.regularize_now(0.1, 0.0),
                     other.anchor_now, other.weight_norms):
            with pytest.raises(err, match=word):
                call()
        other.set_regularizer(0.0, 0.0)                        # off is always allowed
    net = make_net()
    for coeffs, word in (((-0.1, 0.0), "weight_decay"), ((float("nan"), 0.0), "weight_decay"), ((100.0, 0.0), "weight_decay"),
                         ((0.0, -1.0), "l2_init"), ((0.0, float("nan")), "l2_init"), ((0.0, 100.5), "l2_init")):
        with pytest.raises(err, match=word):
            net.set_regularizer(*coeffs)
    assert net.last_regularizer() == (0.0, 0.0)
    with pytest.raises(err, match="anchor"):
        net.regularize_now(0.0, 0.01)                          # no anchor yet
    with pytest.raises(err, match="anchor"):
        net.get_anchor()
