"""--noisy_nets on the device against tests/noisy_oracle.py: composition bit for bit, the noise against its host restatement,
step parity at the bounds of the default step's tests (tests/test_gpu_dqn.py, test_gpu_optimizers.py, test_gpu_head_edges.py: Q 1e-4,
every gradient element 1e-4 of its layer's largest, weights 2e-5 where the gradient is not round-off-small, optimizer state 1e-3),
sigma = 0 as the plain step, the target copy, the acting paths by phase, the launch census, stale buffers, stability and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noisy_oracle as N  # noqa: E402
from collect_oracle import CollectOracle  # noqa: E402
from oracle.dqn_numpy import xavier_weights  # noqa: E402
from oracle.replay_numpy import synthetic_fill  # noqa: E402
from util import make_args, random_minibatch  # noqa: E402

pytestmark = pytest.mark.gpu
Q_TOL = 1e-4          # tests/test_gpu_dqn.py
SEED = 123            # make_args' random_seed
SHAPES = [(2, 4), (32, 4), (33, 4), (128, 4), (32, 3), (32, 18)]      # the batch-regime edges and the action-count buckets


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(B, **kw):
    d = dict(batch_size=B, noisy_nets=True, noisy_sigma=0.5)
    d.update(kw)
    return make_args(**d)


def _pair(sd, A, B, seed, oracle=N.NoisyOracle, **kw):
    """a noisy net and its oracle from the same two Xavier draws.  The oracle composes the effective weights in float32 (bit for bit the
    device's: test_composition_bit_for_bit_and_noise_against_the_host) and runs forward, backward and optimizer in float64, as the free-running
    references of DESIGN.md 28.3 / 32.3 do: a float32 reference flips Rectlin gates of its own.  Measured at B = 128, step 2: ONE a2 gate
    (sample 12, position 49, map 5) open at 1.49e-8 in a float32 oracle and closed on the device and in float64; that alone put the conv2
    gradient 1.2e-2 apart (largest element 2.05) and Q 2.6e-4 apart a step later, while float64 and the device agree on every gate."""
    args = _args(B, **kw)
    net = sd.DeepQNetwork(A, args)
    ws, wt = xavier_weights(A, seed), xavier_weights(A, seed + 1)
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    o = oracle(A, batch_size=B, weights=ws, optimizer=args.optimizer, dtype=np.float64).init_noisy(args.noisy_sigma)
    o.Wt = [np.array(w, dtype=np.float64) for w in wt]
    return net, o


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _host_eps(step, slot, A):
    """the host restatement's factor vectors of (SEED, step, slot)"""
    z = dict((k, sd_noise(step, slot, l, s, n)) for (l, s), n in N.sizes(A).items() for k in [("in4", "out4", "in5", "out5")[2 * l + s]])
    return dict((k, N.factor(v)) for k, v in z.items())


def sd_noise(step, slot, layer, side, n):
    from simple_dqn_amd.deepqnetwork import noisy_noise
    return noisy_noise(SEED, step, slot, layer, side, n)


def _check_step(net, o, mb, epoch=0, label=""):
    """one step, first or free-running: Q, gradients of mu and sigma, mu, sigma and the optimizer state against the oracle fed the device's
    noise, every one at the named tests' bounds.  The oracle runs in float64 (see _pair): measured at B = 128 against it, three free-running
    steps keep Q within 3e-7, every gradient element within 3e-6 and mu / sigma within 1.1e-8."""
    net.train(mb, epoch)
    return _compare(net, o, mb, epoch, label)


def _gates_apart(net, o, B):
    """Rectlin gates of a1 / a2 on which the device and the oracle's last online forward disagree, with both values (a miss's first suspect)"""
    out = []
    for name, li, pix, k in (("a1", 1, 400, 32), ("a2", 2, 81, 64)):
        dev = net.debug_read(name, 2 * B * pix * k).reshape(2, B, pix, k)[0]
        ref = o.last_acts[li].reshape(B, k, pix).transpose(0, 2, 1)
        for m in np.argwhere((dev > 0) != (ref > 0))[:8]:
            out.append("%s%s device %.3e oracle %.3e" % (name, tuple(int(x) for x in m), dev[tuple(m)], ref[tuple(m)]))
    return out


def _compare(net, o, mb, epoch=0, label=""):
    """the step the net has just run on mb, restated by the oracle and compared (both optimizer states where the rule has two).  Every
    figure is printed before anything is asserted; a miss reports the Rectlin gates on which device and oracle disagree."""
    B = mb[0].shape[0]
    eps = net.noisy_eps()
    # gates within round-off of zero go the device's way (tests/noisy_oracle.py: follow); at most a handful per step, each printed
    o.follow = dict((li, net.debug_read(name, 2 * B * pix * k).reshape(2, B, pix, k)[0].transpose(0, 2, 1))
                    for name, li, pix, k in (("a1", 1, 400, 32), ("a2", 2, 81, 64), ("a3", 3, 49, 64)))
    g, gs, cost, preq = o.noisy_train(mb, eps[0], eps[1], epoch)
    o.follow = None
    print("%s gates followed: %s" % (label, o.followed))
    assert len(o.followed) <= 4, o.followed
    q, _ = net.last_q()
    rows = [("Q", float(np.abs(q - preq).max()), Q_TOL)]
    for i in range(5):
        rows.append(("grad layer %d" % i, float(np.abs(net.get_layer(i, which=3) - g[i]).max()), 1e-4 * max(1e-3, float(np.abs(g[i]).max()))))
        big = np.abs(g[i]) / B > 1e-6
        if big.any():
            rows.append(("mu layer %d" % i, float(np.abs(net.get_layer(i, 0) - o.W[i])[big].max()), 2e-5))
        rows.append(("state layer %d" % i, float(np.abs(net.get_layer(i, 2) - o.S[i]).max()), 1e-6 + 1e-3 * float(np.abs(o.S[i]).max())))
        if o.optimizer != "rmsprop":
            rows.append(("second state layer %d" % i, float(np.abs(net.get_layer(i, 4) - o.S2[i]).max()), 1e-6 + 1e-3 * float(np.abs(o.S2[i]).max())))
    dgs, sig = net.noisy_fc("noisy_sigma_grad"), net.get_noisy_sigma(0)
    for k in range(2):
        rows.append(("sigma grad fc%d" % (4 + k), float(np.abs(dgs[k] - gs[k]).max()), 1e-4 * max(1e-3, float(np.abs(gs[k]).max()))))
        big = np.abs(gs[k]) / B > 1e-6
        if big.any():
            rows.append(("sigma fc%d" % (4 + k), float(np.abs(sig[k] - o.sigma[k])[big].max()), 2e-5))
    for name, err, bound in rows:
        print("%s %s: max abs err %.3e (bound %.3e)" % (label, name, err, bound))
    misses = ["%s %.3e >= %.3e" % r for r in rows if not r[1] < r[2]]
    if misses:
        gates = _gates_apart(net, o, B)
        print("%s gates apart: %s" % (label, gates))
        raise AssertionError("%s: %s; Rectlin gates apart: %s" % (label, "; ".join(misses), gates or "none"))
    return eps


# ---- 1, 2: composition and noise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", SHAPES)
def test_composition_bit_for_bit_and_noise_against_the_host(sd, B, A):
    net, _ = _pair(sd, A, B, 11)
    net.train(random_minibatch(B, A, 12))
    assert net.noisy_step() == 1
    eps = net.noisy_eps()
    for z, name in ((0, "noisy_theta"), (1, "noisy_theta_t")):
        w = net.get_weights(z)
        s4, s5 = net.get_noisy_sigma(z)
        e4, e5 = N.compose(w[3], w[4], s4, s5, eps[z])[:2]
        got4, got5 = net.noisy_fc(name)
        assert _bits(got4, e4) and _bits(got5, e5), name
        assert not _bits(got4, w[3])
        nconv = sum(x.size for x in w[:3])
        conv = net.debug_read(name, nconv)
        assert z == 1 or _bits(conv, net.debug_read("theta", nconv))
        assert _bits(conv[:w[0].size].reshape(w[0].shape), w[0])       # (conv1 lies in the flat buffers as get_weights returns it)
        if z == 1:                                                     # the target's conv slices are theta_t's, not the online net's
            assert not _bits(conv, net.debug_read("theta", nconv))
            net.update_target_network()                                # ... and follow a hard copy through the stale mark
            assert _bits(net.debug_read(name, nconv), net.debug_read("theta", nconv))
    assert not np.array_equal(eps[0]["in4"], eps[1]["in4"]) and not np.array_equal(eps[0]["out5"], eps[1]["out5"])
    worst = 0.0
    for z in (0, 1):
        for (layer, side), n in N.sizes(A).items():
            e = eps[z][("in4", "out4", "in5", "out5")[2 * layer + side]]
            zdev = np.sign(e) * e * e
            worst = max(worst, float(np.abs(zdev - sd_noise(1, z, layer, side, n)).max()))
    print("B %d A %d: device z against sdqn_noisy_noise, max abs err %.3e" % (B, A, worst))
    assert worst < 1e-5


# ---- 3: parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", SHAPES)
def test_one_and_three_free_running_steps(sd, B, A):
    net, o = _pair(sd, A, B, 21)
    net.set_option("keep_gradients", 1)
    for s in range(3):
        _check_step(net, o, random_minibatch(B, A, 22 + s, p_term=0.05, reward_range=(-1, 2)), label="B %d A %d step %d" % (B, A, s + 1))
    hold = random_minibatch(B, A, 29)[0]
    assert np.abs(net.predict(hold) - o.predict(hold)).max() < Q_TOL


@pytest.mark.parametrize("opt", ["adam", "adadelta"])
def test_every_optimizer(sd, opt):
    """1 and 3 free-running steps (epochs 0, 0, 1) under Adam and Adadelta: every quantity of _check_step on every step, both optimizer
    states of mu included; sigma's own two states are held through sigma itself, which a wrong second state or lr_t moves by a whole
    update (Adam: lr_t, 2.5e-4 a step) against the 2e-5 bound"""
    A, B = 4, 32
    net, o = _pair(sd, A, B, 31, optimizer=opt)
    net.set_option("keep_gradients", 1)
    for s, epoch in enumerate((0, 0, 1)):
        eps = _check_step(net, o, random_minibatch(B, A, 32 + s, p_term=0.05, reward_range=(-1, 2)), epoch, label="%s step %d" % (opt, s + 1))
    hold = random_minibatch(B, A, 39)[0]
    assert np.abs(net.predict_noisy(hold) - o.predict_noisy(hold, eps[0])).max() < Q_TOL
    assert np.abs(net.predict(hold) - o.predict(hold)).max() < Q_TOL


def test_double_dqn_parity(sd):
    A, B = 4, 32
    net, o = _pair(sd, A, B, 41, oracle=N.NoisyOracleDDQN, double_dqn=True)
    net.set_option("keep_gradients", 1)
    for s in range(2):
        _check_step(net, o, random_minibatch(B, A, 42 + s, p_term=0.05, reward_range=(-1, 2)), label="double_dqn step %d" % (s + 1))


def test_n_step_parity(sd):
    """--n_step 3 through the tuple API (float64 returns, done flags, gamma^3): 1 and 3 free-running steps at B = 32"""
    A, B, n = 4, 32, 3
    net, o = _pair(sd, A, B, 45, oracle=N.NoisyOracleNStep, n_step=n)
    o.n_step = n
    net.set_option("keep_gradients", 1)
    for s in range(3):
        pre, act, _, post, done = random_minibatch(B, A, 46 + s, p_term=0.05)
        r = np.random.RandomState(146 + s).randint(-1, 2, (B, n)).astype(np.float64)
        R = r[:, 0] + 0.99 * r[:, 1] + (0.99 * 0.99) * r[:, 2]
        _check_step(net, o, (pre, act, R, post, done), label="n_step 3 step %d" % (s + 1))


def test_prioritized_replay_parity_and_priorities(sd):
    """--prioritized_replay through the library's loop at B = 32, three steps: the stratified draw and importance weights of
    tests/test_gpu_per.py's test_one_step, the weighted step at _check_step's bounds, and the priorities written back (1e-5 relative,
    as there) — the TD errors behind them come from the noisy forward"""
    import random
    import per_oracle as P
    from oracle.replay_numpy import ReplayOracle
    ALPHA, EPS, A, B, size = 0.6, 1e-6, 4, 32, 3000
    args = _args(B, prioritized_replay=True, priority_alpha=ALPHA, priority_beta=0.4, priority_beta_steps=1000, priority_epsilon=EPS)
    mem = sd.ReplayMemory(size, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    omem = ReplayOracle(size, batch_size=B)
    synthetic_fill(omem, 3, num_actions=A)
    mem.set_priorities(0, (10.0 ** np.random.RandomState(3).uniform(-2, 1, size)).astype(np.float32))
    net, o = _pair(sd, A, B, 47, oracle=N.NoisyOraclePER, **{k: getattr(args, k) for k in ("prioritized_replay", "priority_alpha", "priority_beta",
                                                                                           "priority_beta_steps", "priority_epsilon")})
    net.set_option("keep_gradients", 1)
    random.seed(21)
    for s in range(3):
        leaf = mem.priorities()
        st = random.getstate()
        net.train_from_memory(mem, 1)
        idx, w = mem.last_sample()
        r = random.Random(); r.setstate(st)
        assert np.array_equal(idx, P.sample(leaf, P.uniforms(r, B)))
        assert w.min() < 0.5                                               # (the weights are spread: ignoring them fails below)
        o.weights = w
        _compare(net, o, omem.gather(idx), label="prioritized step %d" % (s + 1))
        newp, pr = P.new_priority(o.last_abs_delta, ALPHA, EPS), mem.priorities()
        last = {int(i): k for k, i in enumerate(idx)}
        np.testing.assert_allclose(np.array([pr[i] for i in last]), np.array([newp[k] for k in last.values()]), rtol=1e-5)


# ---- 4: sigma = 0 is the plain step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 128])
def test_sigma_zero_is_the_plain_step_in_the_split_tail(sd, B):
    A = 4
    net, o = _pair(sd, A, B, 51)
    plain = sd.DeepQNetwork(A, make_args(batch_size=B, clip_grad_norm=1e30))      # the same tail form, scale exactly 1
    plain.set_weights(net.get_weights(1), 1)
    plain.set_weights(net.get_weights(0), 0)
    zero = [np.zeros_like(s) for s in net.get_noisy_sigma(0)]
    for z in (0, 1):
        net.set_noisy_sigma(zero, z)
    o.sigma, o.sigma_t = [s.copy() for s in zero], [s.copy() for s in zero]
    o._sopt.W[3], o._sopt.W[4] = o.sigma
    mb = random_minibatch(B, A, 52)
    plain.train(mb)
    net.train(mb)
    assert plain.last_grad_norm()[1] == 1.0
    assert _bits(net.last_q()[0], plain.last_q()[0])
    for i in range(5):
        assert _bits(net.get_layer(i, 0), plain.get_layer(i, 0)), i
    eps = net.noisy_eps()
    o.noisy_train(mb, eps[0], eps[1])
    sig = net.get_noisy_sigma(0)
    for k in range(2):
        assert np.abs(sig[k]).max() > 0
        big = np.abs(o.last_gsigma[k]) / B > 1e-6
        assert np.abs(sig[k] - o.sigma[k])[big].max() < 2e-5


# ---- 5: target ------------------------------------------------------------------------------------------------------------------------------
def test_target_copy_takes_sigma_and_keeps_its_own_noise(sd):
    A, B = 4, 32
    net, o = _pair(sd, A, B, 61)
    net.train(mb := random_minibatch(B, A, 62))
    eps = net.noisy_eps()
    o.noisy_train(mb, eps[0], eps[1])
    net.update_target_network()
    o.update_target_network()
    for k in range(2):
        assert _bits(net.get_noisy_sigma(1)[k], net.get_noisy_sigma(0)[k])
    same = random_minibatch(B, A, 63)
    same = (same[0], same[1], same[2], same[0], same[4])               # poststates = prestates: both nets see the same states
    net.train(same)
    eps = net.noisy_eps()
    q = net.debug_read("q", 2 * B * A).reshape(2, B, A)
    assert np.abs(q[0] - q[1]).max() > 1e-3
    assert np.abs(q[0] - o.predict_noisy(same[0], eps[0])).max() < Q_TOL
    assert np.abs(q[1] - o.predict_noisy(same[0], eps[1], target=True)).max() < Q_TOL


# ---- 6: acting ------------------------------------------------------------------------------------------------------------------------------
def test_predict_is_mu_and_predict_noisy_the_last_noise(sd):
    A, B = 4, 32
    net, o = _pair(sd, A, B, 71)
    st = random_minibatch(B, A, 72)[0]
    e0 = _host_eps(0, 0, A)
    assert np.abs(net.predict_noisy(st) - o.predict_noisy(st, e0)).max() < Q_TOL           # xi_0 before the first step
    net.train(mb := random_minibatch(B, A, 73))
    eps = net.noisy_eps()
    o.noisy_train(mb, eps[0], eps[1])
    plain = sd.DeepQNetwork(A, make_args(batch_size=B))
    plain.set_weights(net.get_weights(0), 0)
    assert _bits(net.predict(st), plain.predict(st))
    qn = net.predict_noisy(st)
    assert np.abs(qn - o.predict_noisy(st, eps[0])).max() < Q_TOL and np.abs(qn - net.predict(st)).max() > 1e-3
    # the single-environment acting paths by phase, on the one-launch forward and on the five-launch one
    for act_kernel in (1, 0):
        net.set_option("act_kernel", act_kernel)
        plain.set_option("act_kernel", act_kernel)
        net.set_acting(False)
        one = net.predict_one(st[3])
        assert np.abs(one - qn[3]).max() < Q_TOL and not _bits(one, plain.predict_one(st[3]))
        net.set_acting(True)
        assert _bits(net.predict_one(st[3]), plain.predict_one(st[3]))
    # the fused act step's argmax: predict_noisy's while collecting, predict's while testing, on a state where the two differ — under a
    # sigma 30 times the init, so that the noise outweighs fc5's mu (0.66 against 0.077) and the greedy action of most states moves
    net.set_noisy_sigma([30.0 * x for x in net.get_noisy_sigma(0)], 0)
    qn, qm = net.predict_noisy(st), net.predict(st)
    differ = [i for i in range(B) if int(np.argmax(qn[i])) != int(np.argmax(qm[i]))]
    assert differ, "no state on which the noise changes the greedy action: the two phases cannot be told apart"
    i = differ[0]
    buf = sd.DeviceStateBuffer(make_args(batch_size=B))
    for f in st[i]:
        buf.add(f)
    net.set_option("act_kernel", 1)
    net.set_acting(False)
    assert net.act_greedy(buf) == int(np.argmax(qn[i]))
    net.set_acting(True)
    assert net.act_greedy(buf) == int(np.argmax(qm[i]))


def test_collect_follows_predict_noisy_and_evaluate_mu(sd):
    Nenv, B = 4, 4
    args = _args(B, catch_balls=2, random_seed=4, prioritized_replay=False, n_step=1, double_dqn=False, eval_envs=0, train_envs=0,
                 priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000)
    net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(Nenv * 40, args)
    mem.set_lanes(Nenv)
    net.train(random_minibatch(B, 3, 81))
    out = net.collect(env, mem, Nenv, 4, 0.0, seed=77, trace=True)
    o = CollectOracle(Nenv, Nenv * 40, 4, 84, 84, 77, env.balls_per_episode)
    for t in range(4):
        rows = net.predict_noisy(o.games.states)[:Nenv]
        assert _bits(rows, out["q"][t].astype(np.float32)), t
        assert not _bits(rows, net.predict(o.games.states)[:Nenv])
        a, r, term = o.lockstep(0.0, out["q"][t])
        assert np.array_equal(a, np.array([np.argmax(q) for q in rows])) and np.array_equal(a, out["actions"][t]), t
        assert np.array_equal(r, out["rewards"][t]) and np.array_equal(term, out["terminals"][t]), t
    from test_gpu_collect import _assert_ring_equals
    _assert_ring_equals(mem, o, device=False)      # (four locksteps fill no whole state: the HBM mirror is read through states in tests/test_gpu_collect.py)
    # evaluating reads mu: the same mu and sigma after one more noise step give the same tallies
    e1 = net.evaluate(env, Nenv, 30, epsilon=0.0, seed=5, trace=True)
    w, s = net.get_weights(0), net.get_noisy_sigma(0)
    net.train(random_minibatch(B, 3, 82))
    net.set_weights(w, 0)
    net.set_noisy_sigma(s, 0)
    e2 = net.evaluate(env, Nenv, 30, epsilon=0.0, seed=5, trace=True)
    for k in ("steps", "reward", "caught", "missed", "episodes", "actions"):
        assert np.array_equal(e1[k], e2[k]), k
    assert _bits(e1["q"], e2["q"])


# ---- 7: launch census ---------------------------------------------------------------------------------------------------------------------
def _counts(net, fn):
    net.profile(True, -1); net.profile_reset()
    fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("B", [32, 64, 128])
def test_launch_census(sd, B):
    """a noisy step = the clip-form step - its two clip launches + three (compose, sigma, compose), all in the update slot; a plain
    net's step is what it was (tests/test_gpu_step_census.py holds it to the golden)"""
    A, n = 4, 3
    mbs = [random_minibatch(B, A, 90 + s) for s in range(n)]
    nets = dict(plain=sd.DeepQNetwork(A, make_args(batch_size=B)), clip=sd.DeepQNetwork(A, make_args(batch_size=B, clip_grad_norm=10.0)),
                noisy=sd.DeepQNetwork(A, _args(B)))
    c = dict((k, _counts(v, lambda v=v: [v.train(mb) for mb in mbs])) for k, v in nets.items())
    upd = [k for k in c["clip"] if k.startswith("update")]
    assert len(upd) == 1
    upd = upd[0]
    assert c["plain"][upd] == n and c["clip"][upd] == 4 * n
    assert c["noisy"][upd] == c["clip"][upd] - 2 * n + 3 * n == 5 * n
    rest = lambda d: {k: v for k, v in d.items() if k != upd}
    assert rest(c["noisy"]) == rest(c["clip"])


# ---- 8: stale buffers and stability -------------------------------------------------------------------------------------------------------
def test_changes_between_steps_reach_the_next_forward(sd, tmp_path):
    A, B = 4, 32
    net, o = _pair(sd, A, B, 101)
    st = random_minibatch(B, A, 102)[0]
    net.train(mb := random_minibatch(B, A, 103))
    eps = net.noisy_eps()
    o.noisy_train(mb, eps[0], eps[1])
    q0 = net.predict_noisy(st)
    o.W = [w.copy() for w in xavier_weights(A, 104)]
    net.set_weights(o.W, 0)
    q1 = net.predict_noisy(st)
    assert np.abs(q1 - q0).max() > 1e-3 and np.abs(q1 - o.predict_noisy(st, eps[0])).max() < Q_TOL
    o.sigma = [(2.0 * s).astype(np.float32) for s in o.sigma]
    net.set_noisy_sigma(o.sigma, 0)
    q2 = net.predict_noisy(st)
    assert np.abs(q2 - q1).max() > 1e-4 and np.abs(q2 - o.predict_noisy(st, eps[0])).max() < Q_TOL
    p = str(tmp_path / "n.npz")
    net.save_weights(p)
    other = sd.DeepQNetwork(A, _args(B))
    other.train(mb)                                                    # (same noise step as net: xi_1)
    other.load_weights(p)
    assert _bits(other.predict_noisy(st), q2) and _bits(other.get_noisy_sigma(1)[0], net.get_noisy_sigma(1)[0])
    with pytest.raises(ValueError, match="noisy_nets"):
        sd.DeepQNetwork(A, make_args(batch_size=B)).load_weights(p)


def test_200_steps_stay_finite_and_sigma_moves(sd):
    A, B = 3, 32
    args = _args(B)
    net = sd.DeepQNetwork(A, args)
    mem = sd.ReplayMemory(2000, args)
    synthetic_fill(mem, 3, num_actions=A)
    mem.sync_mirror()
    s0 = net.get_noisy_sigma(0)
    net.train_from_memory(mem, 200)
    assert net.noisy_step() == 200
    st = random_minibatch(B, A, 111)[0]
    for a in net.get_weights(0) + net.get_noisy_sigma(0) + [net.predict(st), net.predict_noisy(st)]:
        assert np.isfinite(a).all()
    s1 = net.get_noisy_sigma(0)
    assert all(np.abs(s1[k] - s0[k]).max() > 1e-4 for k in range(2))


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(sd):
    from simple_dqn_amd import _lib
    lib, A, B = _lib.load(), 4, 32
    noisy = sd.DeepQNetwork(A, _args(B))
    for call, word in ((lambda: noisy.set_clip_grad_norm(1.0), "clip_grad_norm"), (lambda: noisy.set_target_tau(0.01), "target_tau"),
                       (lambda: noisy.soft_update_target_network(0.5), "target_tau"), (lambda: noisy.set_munchausen(True), "munchausen"),
                       (lambda: noisy.set_advantage_learning(0.5), "advantage_learning"),
                       (lambda: _lib.check(lib.sdqn_net_set_bootstrap(noisy._h, 2, 1.0, 0)), "bootstrap_heads"),
                       (lambda: _lib.check(lib.sdqn_net_set_quantiles(noisy._h, 2)), "quantiles"),
                       (lambda: _lib.check(lib.sdqn_net_set_dueling(noisy._h, 1)), "dueling"),
                       (lambda: noisy.set_option("grad_only", 1), "data parallel"),
                       (lambda: _lib.check(lib.sdqn_net_apply_update(noisy._h, 32.0)), "data parallel"),
                       (lambda: _lib.check(lib.sdqn_dp_init(noisy._h, None, bytes(128), 0, 1)), "data parallel")):
        with pytest.raises(Exception) as e:
            call()
        assert word in str(e.value) and "noisy_nets" in str(e.value), (word, str(e.value))
    for kw, word in ((dict(datatype="float16"), "float16"), (dict(batch_norm=True), "batch_norm"), (dict(datatype="float64"), "float64"),
                     (dict(screen_height=60, screen_width=52, history_length=3), "84x84x4"), (dict(clip_grad_norm=5.0), "clip_grad_norm"), (dict(target_tau=0.1), "target_tau"),
                     (dict(munchausen=True), "munchausen"), (dict(advantage_learning=0.5), "advantage_learning"), (dict(dueling=True), "dueling")):
        net = sd.DeepQNetwork(A, make_args(batch_size=B, **kw))
        rc = lib.sdqn_net_set_noisy(net._h, 1, 0.5, 1)
        assert rc != 0, kw
        msg = lib.sdqn_last_error().decode()
        assert "noisy_nets" in msg and word in msg, (kw, msg)
    plain = sd.DeepQNetwork(A, make_args(batch_size=B))
    buf = np.zeros(4, np.float32)
    assert lib.sdqn_net_get_noisy_sigma(plain._h, 0, 3, _lib.ptr(buf, C.c_float), 4) != 0
    assert "not a noisy net" in lib.sdqn_last_error().decode()
