"""--train_envs on the device: the collect kernel and the laned ring against tests/collect_oracle.py bit for bit, the
train paths on a laned memory against the numpy DQN oracles, refusals, launch counts and the learning test."""
import ctypes as C
import os
import random
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nstep_oracle as NO  # noqa: E402
from collect_oracle import CollectOracle  # noqa: E402
from oracle.dqn_numpy import xavier_weights  # noqa: E402
from oracle.replay_numpy import MT19937  # noqa: E402
from test_catch import random_baseline  # noqa: E402
from test_gpu_dqn import Q_TOL  # noqa: E402
from test_gpu_nstep import CONFIGS as NSTEP_CONFIGS  # noqa: E402
from test_gpu_catch import EVAL_STEPS, LEARN, per_ball  # noqa: E402
from util import make_args  # noqa: E402

pytestmark = pytest.mark.gpu
TALLIES = ("steps", "reward", "caught", "missed", "episodes")
COLLECT = "catch_collect(lockstep)"


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=10, eval_envs=0, train_envs=0)
    d.update(kw)
    return make_args(**d)


def _device_ring(mem):
    """slots [0, fill) of every lane of the HBM mirror, read through the gather kernel (prestates and poststates of local indexes
    hist, 2 hist, ..., fill - n)"""
    N, L, f, _ = mem.lanes
    hist, B, n = mem.history_length, mem.batch_size, mem.n_step
    idx = [e * L + l for e in range(N) for l in list(range(hist, f - n + 1, hist)) + [f - n]]
    frames = np.zeros((mem.size,) + mem.dims, np.uint8)
    seen = np.zeros(mem.size, bool)
    for o in range(0, len(idx), B):
        part = idx[o:o + B]
        mb = mem.gather(part + [part[-1]] * (B - len(part)))
        pre, post = np.asarray(mb[0]), np.asarray(mb[3])
        for k, i in enumerate(part):
            frames[i - hist:i] = pre[k]; seen[i - hist:i] = True
            frames[i + n - hist:i + n] = post[k]; seen[i + n - hist:i + n] = True
    assert all(seen[e * L:e * L + f].all() for e in range(N))
    return frames


def _filled(mem, a):
    N, L, f, _ = mem.lanes
    return np.concatenate([np.asarray(a)[e * L:e * L + f] for e in range(N)])


def _assert_ring_equals(mem, o, device=True):
    assert mem.lanes == (o.N, o.L, o.f, o.p)
    assert (mem.count, mem.current) == (o.N * o.f, o.p)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(_filled(mem, getattr(mem, name)), _filled(mem, getattr(o, name))), name
    if device:
        assert np.array_equal(_filled(mem, _device_ring(mem)), _filled(mem, o.screens))


def test_the_layer_stack_refuses_36x30(sd):
    """36 x 30 (a frame that is no multiple of 16 bytes) cannot carry a network: conv3 would see a 3 x 2 map.  The byte path of the
    collect kernel is therefore exercised at 36 x 38 below — the smallest such screen the stack of deepqnetwork.py:83-87 digests."""
    with pytest.raises(AssertionError):
        sd.DeepQNetwork(3, _args(screen_height=36, screen_width=30))
    assert (36 * 38) % 16 == 8 and (36 * 30) % 16 == 8


@pytest.mark.parametrize("H,W", [(84, 84), (36, 38)])
def test_collect_equals_the_oracle_random_policy(sd, H, W):
    """epsilon = 1, N = 3, 69 slots, 60 locksteps: every lane of 23 slots wraps 2.6 times; two-ball episodes put terminals in every lane"""
    args = _args(batch_size=32, screen_height=H, screen_width=W, catch_balls=2, random_seed=3)
    net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(69, args)
    assert net.step_structure()[0] == ("fused" if (H, W) == (84, 84) else "generic")
    mem.set_lanes(3)
    out = net.collect(env, mem, 3, 60, 1.0, seed=5)
    o = CollectOracle(3, 69, 4, H, W, 5, env.balls_per_episode)
    for _ in range(60):
        o.lockstep(1.0)
    assert (o.f, o.p) == (23, 60 % 23) and o.terminals.any() and len(set(o.actions.tolist())) == 3
    _assert_ring_equals(mem, o)
    for k in TALLIES:
        assert np.array_equal(out[k], o.tally[k]), k
    assert out["steps"].tolist() == [60] * 3 and out["episodes"].sum() == 3 * (60 // 22)
    # the host ring is a true copy: getState and the sampler's terminal check read it like any other memory
    assert np.array_equal(mem.getState(10), o.screens[7:11])


def test_collect_with_a_live_network(sd):
    """epsilon = 0.3, N = 32 = batch_size, 1280 slots, 50 locksteps (every lane of 40 wraps), traced: the oracle replays the run from the
    library's own Q rows, which in turn are the forward of the ORACLE's states"""
    N, steps, eps = 32, 50, 0.3
    args = _args(batch_size=32, catch_balls=2, random_seed=4)
    net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(N * 40, args)
    mem.set_lanes(N)
    out = net.collect(env, mem, N, steps, eps, seed=77, trace=True)
    o = CollectOracle(N, N * 40, 4, 84, 84, 77, env.balls_per_episode)
    greedy = 0
    for t in range(steps):
        if t % 7 == 0 or t == steps - 1:
            err = np.abs(net.predict(o.games.states)[:N].astype(np.float64) - out["q"][t]).max()
            assert err < Q_TOL, (t, err)
        a, r, term = o.lockstep(eps, out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(r, out["rewards"][t]), t
        assert np.array_equal(term, out["terminals"][t]), t
        greedy += int((a == np.array([np.argmax(q) for q in out["q"][t]])).sum())
    assert greedy > 0.7 * N * steps and out["terminals"].any()
    _assert_ring_equals(mem, o)
    for k in TALLIES:
        assert np.array_equal(out[k], o.tally[k]), k


def test_collect_continues_across_calls(sd):
    rings = []
    for parts in ((60,), (20, 40)):
        args = _args(batch_size=32, catch_balls=2, random_seed=4)
        net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(69, args)
        mem.set_lanes(3)
        seed = 9
        for n in parts:
            out = net.collect(env, mem, 3, n, 0.5, seed=seed)
            seed = None
        rings.append((mem, out, _device_ring(mem)))
    (m0, t0, d0), (m1, t1, d1) = rings
    assert m0.lanes == m1.lanes == (3, 23, 23, 60 % 23)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    assert np.array_equal(d0, d1) and np.array_equal(d0, np.asarray(m0.screens))
    for k in TALLIES:
        assert np.array_equal(t0[k], t1[k]) and t0["steps"].tolist() == [60] * 3, k
    with pytest.raises(AssertionError):                             # nothing to resume for another number of copies
        sd.DeepQNetwork(3, _args(batch_size=32)).collect(sd.CatchEnvironment(_args(), seed=1), m0, 3, 1, 1.0)


@pytest.mark.parametrize("variant", ["n1", "n3", "double_dqn"])
def test_training_reads_lanes_correctly(sd, variant):
    """3 steps of train_from_memory on the collected lanes (float32, B = 32) against the numpy DQN fed the minibatches the lane oracle
    samples and gathers: Q within the bounds of tests/test_gpu_dqn.py (n = 1) / tests/test_gpu_nstep.py (n = 3), and the weights
    bit-identical to the library's own tuple path trained on the oracle's minibatches"""
    n = 3 if variant == "n3" else 1
    double = variant == "double_dqn"
    tol = Q_TOL if n == 1 else NSTEP_CONFIGS["fp32_b32"][5]
    args = _args(batch_size=32, catch_balls=2, random_seed=3, n_step=n, double_dqn=double, target_steps=100)
    env, mem = sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(69, args)
    mem.set_lanes(3)
    ws, wt = xavier_weights(3, 31), xavier_weights(3, 131)
    nets = []
    for _ in range(2):
        net = sd.DeepQNetwork(3, args)
        net.set_weights(wt, 1); net.set_weights(ws, 0)
        nets.append(net)
    ring_net, tuple_net = nets
    ring_net.collect(env, mem, 3, 60, 1.0, seed=5)
    o = CollectOracle(3, 69, 4, 84, 84, 5, env.balls_per_episode)
    for _ in range(60):
        o.lockstep(1.0)
    dqn = (NO.NStepOracleDDQN if double else NO.NStepOracle)(3, batch_size=32, weights=ws)
    dqn.Wt = [w.copy() for w in wt]
    dqn.n_step = n
    seen_done = False
    for s in range(3):
        random.seed(100 + s)
        ring_net.train_from_memory(mem, 1)
        idx, _ = o.sample(MT19937(100 + s), n, 32)
        mb = o.gather(idx, n, args.discount_rate, args.min_reward, args.max_reward)
        got = mem.gather(idx)                                        # the device gather of the same windows: slices of ONE lane
        for x, y in zip(got, mb):
            assert np.array_equal(np.asarray(x), y)
        seen_done |= bool(mb[4].any())
        dqn.train(mb)
        tuple_net.train(mb)
    assert seen_done
    for i in range(5):
        assert np.array_equal(ring_net.get_layer(i), tuple_net.get_layer(i)), i
    hold = o.gather(o.sample(MT19937(99), n, 32)[0], n)[0]
    ref = dqn.predict(hold)
    err = np.abs(ring_net.predict(hold) - ref).max()
    print("%s: Q max abs err after 3 steps %.3e (bound %.1e)" % (variant, err, tol))
    assert err < tol * max(1.0, float(np.abs(ref).max()))
    assert np.abs(ring_net.predict(hold) - xavier_predict(sd, args, ws, hold)).max() > tol           # the steps moved the net


def xavier_predict(sd, args, ws, states):
    net = sd.DeepQNetwork(3, args)
    net.set_weights(ws, 0)
    return net.predict(states)


def test_a_laned_memory_refuses_what_it_cannot_serve(sd):
    args = _args(batch_size=32)
    net, env, buf, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.DeviceStateBuffer(args), sd.ReplayMemory(96, args)
    mem.set_lanes(3)
    screen = np.zeros((84, 84), np.uint8)
    with pytest.raises(AssertionError):
        mem.add(0, 0, screen, False)
    with pytest.raises(AssertionError):
        net.act_step(buf, mem, screen, 0, 0, False)
    with pytest.raises(AssertionError):
        net.act_step_env(buf, mem, env, 0)
    with pytest.raises(AssertionError):
        mem.count = 5
    with pytest.raises(AssertionError):
        mem.current = 5
    with pytest.raises(AssertionError):
        sd.load() and sd._lib.check(sd.load().sdqn_replay_set_state(mem._h, 0, 0))
    with pytest.raises(AssertionError):
        net.train_from_memory(mem, 1)                                # empty lanes: span <= 0
    net.collect(env, mem, 3, 10, 1.0, seed=1)
    with pytest.raises(AssertionError):
        mem.set_lanes(3)                                             # only on an empty memory
    with pytest.raises(AssertionError):
        net.collect(env, mem, 4, 1, 1.0, seed=1)                     # num_envs != lanes
    for bad in (0, 5, 96 // 4):                                      # 0 lanes, 96 % 5 != 0, lanes of 4 < hist + n + 2
        with pytest.raises(AssertionError):
            sd.ReplayMemory(96, args).set_lanes(bad)
    per = sd.ReplayMemory(96, _args(batch_size=32, prioritized_replay=True))
    with pytest.raises(AssertionError) as ei:
        per.set_lanes(3)
    assert "prioritized" in str(ei.value)
    used = sd.ReplayMemory(96, args)
    used.add(0, 0, screen, False)
    with pytest.raises(AssertionError):
        used.set_lanes(3)
    # an unlaned memory is served as ever by a net that has collected before
    res = []
    for net_k in (net, sd.DeepQNetwork(3, args)):
        plain = sd.ReplayMemory(200, args)
        assert plain.lanes == (0, 0, 0, 0)
        e2, b2 = sd.CatchEnvironment(args, seed=4), sd.DeviceStateBuffer(args)
        for t in range(120):
            if net_k.act_step_env(b2, plain, e2, t % 3)[1]:
                e2.restart()
        assert (plain.count, plain.current) == (120, 120)
        random.seed(2)
        idx = plain.sample_indexes().copy()
        res.append((idx, np.asarray(plain.gather(idx)[0]).copy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("kw", [{}, dict(datatype="float16"), dict(batch_norm=True)])
def test_launches_per_lockstep(sd, kw):
    args = _args(batch_size=32, **kw)
    net, env, mem = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1), sd.ReplayMemory(320, args)
    mem.set_lanes(32)
    net.collect(env, mem, 32, 2, 1.0, seed=1)
    states = np.zeros((32, 4, 84, 84), np.uint8)
    forward = _counts(net, lambda: net.predict(states))
    assert forward and COLLECT not in forward
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 1.0)) == {COLLECT: 3}          # epsilon >= 1: one kernel
    live = _counts(net, lambda: net.collect(env, mem, 32, 1, 0.3))
    assert live == dict(forward, **{COLLECT: 3})                                             # else the forward's launches plus one
    assert _counts(net, lambda: net.collect(env, mem, 32, 2, 0.9, epsilon_step=0.1)) == dict(
        dict((k, v) for k, v in forward.items()), **{COLLECT: 6})                            # (0.9 runs the forward, 1.0 does not)


# ---- the learning test: tests/test_gpu_catch.py's task, criterion and command line with --train_envs 32 -----------------------------
# The step budget is NOT the measured "twice the slowest first crossing" of DESIGN.md §18's rule yet: the curves of seeds 1, 2, 3 (60 000
# env-steps, evaluated every 5 000) could not be taken when this file was written (DESIGN.md §19 says why), so the budget is the whole
# horizon those curves are to be measured over.  The criterion is tests/test_gpu_catch.py's, unchanged.
BUDGET_STEPS = 60000


def _midpoint():
    return (random_baseline() + 1.0) / 2.0


def learning_run(sd, seed, steps, every=None, **kw):
    """main.run's loop on catch with --train_envs 32; returns (mean reward per ball of the untrained net, [(env steps, per ball)])"""
    from simple_dqn_amd import main
    kw = dict(LEARN, train_envs=32, **kw)
    st = main.run(_args(random_seed=seed, epochs=0, train_steps=0, **dict(kw, random_steps=0)))
    before = per_ball(st.net, st.env, 1000 + seed)
    chunk = every or steps
    curve = []
    if every is None:
        st = main.run(_args(random_seed=seed, epochs=1, train_steps=steps, **kw))
        return before, [(steps, per_ball(st.net, st.env, 2000 + seed))]
    from simple_dqn_amd import Agent, CatchEnvironment, DeepQNetwork, ReplayMemory
    args = _args(random_seed=seed, epochs=steps // chunk, train_steps=chunk, **kw)
    random.seed(seed)
    env = CatchEnvironment(args, seed=seed)
    mem, net = ReplayMemory(args.replay_size, args), DeepQNetwork(3, args)
    agent = Agent(env, mem, net, args)
    agent.play_random_vectorised(args.random_steps)
    for epoch in range(args.epochs):
        agent.train_vectorised(chunk, epoch)
        curve.append(((epoch + 1) * chunk, per_ball(net, env, 2000 + seed + epoch)))
    return before, curve


@pytest.mark.parametrize("seed,kw", [(1, {}), (2, {}), (3, {}), (1, dict(double_dqn=True)), (1, dict(n_step=3))])
def test_the_agent_learns_catch_from_32_copies(sd, seed, kw):
    """tests/test_gpu_catch.py's learning test with --train_envs 32 (float32, otherwise that file's command line): after BUDGET_STEPS
    environment steps the mean reward per ball over >= 2 000 balls (evaluate, 32 copies, 770 steps, epsilon 0.05) reaches the midpoint
    between the random policy's and +1 (0.2445); the untrained net stays below it.  Seeds 1, 2, 3, and seed 1 with --double_dqn and
    with --n_step 3.  No run of this test had been made on a device when it was committed: no figures to report yet."""
    t0 = time.time()
    before, curve = learning_run(sd, seed, BUDGET_STEPS, **kw)
    after = curve[-1][1]
    print("seed %d %s: midpoint %.3f, untrained %.3f, after %d steps %.3f, %.1f s"
          % (seed, kw, _midpoint(), before, BUDGET_STEPS, after, time.time() - t0))
    assert EVAL_STEPS == 770 and before < _midpoint()
    assert after >= _midpoint()
