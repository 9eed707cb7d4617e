"""The device side of "freeway" (DESIGN.md §25): the render kernel, the fused act step against the host-driven one bit for bit,
vectorised evaluation and collection against tests/freeway_oracle.py, frame skip and sticky actions on the device, training on the
collected lanes against the tuple path, and main.run's loop.

A random policy almost never crosses (tests/test_freeway.py), so the runs that must see a reward play a network whose greedy action is
"up": fc5 is zero but for a positive row 1, so Q = (0, 0.01 sum(fc4 output), 0) and the first maximum is action 1 wherever any fc4 unit
is active.  The oracle follows the library's own Q rows, so the comparison does not depend on that."""
import ctypes as C
import csv
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import make_args  # noqa: E402
from oracle.replay_numpy import MT19937  # noqa: E402
from freeway_oracle import TALLIES, FreewayCollectOracle, FreewayEvalOracle, FreewayOracle, dynamics_collect_oracle, pack  # noqa: E402

pytestmark = pytest.mark.gpu
Q_TOL = 1e-4          # the tolerance tests/test_gpu_dqn.py uses for predict, the existing games' bound
COLLECT = "catch_collect(lockstep)"       # the profile's lockstep row counts every game's collect kernel (kernel ids are public numbers)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=10, breakout_balls=3, freeway_ticks=500, eval_envs=0, train_envs=0, frame_skip=1,
             repeat_action_probability=0.0)
    d.update(kw)
    return make_args(**d)


def _up_net(sd, args):
    """a network whose greedy action is "up" (the module's docstring)"""
    net = sd.DeepQNetwork(3, args)
    w = np.zeros_like(np.asarray(net.get_layer(4)))
    assert w.shape == (3, 512)
    w[1, :] = 0.01
    net.set_layer(4, w, 0)
    return net


def _device_window(sd, buf):
    out = np.empty((buf.history_length,) + buf.dims, np.uint8)
    sd._lib.check(sd.load().sdqn_statebuf_read_device(buf._h, sd._lib.ptr(out, C.c_uint8)))
    return out


def _device_ring(mem):
    """frames [0, covered) of an unlaned HBM mirror, read through the gather kernel (prestates of indexes hist, 2 hist, ...)"""
    hist, B = mem.history_length, mem.batch_size
    idx = list(range(hist, mem.count - mem.n_step + 1, hist))
    frames = np.zeros((idx[-1],) + mem.dims, np.uint8)
    for o in range(0, len(idx), B):
        part = idx[o:o + B]
        pre = np.asarray(mem.gather(part + [part[-1]] * (B - len(part)))[0])
        for k, i in enumerate(part):
            frames[i - hist:i] = pre[k]
    return frames


def _lane_ring(mem):
    """slots [0, fill) of every lane of the HBM mirror, read through the gather kernel (pre- and poststates of local indexes hist,
    2 hist, ..., fill - n)"""
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


def _assert_ring_equals(mem, o):
    """the host master, its metadata, fill / position and the device ring against the oracle's"""
    assert mem.lanes == (o.N, o.L, o.f, o.p)
    assert (mem.count, mem.current) == (o.N * o.f, o.p)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(_filled(mem, getattr(mem, name)), _filled(mem, getattr(o, name))), name
    assert np.array_equal(_filled(mem, _lane_ring(mem)), _filled(mem, o.screens))


@pytest.mark.parametrize("H,W", [(84, 84), (12, 12), (36, 38), (96, 96), (60, 52)])
def test_render_kernel_equals_host_and_oracle(sd, H, W):
    """84 x 84 and 96 x 96: 16-byte stores; 12 x 12: one cell per pixel; 36 x 38: the byte path (1 368 bytes), two remainder columns;
    60 x 52: cells 5 x 4, not square, four remainder columns"""
    env, o = sd.FreewayEnvironment(_args(screen_height=H, screen_width=W), seed=3), FreewayOracle(H, W, 3)
    base = env.get_state()
    five = pack([5] * 10)
    cases = [dict(row=11, cars=pack([0] * 10)), dict(row=11, cars=pack([11] * 10)),                 # every car on the first / last column
             dict(row=11, cars=pack([6] * 10)),                                                     # a column of cars above the chicken
             dict(row=0, cars=pack(list(range(10)))), dict(row=0, cars=pack(list(range(11, 1, -1)))),   # the diagonals; the chicken on row 0
             dict(row=5, cars=pack([6, 6, 6, 6, 5, 6, 6, 6, 6, 6])), dict(row=5, cars=pack([6, 6, 6, 6, 7, 6, 6, 6, 6, 6])),   # a car beside the chicken
             dict(row=1, cars=pack([0, 6, 1, 2, 3, 4, 5, 7, 8, 11])), dict(row=10, cars=pack([6, 0, 11, 3, 3, 3, 9, 9, 6, 7]))]
    for case in cases:
        st = dict(base, timers=five, periods=five, **case)
        env.set_state(st); o.set_state(st)
        d = env.render_device()
        assert np.array_equal(d, o.screen()) and np.array_equal(d, env.getScreen()), case
        assert (d == 255).sum() == (H // 12) * (W // 12) and (d == 128).sum() == 10 * (H // 12) * (W // 12)
    env.set_state(base); o.set_state(base)
    for t in range(120):                                                             # and along a game
        a = (1, 1, 0, 1, 2, 1)[t % 6]
        env.act(a); o.act(a)
        if t % 4 == 0:
            d = env.render_device()
            assert np.array_equal(d, o.screen()) and np.array_equal(d, env.getScreen()), t
        if o.terminal:
            env.restart(); o.restart()


def test_fused_act_step_equals_host_driven(sd):
    """300 steps of sdqn_net_act_step_env against sdqn_env_step + sdqn_env_screen + add: ring mirror (120 slots: it wraps twice),
    state-buffer window and metadata bit for bit; mostly "up", episodes of 70 ticks: crossings, hits and terminals all occur"""
    args = _args(batch_size=32, random_seed=11, target_steps=100, freeway_ticks=70)
    steps, size = 300, 120
    sets = []
    for fused in (False, True):
        env, buf, mem = sd.FreewayEnvironment(args, seed=77), sd.DeviceStateBuffer(args), sd.ReplayMemory(size, args)
        sets.append((fused, env, buf, mem, sd.DeepQNetwork(3, args)))
    rs = np.random.RandomState(5)
    actions = np.where(rs.rand(steps) < 0.7, 1, rs.randint(0, 3, steps))
    log = [[], []]
    for t in range(steps):
        spec = bool(t % 5 == 0)
        for k, (fused, env, buf, mem, net) in enumerate(sets):
            a = int(actions[t])
            if fused:
                r, term = net.act_step_env(buf, mem, env, a, speculate=spec)
            else:
                r = env.act(a)
                term = env.isTerminal()
                net.act_step(buf, mem, env.getScreen(), a, r, term, speculate=spec and not term)
            log[k].append((a, r, term))
            if term:
                env.restart()
        if t % 29 == 0 or t > steps - 20:
            w = [_device_window(sd, s[2]) for s in sets]
            assert np.array_equal(w[0], w[1]), t
            assert np.array_equal(sets[0][2].getState(), sets[1][2].getState()) and np.array_equal(w[1], sets[1][2].getState()), t
            assert np.array_equal(sets[0][1].getScreen(), sets[1][1].getScreen())
            assert sets[0][1].get_state() == sets[1][1].get_state()
            if spec:
                assert np.array_equal(sets[0][4].predict_state(sets[0][2]), sets[1][4].predict_state(sets[1][2]))
    assert log[0] == log[1] and sum(x[2] for x in log[0]) == steps // 70 and any(x[1] for x in log[0])
    m0, m1 = sets[0][3], sets[1][3]
    assert (m0.count, m0.current) == (m1.count, m1.current) == (size, steps % size)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    d0, d1 = _device_ring(m0), _device_ring(m1)
    assert len(d0) >= size - 8 and np.array_equal(d0, d1)
    assert np.array_equal(d1, np.asarray(m1.screens)[:len(d1)])       # the kernel-rendered mirror == the host-rendered ring
    assert (d1 == 128).any() and (d1 == 255).any()
    mbs = []
    for m in (m0, m1):
        random.seed(1)
        mbs.append([np.array(x) for x in m.getMinibatch()])
    for x, y in zip(*mbs):
        assert np.array_equal(x, y)


def _check_against_oracle(net, env, N, steps, eps, seed, check_q):
    B = net.batch_size
    out = net.evaluate(env, N, steps, eps, seed, trace=True)
    o = FreewayEvalOracle(N, net.history_length, env.dims[0], env.dims[1], eps, seed, env.balls_per_episode)
    explored = 0
    for t in range(steps):
        if check_q:                                                  # (i) the forward saw the oracle's states
            st = np.zeros((B,) + o.states.shape[1:], np.uint8); st[:N] = o.states
            err = np.abs(net.predict(st)[:N].astype(np.float64) - out["q"][t]).max()
            assert err < Q_TOL, (t, err)
        a, r, term = o.step(out["q"][t])                             # (ii) the rule on the library's own Q bits
        assert np.array_equal(a, out["actions"][t]), t
        assert np.array_equal(r, out["rewards"][t]) and np.array_equal(term, out["terminals"][t]), t   # (iii)
        explored += int((a != np.array([np.argmax(q) for q in out["q"][t]])).sum())
    for k in TALLIES:
        assert np.array_equal(out[k], o.tally[k]), k
    assert out["steps"].tolist() == [steps] * N
    plain = net.evaluate(env, N, steps, eps, seed)                   # (iv) the untraced call gives the same tallies
    for k in TALLIES:
        assert np.array_equal(plain[k], out[k]), k
    assert explored <= o.explored <= steps * N                       # an action off the greedy one comes from an exploring draw
    return out, explored


@pytest.mark.parametrize("N", [32, 4])
def test_evaluate_equals_the_oracle_float32(sd, N):
    """N = 32: the "up" network, episodes of 60 ticks: crossings, hits and terminals; N = 4: an untrained network as it comes"""
    args = _args(batch_size=32, random_seed=4, freeway_ticks=60)
    net, env = (_up_net(sd, args) if N == 32 else sd.DeepQNetwork(3, args)), sd.FreewayEnvironment(args, seed=1)
    before = env.get_state()
    out, explored = _check_against_oracle(net, env, N, 150, 0.1, 1234 + N, check_q=True)
    assert env.get_state() == before
    assert out["episodes"].tolist() == [150 // 60] * N and out["reward"].sum() == out["caught"].sum()
    assert explored > 0
    if N == 32:
        assert out["caught"].sum() > 0 and out["missed"].sum() > 0
        with pytest.raises(AssertionError):
            net.evaluate(env, 33, 10)
        with pytest.raises(AssertionError):
            net.evaluate(sd.FreewayEnvironment(_args(screen_height=96, screen_width=96), seed=1), 4, 10)
        with pytest.raises(AssertionError):
            sd.DeepQNetwork(4, args).evaluate(env, 4, 10)            # a network of 4 actions cannot play a game of 3


@pytest.mark.parametrize("kw", [dict(datatype="float16", batch_size=32), dict(datatype="float64", batch_size=8, screen_height=36, screen_width=38)])
def test_evaluate_other_configurations(sd, kw):
    args = _args(random_seed=6, freeway_ticks=25, **kw)
    net, env = sd.DeepQNetwork(3, args), sd.FreewayEnvironment(args, seed=2)
    _check_against_oracle(net, env, 8, 60, 0.1, 99, check_q=False)


@pytest.mark.parametrize("H,W,eps", [(84, 84, 0.3), (84, 84, 1.0), (36, 38, 1.0)])
def test_collect_equals_the_oracle(sd, H, W, eps):
    """N = 4 lanes of 24 slots (a 96-slot ring), 60 locksteps (every lane wraps 2.5 times), episodes of 30 ticks so that every lane
    holds terminals on slots a sampler can pick; epsilon 0.3 (traced, the "up" network: the oracle replays the run from the library's own Q rows, which are the
    forward of the oracle's states) and 1 (no forward runs); 36 x 38: a generic net and the byte path of the collect kernel"""
    N, steps = 4, 60
    args = _args(batch_size=32, screen_height=H, screen_width=W, freeway_ticks=30, random_seed=3)
    net = _up_net(sd, args) if eps < 1.0 else sd.DeepQNetwork(3, args)
    env, mem = sd.FreewayEnvironment(args, seed=1), sd.ReplayMemory(N * 24, args)
    assert net.step_structure()[0] == ("fused" if (H, W) == (84, 84) else "generic")
    mem.set_lanes(N)
    out = net.collect(env, mem, N, steps, eps, seed=5, trace=eps < 1.0)
    o = FreewayCollectOracle(N, N * 24, 4, H, W, 5, env.balls_per_episode)
    for t in range(steps):
        if eps < 1.0:
            if t % 6 == 0 or t == steps - 1:
                st = np.zeros((32,) + o.games.states.shape[1:], np.uint8); st[:N] = o.games.states
                err = np.abs(net.predict(st)[:N].astype(np.float64) - out["q"][t]).max()
                assert err < Q_TOL, (t, err)
            a, r, term = o.lockstep(eps, out["q"][t])
            assert np.array_equal(a, out["actions"][t]) and np.array_equal(r, out["rewards"][t]), t
            assert np.array_equal(term, out["terminals"][t]), t
        else:
            o.lockstep(1.0)
    assert (o.f, o.p) == (24, 60 % 24) and o.terminals.any() and len(set(o.actions.tolist())) == 3
    _assert_ring_equals(mem, o)
    for k in TALLIES:
        assert np.array_equal(out[k], o.tally[k]), k
    assert out["steps"].tolist() == [steps] * N and out["episodes"].tolist() == [60 // 30] * N and out["missed"].sum() > 0
    assert eps == 1.0 or o.rewards.any()                             # the "up" network crossed, and the crossing is still in the ring
    assert np.array_equal(mem.getState(10), o.screens[7:11])


def test_collect_continues_across_calls(sd):
    """collect(20); collect(40) equals collect(60)"""
    rings = []
    for parts in ((60,), (20, 40)):
        args = _args(batch_size=32, freeway_ticks=25, random_seed=4)
        net, env, mem = _up_net(sd, args), sd.FreewayEnvironment(args, seed=1), sd.ReplayMemory(96, args)
        mem.set_lanes(4)
        seed = 9
        for n in parts:
            out = net.collect(env, mem, 4, n, 0.5, seed=seed)
            seed = None
        rings.append((mem, out, _lane_ring(mem)))
    (m0, t0, d0), (m1, t1, d1) = rings
    assert m0.lanes == m1.lanes == (4, 24, 24, 60 % 24)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    assert np.array_equal(d0, d1) and np.array_equal(d0, np.asarray(m0.screens))
    for k in TALLIES:
        assert np.array_equal(t0[k], t1[k]) and t0["steps"].tolist() == [60] * 4, k
    # the copies on the net handle play ONE game: another game's environment cannot resume freeway's copies, nor freeway another's
    net, mem = sd.DeepQNetwork(3, _args(batch_size=32)), sd.ReplayMemory(96, _args(batch_size=32))
    mem.set_lanes(4)
    net.collect(sd.FreewayEnvironment(_args(), seed=1), mem, 4, 2, 1.0, seed=1)
    for other in (sd.CatchEnvironment, sd.BreakoutEnvironment):
        with pytest.raises(AssertionError):
            net.collect(other(_args(), seed=1), mem, 4, 1, 1.0)
    net.collect(sd.FreewayEnvironment(_args(), seed=1), mem, 4, 1, 1.0)
    net.collect(sd.BreakoutEnvironment(_args(), seed=1), mem, 4, 2, 1.0, seed=1)
    with pytest.raises(AssertionError):
        net.collect(sd.FreewayEnvironment(_args(), seed=1), mem, 4, 1, 1.0)


def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


def test_launches_per_lockstep(sd):
    args = _args(batch_size=32)
    net, env, mem = sd.DeepQNetwork(3, args), sd.FreewayEnvironment(args, seed=1), sd.ReplayMemory(320, args)
    mem.set_lanes(32)
    net.collect(env, mem, 32, 2, 1.0, seed=1)
    states = np.zeros((32, 4, 84, 84), np.uint8)
    forward = _counts(net, lambda: net.predict(states))
    assert forward and COLLECT not in forward
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 1.0)) == {COLLECT: 3}          # epsilon >= 1: one kernel
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 0.3)) == dict(forward, **{COLLECT: 3})   # else the forward's launches plus one
    assert _counts(net, lambda: net.collect(env, mem, 32, 2, 0.9, epsilon_step=0.1)) == dict(forward, **{COLLECT: 6})


def test_training_on_the_lanes_equals_the_tuple_path(sd):
    """three train_from_memory steps on the collected lanes: the windows the lane sampler picks, gathered from the device, are slices
    of the oracle's ring, and the weights afterwards are bit-identical to the library's own tuple path trained on the minibatches the
    oracle samples and gathers"""
    N, size, steps = 4, 96, 60
    args = _args(batch_size=32, freeway_ticks=30, random_seed=3, target_steps=100)
    env, mem = sd.FreewayEnvironment(args, seed=1), sd.ReplayMemory(size, args)
    mem.set_lanes(N)
    ring_net, tuple_net = _up_net(sd, args), _up_net(sd, args)
    for which in (0, 1):
        for i in range(5):
            tuple_net.set_layer(i, np.asarray(ring_net.get_layer(i, which)), which)
    out = ring_net.collect(env, mem, N, steps, 0.1, seed=7, trace=True)
    o = FreewayCollectOracle(N, size, 4, 84, 84, 7, env.balls_per_episode)
    for t in range(steps):
        o.lockstep(0.1, out["q"][t])
    _assert_ring_equals(mem, o)
    seen_done = seen_reward = False
    w0 = [np.array(ring_net.get_layer(i)) for i in range(5)]
    for s in range(3):
        random.seed(100 + s)
        ring_net.train_from_memory(mem, 1)
        idx, _ = o.sample(MT19937(100 + s), 1, 32)
        mb = o.gather(idx, 1, args.discount_rate, args.min_reward, args.max_reward)
        got = mem.gather(idx)
        for x, y in zip(got, mb):
            assert np.array_equal(np.asarray(x), y)
        seen_done |= bool(mb[4].any()); seen_reward |= bool(mb[2].any())
        tuple_net.train(mb)
    assert seen_done and seen_reward
    for i in range(5):
        assert np.array_equal(ring_net.get_layer(i), tuple_net.get_layer(i)), i
    assert any(not np.array_equal(w0[i], ring_net.get_layer(i)) for i in range(5))       # the steps moved the net


def test_collect_under_frame_skip_and_sticky_actions(sd):
    """--frame_skip 2 --repeat_action_probability 0.25: 40 locksteps of N = 3 lanes of 32 slots against tests/dynamics_oracle.py's
    rule on the freeway oracle — chosen actions, summed rewards, terminals (episodes of 25 ticks: 13 agent steps, the last cut short),
    the ring and the tallies"""
    N, size, steps, seed, k, p = 3, 96, 40, 5, 2, 0.25
    args = _args(batch_size=32, random_seed=3, freeway_ticks=25, frame_skip=k, repeat_action_probability=p)
    net, env, mem = _up_net(sd, args), sd.FreewayEnvironment(args, seed=1), sd.ReplayMemory(size, args)
    mem.set_lanes(N)
    out = net.collect(env, mem, N, steps, 0.3, seed=seed, trace=True)
    o = dynamics_collect_oracle(N, size, 4, 84, 84, seed, env.balls_per_episode, k, p)
    for t in range(steps):
        a, r, term = o.lockstep(0.3, out["q"][t])
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(r, out["rewards"][t]), t
        assert np.array_equal(term, out["terminals"][t]), t
    assert (o.f, o.p) == (32, 40 % 32) and o.terminals.any()
    assert sum(g.stuck for g in o.games.envs) > 0 and out["episodes"].tolist() == [40 // 13] * N
    _assert_ring_equals(mem, o)
    for name in TALLIES:
        assert np.array_equal(out[name], o.tally[name]), name


def test_main_loop_on_freeway(sd, tmp_path):
    from simple_dqn_amd import main
    path = str(tmp_path / "freeway.csv")
    args = _args(environment="freeway", train_envs=4, eval_envs=4, replay_size=800, random_steps=320, train_steps=80, test_steps=200,
                 epochs=1, batch_size=32, random_seed=5, target_steps=40, exploration_decay_steps=400, csv_file=path, num_actions=3,
                 synthetic_frame_pool=0, game="freeway", visualization_file=None, visualization_filters=4, freeway_ticks=40)
    st = main.run(args)
    rows = list(csv.reader(open(path)))
    assert [r[1] for r in rows[1:]] == ["random", "train", "test"] and len(rows) == 4
    assert [int(r[2]) for r in rows[1:]] == [320, 80, 200]
    assert st.env.name() == "freeway" and st.mem.lanes[0] == 4 and st.net.train_iterations == 80 // 4
