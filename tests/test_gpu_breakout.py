"""The device side of "breakout" (DESIGN.md §20): the render kernel, the fused act step against the host-driven one bit for bit,
vectorised evaluation and collection against tests/breakout_oracle.py, training on the collected lanes, and main.run's loop."""
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
from breakout_oracle import TALLIES, WALL, BreakoutCollectOracle, BreakoutEvalOracle, BreakoutOracle, brick_bit  # noqa: E402

pytestmark = pytest.mark.gpu
Q_TOL = 1e-4          # the tolerance tests/test_gpu_dqn.py uses for predict
COLLECT = "catch_collect(lockstep)"       # the profile's lockstep row counts either game's collect kernel (kernel ids are public numbers)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=10, breakout_balls=3, eval_envs=0, train_envs=0)
    d.update(kw)
    return make_args(**d)


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


@pytest.mark.parametrize("H,W", [(84, 84), (96, 96), (60, 52), (12, 12), (36, 38)])
def test_render_kernel_equals_host_and_oracle(sd, H, W):
    env, o = sd.BreakoutEnvironment(_args(screen_height=H, screen_width=W), seed=3), BreakoutOracle(H, W, 3)
    base = env.get_state()
    cases = [dict(bricks=WALL),                                                       # the full wall
             dict(bricks=brick_bit(2, 11), row=10, col=0, paddle=9),                  # empty but one, in the last column
             dict(bricks=brick_bit(1, 0), row=0, col=11, paddle=0),
             dict(bricks=WALL & ~brick_bit(2, 5), row=2, col=5),                      # the ball inside the wall, bricks on every side
             dict(bricks=WALL & ~brick_bit(3, 0), row=3, col=0),
             dict(bricks=WALL, row=4, col=11), dict(bricks=WALL, row=0, col=6),       # below / above the wall, touching it
             dict(bricks=0x555555555 & WALL, row=1, col=1, paddle=5)]                 # every other brick
    for case in cases:
        st = dict(base, **case)
        env.set_state(st); o.set_state(st)
        d = env.render_device()
        assert np.array_equal(d, o.screen()) and np.array_equal(d, env.getScreen()), case
    for t in range(120):                                                             # and along a game
        a = (t * 7 + t // 5) % 3
        env.act(a); o.act(a)
        if t % 4 == 0:
            d = env.render_device()
            assert np.array_equal(d, o.screen()) and np.array_equal(d, env.getScreen()), t
        if o.terminal:
            env.restart(); o.restart()


@pytest.mark.parametrize("variant", ["uniform", "prioritized"])
def test_fused_act_step_equals_host_driven(sd, variant):
    """300 steps of sdqn_net_act_step_env against sdqn_env_step + sdqn_env_screen + add: ring mirror (it wraps twice), state-buffer
    window and metadata bit for bit"""
    kw = dict(uniform={}, prioritized=dict(prioritized_replay=True))[variant]
    args = _args(batch_size=32, random_seed=11, target_steps=100, **kw)
    steps, size = 300, 120
    sets = []
    for fused in (False, True):
        env, buf, mem = sd.BreakoutEnvironment(args, seed=77), sd.DeviceStateBuffer(args), sd.ReplayMemory(size, args)
        sets.append((fused, env, buf, mem, sd.DeepQNetwork(3, args)))
    actions = np.random.RandomState(5).randint(0, 3, steps)
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
    assert log[0] == log[1] and any(x[2] for x in log[0]) and any(x[1] for x in log[0])
    m0, m1 = sets[0][3], sets[1][3]
    assert (m0.count, m0.current) == (m1.count, m1.current) == (size, steps % size)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    d0, d1 = _device_ring(m0), _device_ring(m1)
    assert len(d0) >= size - 8 and np.array_equal(d0, d1)
    assert np.array_equal(d1, np.asarray(m1.screens)[:len(d1)])       # the kernel-rendered mirror == the host-rendered ring
    assert (d1 == 64).any() and (d1 == 255).any()
    mbs = []
    for m in (m0, m1):
        random.seed(1)
        mbs.append([np.array(x) for x in m.getMinibatch()])
    for x, y in zip(*mbs):
        assert np.array_equal(x, y)
    if variant == "prioritized":
        assert np.array_equal(m0.priorities(), m1.priorities())


def _check_against_oracle(net, env, N, steps, eps, seed, check_q):
    B = net.batch_size
    out = net.evaluate(env, N, steps, eps, seed, trace=True)
    o = BreakoutEvalOracle(N, net.history_length, env.dims[0], env.dims[1], eps, seed, env.balls_per_episode)
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


@pytest.mark.parametrize("N", [32, 5])
def test_evaluate_equals_the_oracle_float32(sd, N):
    args = _args(batch_size=32, random_seed=4)
    net, env = sd.DeepQNetwork(3, args), sd.BreakoutEnvironment(args, seed=1)
    before = env.get_state()
    out, explored = _check_against_oracle(net, env, N, 150, 0.1, 1234 + N, check_q=True)
    assert env.get_state() == before
    assert out["missed"].sum() > 0 and out["episodes"].sum() > 0 and out["reward"].sum() == out["caught"].sum()
    assert explored > 0
    with pytest.raises(AssertionError):
        net.evaluate(env, 33, 10)
    with pytest.raises(AssertionError):
        net.evaluate(sd.BreakoutEnvironment(_args(screen_height=96, screen_width=96), seed=1), 4, 10)
    with pytest.raises(AssertionError):
        sd.DeepQNetwork(4, args).evaluate(env, 4, 10)                # a network of 4 actions cannot play a game of 3


@pytest.mark.parametrize("kw", [dict(datatype="float16", batch_size=32), dict(datatype="float64", batch_size=8, screen_height=36, screen_width=38)])
def test_evaluate_other_configurations(sd, kw):
    args = _args(random_seed=6, **kw)
    net, env = sd.DeepQNetwork(3, args), sd.BreakoutEnvironment(args, seed=2)
    _check_against_oracle(net, env, 8, 60, 0.1, 99, check_q=False)


@pytest.mark.parametrize("H,W,eps", [(84, 84, 1.0), (84, 84, 0.3), (36, 38, 1.0)])
def test_collect_equals_the_oracle(sd, H, W, eps):
    """N = 4 lanes of 24 slots, 60 locksteps (every lane wraps 2.5 times), one-ball episodes so that every lane holds terminals;
    epsilon 1 (no forward runs) and 0.3 (traced: the oracle replays the run from the library's own Q rows, which are the forward of
    the oracle's states); 36 x 38: a generic net and the byte path of the collect kernel"""
    N, steps = 4, 60
    args = _args(batch_size=32, screen_height=H, screen_width=W, breakout_balls=1, random_seed=3)
    net, env, mem = sd.DeepQNetwork(3, args), sd.BreakoutEnvironment(args, seed=1), sd.ReplayMemory(N * 24, args)
    assert net.step_structure()[0] == ("fused" if (H, W) == (84, 84) else "generic")
    mem.set_lanes(N)
    out = net.collect(env, mem, N, steps, eps, seed=5, trace=eps < 1.0)
    o = BreakoutCollectOracle(N, N * 24, 4, H, W, 5, env.balls_per_episode)
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
    assert out["steps"].tolist() == [steps] * N and out["episodes"].sum() == out["missed"].sum() > 0
    assert np.array_equal(mem.getState(10), o.screens[7:11])


def test_collect_continues_across_calls(sd):
    rings = []
    for parts in ((60,), (20, 40)):
        args = _args(batch_size=32, breakout_balls=1, random_seed=4)
        net, env, mem = sd.DeepQNetwork(3, args), sd.BreakoutEnvironment(args, seed=1), sd.ReplayMemory(96, args)
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
    # the copies on the net handle play ONE game: a catch environment cannot resume breakout's copies
    net, mem = sd.DeepQNetwork(3, _args(batch_size=32)), sd.ReplayMemory(96, _args(batch_size=32))
    mem.set_lanes(4)
    net.collect(sd.BreakoutEnvironment(_args(), seed=1), mem, 4, 2, 1.0, seed=1)
    with pytest.raises(AssertionError):
        net.collect(sd.CatchEnvironment(_args(), seed=1), mem, 4, 1, 1.0)
    net.collect(sd.BreakoutEnvironment(_args(), seed=1), mem, 4, 1, 1.0)


def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


def test_launches_per_lockstep(sd):
    args = _args(batch_size=32)
    net, env, mem = sd.DeepQNetwork(3, args), sd.BreakoutEnvironment(args, seed=1), sd.ReplayMemory(320, args)
    mem.set_lanes(32)
    net.collect(env, mem, 32, 2, 1.0, seed=1)
    states = np.zeros((32, 4, 84, 84), np.uint8)
    forward = _counts(net, lambda: net.predict(states))
    assert forward and COLLECT not in forward
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 1.0)) == {COLLECT: 3}          # epsilon >= 1: one kernel
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 0.3)) == dict(forward, **{COLLECT: 3})   # else the forward's launches plus one
    assert _counts(net, lambda: net.collect(env, mem, 32, 2, 0.9, epsilon_step=0.1)) == dict(forward, **{COLLECT: 6})


def test_training_reads_lanes_correctly(sd):
    """three train_from_memory steps on the collected lanes: the windows the lane sampler picks, gathered from the device, are slices
    of the oracle's ring, and the steps move the net"""
    args = _args(batch_size=32, breakout_balls=1, random_seed=3, target_steps=100)
    env, mem, net = sd.BreakoutEnvironment(args, seed=1), sd.ReplayMemory(96, args), sd.DeepQNetwork(3, args)
    mem.set_lanes(4)
    net.collect(env, mem, 4, 60, 1.0, seed=5)
    o = BreakoutCollectOracle(4, 96, 4, 84, 84, 5, env.balls_per_episode)
    for _ in range(60):
        o.lockstep(1.0)
    w0 = [np.array(w) for w in net.get_weights()]
    seen_done = seen_reward = False
    for s in range(3):
        random.seed(100 + s)
        net.train_from_memory(mem, 1)
        idx, _ = o.sample(MT19937(100 + s), 1, 32)
        mb = o.gather(idx, 1, args.discount_rate, args.min_reward, args.max_reward)
        got = mem.gather(idx)
        for x, y in zip(got, mb):
            assert np.array_equal(np.asarray(x), y)
        seen_done |= bool(mb[4].any()); seen_reward |= bool(mb[2].any())
    assert seen_done and seen_reward
    assert any(not np.array_equal(a, b) for a, b in zip(w0, net.get_weights()))


def test_main_loop_on_breakout(sd, tmp_path):
    from simple_dqn_amd import main
    path = str(tmp_path / "breakout.csv")
    args = _args(environment="breakout", train_envs=8, eval_envs=8, replay_size=800, random_steps=320, train_steps=80, test_steps=200,
                 epochs=1, batch_size=32, random_seed=5, target_steps=40, exploration_decay_steps=400, csv_file=path, num_actions=3,
                 synthetic_frame_pool=0, game="breakout", visualization_file=None, visualization_filters=4)
    st = main.run(args)
    rows = list(csv.reader(open(path)))
    assert [r[1] for r in rows[1:]] == ["random", "train", "test"] and len(rows) == 4
    assert [int(r[2]) for r in rows[1:]] == [320, 80, 200]
    assert st.env.name() == "breakout" and st.mem.lanes[0] == 8 and st.net.train_iterations == 80 // 4
