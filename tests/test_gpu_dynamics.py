"""Frame skip and sticky actions on the device: vectorised evaluation and collection against tests/dynamics_oracle.py bit
for bit, the fused act step against its host mirror and the oracle, the defaults against the unwrapped oracles, launch counts, and the
learning test under sticky actions."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import make_args  # noqa: E402
from catch_oracle import CatchOracle, SplitMix, stream_seed  # noqa: E402
from dynamics_oracle import COLLECT, EVAL, DynamicsGame, dynamics_collect_oracle, dynamics_eval_oracle, single_game  # noqa: E402

pytestmark = pytest.mark.gpu
TALLIES = ("steps", "reward", "caught", "missed", "episodes")
Q_TOL = 1e-4          # the tolerance tests/test_gpu_dqn.py uses for predict
LOCKSTEP = "catch_collect(lockstep)"      # the profile's lockstep row counts either game's collect kernel
GEOMETRIES = {"fused": dict(batch_size=32), "generic": dict(batch_size=32, screen_height=36, screen_width=38)}


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=2, breakout_balls=1, eval_envs=0, train_envs=0, frame_skip=1,
             repeat_action_probability=0.0)
    d.update(kw)
    return make_args(**d)


def _env(sd, game, args, seed=1):
    return dict(catch=sd.CatchEnvironment, breakout=sd.BreakoutEnvironment)[game](args, seed=seed)


def _lane_ring(mem):
    """slots [0, fill) of every lane of the HBM mirror, read through the gather kernel"""
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
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(_filled(mem, getattr(mem, name)), _filled(mem, getattr(o, name))), name
    assert np.array_equal(_filled(mem, _lane_ring(mem)), _filled(mem, o.screens))


def _evaluate_against(net, env, o, N, steps, eps, seed):
    """the traces and tallies of evaluate against oracle o, which is fed the library's own Q rows; the window the forward read is
    held to the oracle's byte for byte through the forward itself: predict of the oracle's windows (rows N.. zero, as in the window
    buffer) gives the traced Q rows bit for bit, and within Q_TOL as in the existing evaluation tests"""
    B = net.batch_size
    out = net.evaluate(env, N, steps, eps, seed, trace=True)
    worst, differ = 0.0, 0
    for t in range(steps):
        st = np.zeros((B,) + o.states.shape[1:], np.uint8); st[:N] = o.states
        q = net.predict(st)[:N]
        worst = max(worst, float(np.abs(q.astype(np.float64) - out["q"][t]).max()))
        differ += not np.array_equal(q, out["q"][t])
        a, r, term = o.step(out["q"][t])
        assert np.array_equal(a, out["actions"][t]), t
        assert np.array_equal(r, out["rewards"][t]) and np.array_equal(term, out["terminals"][t]), t
    print("Q of the oracle's windows against the traced rows: max abs err %.3e, %d of %d locksteps not bit-equal" % (worst, differ, steps))
    assert worst < Q_TOL and differ == 0
    for k in TALLIES:
        assert np.array_equal(out[k], o.tally[k]), k
    assert out["steps"].tolist() == [steps] * N
    plain = net.evaluate(env, N, steps, eps, seed)
    for k in TALLIES:
        assert np.array_equal(plain[k], out[k]), k
    return out


@pytest.mark.parametrize("k,p", [(4, 0.0), (1, 0.25), (3, 0.25)])
@pytest.mark.parametrize("geometry", ["fused", "generic"])
@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_evaluate_equals_the_oracle(sd, game, geometry, k, p):
    """N = 3 copies, 60 locksteps, epsilon 0.3: float32 at 84 x 84 (the tuned net) and the generic net at 36 x 38 (the byte path of the
    kernel); short episodes so that terminals fall inside skips"""
    N, steps, eps, seed = 3, 60, 0.3, 77
    args = _args(random_seed=4, frame_skip=k, repeat_action_probability=p, **GEOMETRIES[geometry])
    net, env = sd.DeepQNetwork(3, args), _env(sd, game, args)
    assert net.step_structure()[0] == geometry
    before = (env.get_state(), env.get_dynamics())
    o = dynamics_eval_oracle(game, N, 4, env.dims[0], env.dims[1], eps, seed, env.balls_per_episode, k, p)
    out = _evaluate_against(net, env, o, N, steps, eps, seed)
    assert (env.get_state(), env.get_dynamics()) == before           # the handle's own game is not touched
    assert out["episodes"].sum() > 0 and out["terminals"].any()
    assert sum(g.ticks for g in o.envs) > N * steps or k == 1
    assert (sum(g.stuck for g in o.envs) > 0) == (p > 0)
    if k > 1:
        assert sum(g.ticks for g in o.envs) < N * steps * k           # some agent step was cut short by a terminal


@pytest.mark.parametrize("eps", [1.0, 0.3])
@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_collect_equals_the_oracle(sd, game, eps):
    """N = 3 lanes of 32 slots, 40 locksteps (the lanes wrap) at (3, 0.25): epsilon 1 (no forward runs) and 0.3 (traced: the oracle
    replays the run from the library's own Q rows); then the same 40 locksteps as collect(15) ; collect(25)"""
    N, size, steps, seed, k, p = 3, 96, 40, 5, 3, 0.25
    args = _args(batch_size=32, random_seed=3, frame_skip=k, repeat_action_probability=p)
    runs = []
    for parts in ((40,), (15, 25)):
        net, env, mem = sd.DeepQNetwork(3, args), _env(sd, game, args), sd.ReplayMemory(size, args)
        mem.set_lanes(N)
        outs, s = [], seed
        for n in parts:
            outs.append(net.collect(env, mem, N, n, eps, seed=s, trace=True))
            s = None
        runs.append((mem, outs, _lane_ring(mem)))
    mem, (out,), ring = runs[0]
    o = dynamics_collect_oracle(game, N, size, 4, 84, 84, seed, env.balls_per_episode, k, p)
    for t in range(steps):
        a, r, term = o.lockstep(eps, out["q"][t] if eps < 1.0 else None)
        assert np.array_equal(a, out["actions"][t]) and np.array_equal(r, out["rewards"][t]), t
        assert np.array_equal(term, out["terminals"][t]), t
    assert (o.f, o.p) == (32, 40 % 32) and o.terminals.any() and len(set(o.actions.tolist())) == 3
    assert sum(g.stuck for g in o.games.envs) > 0
    _assert_ring_equals(mem, o)
    for name in TALLIES:
        assert np.array_equal(out[name], o.tally[name]), name
    assert out["steps"].tolist() == [steps] * N
    mem2, outs2, ring2 = runs[1]                                      # prev and the sticky stream persist between the calls
    assert mem2.lanes == mem.lanes
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(mem, name)), np.asarray(getattr(mem2, name))), name
    assert np.array_equal(ring, ring2)
    for name in TALLIES:
        assert np.array_equal(outs2[-1][name], out[name]), name
    for name in ("actions", "rewards", "terminals"):
        assert np.array_equal(np.concatenate([x[name] for x in outs2]), out[name]), name


def _device_window(sd, buf):
    out = np.empty((buf.history_length,) + buf.dims, np.uint8)
    sd._lib.check(sd.load().sdqn_statebuf_read_device(buf._h, sd._lib.ptr(out, C.c_uint8)))
    return out


@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_fused_act_step_equals_its_host_mirror_and_the_oracle(sd, game):
    """200 steps of sdqn_net_act_step_env at (3, 0.25) against sdqn_env_step + sdqn_env_screen + act_step and against the oracle:
    reward, terminal, state, prev, sticky generator, the device window and the ring (it wraps)"""
    k, p, steps, size = 3, 0.25, 200, 120
    args = _args(batch_size=32, random_seed=11, target_steps=100, frame_skip=k, repeat_action_probability=p)
    sets = []
    for fused in (False, True):
        env, buf, mem = _env(sd, game, args, seed=77), sd.DeviceStateBuffer(args), sd.ReplayMemory(size, args)
        sets.append((fused, env, buf, mem, sd.DeepQNetwork(3, args)))
    o = single_game(game, 84, 84, 77, sets[0][1].balls_per_episode, k, p)
    actions = np.random.RandomState(5).randint(0, 3, steps)
    terminals = 0
    for t in range(steps):
        a = int(actions[t])
        ro = o.act(a)
        for fused, env, buf, mem, net in sets:
            if fused:
                r, term = net.act_step_env(buf, mem, env, a)
            else:
                r = env.act(a)
                term = env.isTerminal()
                net.act_step(buf, mem, env.getScreen(), a, r, term)
            assert (r, term) == (ro, o.terminal), (t, fused)
            d = env.get_dynamics()
            assert env.get_state() == o.state() and (d["prev_action"], d["sticky_rng"]) == (o.prev, o.sticky.state), (t, fused)
            assert np.array_equal(env.getScreen(), o.screen()), (t, fused)
        if t % 9 == 0 or o.terminal:
            w = [_device_window(sd, s[2]) for s in sets]
            assert np.array_equal(w[0], w[1]) and np.array_equal(w[1], sets[1][2].getState()), t
            assert np.array_equal(w[1][-1], o.screen()), t
        if o.terminal:
            terminals += 1
            o.restart()
            for s in sets:
                s[1].restart()
                assert s[1].get_dynamics()["prev_action"] == 0
    assert terminals > 2 and o.stuck > 0 and o.ticks < k * steps
    m0, m1 = sets[0][3], sets[1][3]
    assert (m0.count, m0.current) == (m1.count, m1.current) == (size, steps % size)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    assert np.asarray(m1.actions)[:steps % size].tolist() == actions[size:].tolist()      # the ring records the CHOSEN action
    idx = list(range(4, size - 8, 4))
    idx = idx + [idx[-1]] * (32 - len(idx))
    g0, g1 = m0.gather(idx), m1.gather(idx)                           # the kernel-rendered mirror == the host-rendered ring
    assert np.array_equal(np.asarray(g0[0]), np.asarray(g1[0]))
    assert np.array_equal(np.asarray(g1[0]), np.stack([np.asarray(m1.screens)[i - 4:i] for i in idx]))


@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_defaults_are_the_unwrapped_oracles(sd, game):
    """(1, 0), given explicitly or by a namespace that has never heard of the flags: evaluate and collect leave exactly the traces,
    ring and tallies of the existing oracles"""
    N, steps, eps, seed = 3, 40, 0.3, 21
    for kw in (dict(frame_skip=1, repeat_action_probability=0.0), None):
        args = _args(batch_size=32, random_seed=4)
        if kw is None:
            del args.frame_skip, args.repeat_action_probability
        net, env = sd.DeepQNetwork(3, args), _env(sd, game, args)
        assert env.get_dynamics() == dict(frame_skip=1, repeat_action_probability=0.0, prev_action=0, sticky_rng=stream_seed(1, 0, 2))
        _evaluate_against(net, env, EVAL[game](N, 4, 84, 84, eps, seed, env.balls_per_episode), N, steps, eps, seed)
        mem = sd.ReplayMemory(96, args)
        mem.set_lanes(N)
        out = net.collect(env, mem, N, steps, eps, seed=seed, trace=True)
        o = COLLECT[game](N, 96, 4, 84, 84, seed, env.balls_per_episode)
        for t in range(steps):
            a, r, term = o.lockstep(eps, out["q"][t])
            assert np.array_equal(a, out["actions"][t]) and np.array_equal(r, out["rewards"][t]) and np.array_equal(term, out["terminals"][t]), t
        _assert_ring_equals(mem, o)
        for name in TALLIES:
            assert np.array_equal(out[name], o.tally[name]), name


def _counts(net, fn, n=3):
    net.profile(True, -1); net.profile_reset()
    for _ in range(n):
        fn()
    c = {p["name"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    return c


@pytest.mark.parametrize("k,p", [(1, 0.0), (8, 0.9)])
def test_launches_per_lockstep(sd, k, p):
    """the dynamics add no launch: the forward's launches plus one per lockstep, or exactly one while epsilon >= 1"""
    args = _args(batch_size=32, frame_skip=k, repeat_action_probability=p)
    net, env, mem = sd.DeepQNetwork(3, args), _env(sd, "breakout", args), sd.ReplayMemory(320, args)
    mem.set_lanes(32)
    net.collect(env, mem, 32, 2, 1.0, seed=1)
    states = np.zeros((32, 4, 84, 84), np.uint8)
    forward = _counts(net, lambda: net.predict(states))
    assert forward and LOCKSTEP not in forward
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 1.0)) == {LOCKSTEP: 3}
    assert _counts(net, lambda: net.collect(env, mem, 32, 1, 0.3)) == dict(forward, **{LOCKSTEP: 3})


# ---- the learning test: tests/test_gpu_catch.py's task and command line with --train_envs 32 --eval_envs 32 and sticky actions ----------
STICKY_P = 0.25
CRITERION_BALLS = 5000
# twice the slowest first crossing of the criterion among seeds 1, 2, 3, evaluated every 5 000 environment steps over 60 000: all three
# first met it at the 10 000-step evaluation (tools/dynamics_curves.py; profiles/dynamics_curves.json; the table in DESIGN.md §23)
BUDGET_STEPS = 20000


def _per_ball_on_the_oracle(policy, p, balls=CRITERION_BALLS, seed=2016):
    """mean reward per ball of `policy(game, draw)` on the Python oracle under sticky actions p (frame skip 1)"""
    env = DynamicsGame(CatchOracle(84, 84, seed), 1, p, stream_seed(seed, 0, 2))
    pol = SplitMix(seed ^ 0xABCDEF)
    total = landed = 0
    while landed < balls:
        r = env.act(policy(env, pol.next()))
        if r:
            total += r
            landed += 1
        if env.terminal:
            env.restart()
    return total / float(landed)


def _landing_column_policy(env, _):
    target = min(max(env.landing_column() - 1, 0), 9)
    return 0 if env.paddle == target else (1 if env.paddle > target else 2)


@functools.lru_cache(maxsize=None)
def criterion(p=STICKY_P):
    """half-way between the uniformly random policy and the landing_column policy, both played by the oracle under the same dynamics"""
    rnd = _per_ball_on_the_oracle(lambda env, d: d % 3, p)
    best = _per_ball_on_the_oracle(_landing_column_policy, p)
    return rnd, best, (rnd + best) / 2.0


def learning_run(sd, seed, steps, every=None, p=STICKY_P, frame_skip=1):
    """main.run's arguments of tests/test_gpu_catch.py's loop with --train_envs 32 and the dynamics; returns (mean reward per ball of the
    untrained net, [(env steps, mean reward per ball)]), every evaluation on 32 copies under the same dynamics, epsilon 0.05"""
    import random
    from test_gpu_catch import LEARN, per_ball
    from simple_dqn_amd import Agent, CatchEnvironment, DeepQNetwork, ReplayMemory, main
    chunk = every or steps
    args = _args(random_seed=seed, epochs=steps // chunk, train_steps=chunk, catch_balls=10, breakout_balls=3,
                 **dict(LEARN, train_envs=32, eval_envs=32, frame_skip=frame_skip, repeat_action_probability=p))
    main.check_train_envs(args); main.check_dynamics(args)
    random.seed(seed)
    env = CatchEnvironment(args, seed=seed)
    mem, net = ReplayMemory(args.replay_size, args), DeepQNetwork(3, args)
    agent = Agent(env, mem, net, args)
    before = per_ball(net, env, 1000 + seed)
    agent.play_random_vectorised(args.random_steps)
    curve = []
    for epoch in range(args.epochs):
        agent.train_vectorised(chunk, epoch)
        curve.append(((epoch + 1) * chunk, per_ball(net, env, 2000 + seed + epoch)))
    return before, curve


def test_the_agent_learns_catch_under_sticky_actions(sd):
    """catch, --train_envs 32 --eval_envs 32 --repeat_action_probability 0.25, seed 1: after BUDGET_STEPS environment steps the mean
    reward per ball over >= 2 000 balls (evaluate under the same dynamics, epsilon 0.05) reaches the criterion; the untrained net
    stays below it"""
    rnd, best, mid = criterion()
    t0 = time.time()
    before, curve = learning_run(sd, 1, BUDGET_STEPS)
    after = curve[-1][1]
    print("random %.3f, landing-column policy %.3f, criterion %.3f; untrained %.3f, after %d steps %.3f, %.1f s"
          % (rnd, best, mid, before, BUDGET_STEPS, after, time.time() - t0))
    assert rnd < -0.25 and best > 0.8                                # the two policies the criterion stands between are what they are meant to be
    assert before < mid
    assert after >= mid
