"""The game "freeway" without a device: the library's host functions against the independent oracle
(tests/freeway_oracle.py) bit for bit over long random trajectories and from hand-made states, the refusals of the new entry points,
frame skip and sticky actions against tests/dynamics_oracle.py's rule, the command line and bindings, the ISA census of the freeway
kernels, and the device renderer's text walked on the host (tests/freeway_render_walk.cpp)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
from catch_oracle import SplitMix, stream_seed  # noqa: E402
from freeway_oracle import EVENTS, FreewayOracle, pack, single_game, unpack  # noqa: E402

SIDE_GEOMETRIES = [(12, 12), (36, 38), (96, 96)]
SEEDS = [1, 2, 3]
STEPS = 20000                 # pseudo-random actions ...
UP_STEPS = 1500               # ... and then "always up": a random policy crosses a handful of times in 20 000 steps, this one every few dozen
TICKS = 500
LANE_MASK = (1 << 40) - 1


def _env(H, W, seed, ticks=TICKS, cls=None, **dyn):
    args = type("A", (), dict(screen_height=H, screen_width=W, **dyn))()
    return (cls or sd.FreewayEnvironment)(args, seed=seed, balls_per_episode=ticks)


def _lanes(cars=None, timers=None, periods=None, default=(0, 5, 5)):
    """the three words of a traffic picture: every row's car on column default[0] with timer default[1] and period default[2], except
    the rows named in the dicts"""
    out = {}
    for k, given, d in (("cars", cars, default[0]), ("timers", timers, default[1]), ("periods", periods, default[2])):
        v = [d] * 10
        for r, x in (given or {}).items():
            v[r - 1] = x
        out[k] = pack(v)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_long_trajectory_equals_the_oracle(seed):
    """20 000 pseudo-random actions, then 1 500 times "up": the state POD, reward, terminal and every byte of the 84 x 84 frame at every
    step; every 50th step the frame at 12 x 12, 36 x 38 (cells 3 x 3, two remainder columns) and 96 x 96.  The ORACLE's trajectory must
    contain every rule.  On the oracle alone, seeds 1, 2, 3 over the 20 000 random actions: 833 .. 848 hits by walking, 473 .. 524 hits
    by a car, 3 873 .. 3 951 wraps to the right and 3 824 .. 4 245 to the left, 40 terminals, 46 .. 54 shuffles — and 5, 13 and 6
    crossings: a random policy almost never crosses, so the scripted "always up" segment behind it supplies them by the dozen."""
    env, o = _env(84, 84, seed * 7919 + 1), FreewayOracle(84, 84, seed * 7919 + 1, TICKS)
    side = [(_env(H, W, 0), FreewayOracle(H, W, 0, TICKS)) for H, W in SIDE_GEOMETRIES]
    actions = np.concatenate([np.random.RandomState(seed).randint(0, 3, STEPS), np.ones(UP_STEPS, np.int64)])
    assert env.numActions() == 3 and env.name() == "freeway"
    assert env.get_state() == o.state() and np.array_equal(env.getScreen(), o.screen())
    random_part = None
    for t in range(STEPS + UP_STEPS):
        if t == STEPS:
            random_part = dict(o.events)
        a = int(actions[t])
        r, ro = env.act(a), o.act(a)
        assert (r, env.isTerminal()) == (ro, o.terminal), (seed, t)
        st = env.get_state()
        assert st == o.state(), (seed, t)
        assert np.array_equal(env.getScreen(), o.screen()), (seed, t)
        assert 1 <= st["row"] <= 11 and not (st["row"] <= 10 and unpack(st["cars"])[st["row"] - 1] == 6)      # after a step: never on row 0, in no car
        if t % 50 == 0:
            for e2, o2 in side:
                e2.set_state(st); o2.set_state(o.state())
                assert np.array_equal(e2.getScreen(), o2.screen()), (seed, t, e2.dims)
        if o.terminal:
            env.restart(); o.restart()
            assert env.get_state() == o.state() and not env.isTerminal()
    print("seed %d: random part %s, all %s" % (seed, random_part, o.events))
    for k in EVENTS:
        assert random_part[k] >= 5, (k, random_part)
    assert o.events["crossing"] >= random_part["crossing"] + 20, o.events


def _one_step(state, action, ticks=TICKS):
    env, o = _env(84, 84, 5, ticks), FreewayOracle(84, 84, 5, ticks)
    base = dict(env.get_state(), **state)
    env.set_state(base); o.set_state(base)
    assert env.get_state() == o.state() == base and np.array_equal(env.getScreen(), o.screen())
    before = dict(o.events)
    r, ro = env.act(action), o.act(action)
    assert (r, env.isTerminal()) == (ro, o.terminal)
    assert env.get_state() == o.state() and np.array_equal(env.getScreen(), o.screen())
    return r, env.get_state(), [k for k in EVENTS if o.events[k] != before[k]]


def test_set_state_cases():
    # nothing happens: every timer counts down, no car moves
    r, st, ev = _one_step(dict(row=7, ticks=3, **_lanes()), 0)
    assert (r, st["row"], st["ticks"], st["terminal"], ev) == (0, 7, 4, 0, []) and unpack(st["timers"]) == [4] * 10 and unpack(st["cars"]) == [0] * 10
    # the chicken walks into a standing car: back to row 11, no reward
    r, st, ev = _one_step(dict(row=5, **_lanes(cars={4: 6})), 1)
    assert (r, st["row"], ev) == (0, 11, ["walked_into_car"]) and unpack(st["cars"])[3] == 6
    # ... and into a car that leaves column 6 in this very tick: the walk is judged before the traffic moves, it is a hit (row 4 drives left)
    r, st, ev = _one_step(dict(row=5, **_lanes(cars={4: 6}, timers={4: 1}, periods={4: 3})), 1)
    assert (r, st["row"], ev) == (0, 11, ["walked_into_car"]) and (unpack(st["cars"])[3], unpack(st["timers"])[3]) == (5, 3)
    # DESIGN.md §25, decided case 1: a car reaches column 6 in the same tick the chicken arrives on its row: a car drove into it
    r, st, ev = _one_step(dict(row=6, **_lanes(cars={5: 5}, timers={5: 1}, periods={5: 2})), 1)           # row 5 drives right
    assert (r, st["row"], ev) == (0, 11, ["hit_by_car"]) and (unpack(st["cars"])[4], unpack(st["timers"])[4]) == (6, 2)
    r, st, ev = _one_step(dict(row=3, **_lanes(cars={4: 7}, timers={4: 1}, periods={4: 1})), 2)           # row 4 drives left, walking down
    assert (r, st["row"], ev) == (0, 11, ["hit_by_car"]) and unpack(st["cars"])[3] == 6
    # ... and a car whose timer has a tick to go does not move: the chicken stands beside it
    r, st, ev = _one_step(dict(row=6, **_lanes(cars={5: 5}, timers={5: 2}, periods={5: 2})), 1)
    assert (r, st["row"], ev) == (0, 5, []) and (unpack(st["cars"])[4], unpack(st["timers"])[4]) == (5, 1)
    # a car drives into a chicken that stays
    r, st, ev = _one_step(dict(row=8, **_lanes(cars={8: 7}, timers={8: 1})), 0)
    assert (r, st["row"], ev) == (0, 11, ["hit_by_car"])
    # one hit per tick: the chicken walked into the car of row 5 and is on row 11 when the traffic moves
    r, st, ev = _one_step(dict(row=6, **_lanes(cars={5: 6, 6: 1}, timers={5: 1})), 1)
    assert (r, st["row"], ev) == (0, 11, ["walked_into_car"])
    # the wraps: an odd row drives off the right edge, an even row off the left one
    r, st, ev = _one_step(dict(row=11, **_lanes(cars={3: 11}, timers={3: 1})), 0)
    assert ev == ["wrap_right"] and unpack(st["cars"])[2] == 0
    r, st, ev = _one_step(dict(row=11, **_lanes(cars={8: 0}, timers={8: 1})), 0)
    assert ev == ["wrap_left"] and unpack(st["cars"])[7] == 11
    # the clamps: down on row 11 stays there
    r, st, ev = _one_step(dict(row=11, **_lanes()), 2)
    assert (r, st["row"], ev) == (0, 11, [])
    # a crossing: +1, back on row 11, new traffic from one draw, every timer at its period (the traffic did not move in this tick)
    r, st, ev = _one_step(dict(row=1, ticks=10, crossings=2, **_lanes()), 1)
    assert (r, st["row"], st["ticks"], st["crossings"], st["terminal"], ev) == (1, 11, 11, 3, 0, ["crossing", "shuffle"])
    assert st["timers"] == st["periods"] and st["cars"] != 0 and unpack(st["cars"])[9] != 6
    # ... on the episode's last tick: the reward and the terminal come together
    r, st, ev = _one_step(dict(row=1, ticks=TICKS - 1, **_lanes()), 1)
    assert (r, st["ticks"], st["crossings"], st["terminal"], ev) == (1, TICKS, 1, 1, ["crossing", "shuffle", "terminal"])
    # the last tick without one
    r, st, ev = _one_step(dict(row=11, ticks=TICKS - 1, **_lanes()), 0)
    assert (r, st["ticks"], st["terminal"], ev) == (0, TICKS, 1, ["terminal"])
    r, st, ev = _one_step(dict(row=11, ticks=TICKS - 2, **_lanes()), 0)
    assert (st["ticks"], st["terminal"], ev) == (TICKS - 1, 0, [])
    # DESIGN.md §25, decided case 2: a state set with ticks >= episode_ticks is accepted as it is and ends at its next tick (`>=`)
    r, st, ev = _one_step(dict(row=4, ticks=TICKS + 200, terminal=0, **_lanes()), 0)
    assert (r, st["row"], st["ticks"], st["terminal"], ev) == (0, 4, TICKS + 201, 1, ["terminal"])
    r, st, ev = _one_step(dict(row=4, ticks=7, **_lanes()), 0, ticks=1)
    assert (st["ticks"], st["terminal"]) == (8, 1)
    # decided case 3: a state set on row 0 (no step leaves the chicken there) crosses at its next tick, whatever the action
    for a in (0, 1):
        r, st, ev = _one_step(dict(row=0, **_lanes()), a)
        assert (r, st["row"], st["crossings"], ev) == (1, 11, 1, ["crossing", "shuffle"])
    r, st, ev = _one_step(dict(row=0, **_lanes(cars={1: 6})), 2)          # ... unless it walks down, here into a car
    assert (r, st["row"], ev) == (0, 11, ["walked_into_car"])


def test_the_shuffle():
    """one draw for all ten rows, and the car of row 10 never starts on column 6: the seeds are searched with the draw's arithmetic
    alone (row 10's column is digit 19 of d in the mixed radix 5, 12, 5, 12, ...)"""
    found = {6: None, 5: None}
    for seed in range(400):
        d = SplitMix(seed).next()
        col10 = d // (60 ** 9 * 5) % 12
        if col10 in found and found[col10] is None:
            found[col10] = (seed, d)
    for col10, (seed, d) in found.items():
        env, o = _env(84, 84, seed), FreewayOracle(84, 84, seed, TICKS)
        st = env.get_state()
        assert st == o.state()
        periods, cars = [], []
        for r in range(10):
            periods.append(1 + d % 5); d //= 5
            cars.append(d % 12); d //= 12
        assert cars[9] == col10
        cars[9] = 7 if col10 == 6 else cars[9]
        assert (unpack(st["cars"]), unpack(st["periods"]), st["timers"]) == (cars, periods, st["periods"])
        assert (st["row"], st["ticks"], st["crossings"], st["terminal"], st["pad0"], st["pad1"]) == (11, 0, 0, 0, 0, 0)
        g = SplitMix(seed); g.next()
        assert st["rng"] == g.state                                      # ONE draw


def test_refusals():
    lib, h = sd.load(), C.c_void_p()
    for name in (b"pong", b"Freeway", b"", b"freeway ", b"Breakout", b"catch "):
        assert lib.sdqn_env_create(C.byref(h), name, 84, 84, 0, 3) == -1
        assert all(w in lib.sdqn_last_error() for w in (b"catch", b"breakout", b"freeway"))
    assert lib.sdqn_env_create(C.byref(h), b"freeway", 84, 84, 0, 0) == -1
    assert lib.sdqn_env_create(C.byref(h), b"freeway", 84, 84, 0, -5) == -1
    with pytest.raises(AssertionError):
        _env(84, 84, 0, ticks=0)
    for H, W in ((11, 84), (84, 11)):
        with pytest.raises(AssertionError):
            _env(H, W, 0)
    f, b, c = _env(84, 84, 1), _env(84, 84, 1, 3, sd.BreakoutEnvironment), _env(84, 84, 1, 10, sd.CatchEnvironment)
    assert (f.name(), b.name(), c.name()) == ("freeway", "breakout", "catch")
    cs, bs, fs = _lib.EnvState(), _lib.EnvStateBreakout(), _lib.EnvStateFreeway()
    calls = {"catch": (lib.sdqn_env_get_state, lib.sdqn_env_set_state, cs), "breakout": (lib.sdqn_env_get_state_breakout, lib.sdqn_env_set_state_breakout, bs),
             "freeway": (lib.sdqn_env_get_state_freeway, lib.sdqn_env_set_state_freeway, fs)}
    for env in (f, b, c):
        before = env.get_state()
        for game, (get, put, st) in calls.items():
            if game == env.name():
                assert get(env._h, C.byref(st)) == 0 and put(env._h, C.byref(st)) == 0
            else:
                assert put(env._h, C.byref(st)) == -1 and env.name().encode() in lib.sdqn_last_error()
                assert get(env._h, C.byref(st)) == -1 and game.encode() in lib.sdqn_last_error()
        assert env.get_state() == before                                 # the other games' calls changed nothing
    assert lib.sdqn_env_get_state_freeway(None, C.byref(fs)) == -1 and lib.sdqn_env_set_state_freeway(f._h, None) == -1
    with pytest.raises(AssertionError):
        f.act(3)
    with pytest.raises(AssertionError):
        f.act(-1)
    good = dict(f.get_state(), row=5, ticks=17, crossings=2, terminal=0, **_lanes(cars={5: 3, 10: 11}, timers={5: 2, 1: 1}, periods={5: 4, 1: 1}))
    f.set_state(good)
    assert f.get_state() == good
    bad_cases = [dict(row=12), dict(row=-1), dict(ticks=-1), dict(crossings=-1), dict(terminal=2), dict(terminal=-1), dict(pad0=1), dict(pad1=1),
                 dict(pad1=-1), dict(cars=good["cars"] | (1 << 40)), dict(cars=good["cars"] | (1 << 63)), dict(timers=good["timers"] | (1 << 40)),
                 dict(periods=good["periods"] | (1 << 47)),
                 _lanes(cars={5: 6}, timers={5: 2}, periods={5: 4}),                          # the chicken's row 5, its car on column 6
                 _lanes(cars={7: 12}), _lanes(cars={1: 15}),                                   # a column > 11
                 _lanes(timers={3: 0}), _lanes(timers={10: 0}),                                # a timer of 0
                 _lanes(timers={3: 5}, periods={3: 4}), _lanes(timers={1: 2}, periods={1: 1}),  # a timer beyond its period
                 _lanes(periods={2: 6}, timers={2: 6}), _lanes(periods={9: 15}, timers={9: 1}),  # a period > 5
                 _lanes(periods={4: 0}, timers={4: 0}), dict(periods=0, timers=0)]             # a period of 0
    for bad in bad_cases:
        with pytest.raises(AssertionError):
            f.set_state(dict(good, **bad))
        assert f.get_state() == good                                     # a refused state changes nothing
    f.set_state(dict(good, **_lanes(cars={4: 6, 6: 6})))                 # cars beside the chicken's row on column 6 are fine
    f.set_state(dict(good, row=11, **_lanes(cars=dict((r, 6) for r in range(1, 11)))))
    f.set_state(dict(good, ticks=2 ** 31 - 2, terminal=1))


def test_state_round_trip_and_restart():
    env, o = _env(60, 52, 99), FreewayOracle(60, 52, 99, TICKS)
    for t in range(157):
        a = (1, 1, 0, 1, 2)[t % 5]
        env.act(a); o.act(a)
    saved = env.get_state()
    tail = [(env.act((1, 1, 0)[t % 3]), env.get_state()) for t in range(600)]
    assert any(r for r, _ in tail) and any(s["terminal"] for _, s in tail)
    env.set_state(saved)
    assert env.get_state() == saved == o.state() and np.array_equal(env.getScreen(), o.screen())
    assert [(env.act((1, 1, 0)[t % 3]), env.get_state()) for t in range(600)] == tail
    rng = env.get_state()["rng"]
    env.restart(); o.set_state(env.get_state())
    st = env.get_state()
    g = SplitMix(rng); g.next()
    assert (st["row"], st["ticks"], st["crossings"], st["terminal"], st["rng"]) == (11, 0, 0, 0, g.state) and not env.isTerminal()   # no reseed
    assert st["timers"] == st["periods"] and not (st["cars"] | st["timers"]) & ~LANE_MASK
    s = env.getScreen()                                                  # cells 5 x 4: columns 48..51 are never written
    assert not s[:, 48:].any() and (s == 128).sum() == 10 * 20 and (s == 255).sum() == 20 and not s[:5].any()
    assert np.array_equal(s, o.screen())


@pytest.mark.parametrize("k,p", [(4, 0.0), (1, 0.25), (4, 0.25)])
def test_dynamics_equal_the_oracle(k, p):
    """--frame_skip 4 and --repeat_action_probability 0.25 (env_dynamics.h serves the game unchanged): 2 000 agent steps
    against tests/dynamics_oracle.py's rule applied to the freeway oracle — the summed reward, terminal, the whole state, prev, the
    sticky generator (stream 2) and the frame after every agent step.  Episodes of 30 ticks: 30 is no multiple of 4, so every
    episode's last agent step is cut short by its terminal tick."""
    seed, ticks, steps = 4242 + k, 30, 2000
    env, o = _env(84, 84, seed, ticks, frame_skip=k, repeat_action_probability=p), single_game(84, 84, seed, ticks, k, p)
    d0 = env.get_dynamics()
    assert d0 == dict(frame_skip=k, repeat_action_probability=p, prev_action=0, sticky_rng=stream_seed(seed, 0, 2))
    actions = np.where(np.random.RandomState(k).rand(steps) < 0.6, 1, np.random.RandomState(k + 1).randint(0, 3, steps))
    rewards = episodes = 0
    for t in range(steps):
        a = int(actions[t])
        r, ro = env.act(a), o.act(a)
        assert (r, env.isTerminal()) == (ro, o.terminal) and 0 <= r <= k, t
        d = env.get_dynamics()
        assert env.get_state() == o.state() and (d["prev_action"], d["sticky_rng"]) == (o.prev, o.sticky.state), t
        assert np.array_equal(env.getScreen(), o.screen()), t
        rewards += r
        if o.terminal:
            episodes += 1
            env.restart(); o.restart()
            assert env.get_dynamics()["prev_action"] == 0 and env.get_state() == o.state()
    assert episodes > 50 and rewards > 5
    assert (o.stuck > 0) == (p > 0) and (env.get_dynamics()["sticky_rng"] != d0["sticky_rng"]) == (p > 0)
    assert o.ticks == 30 * episodes + o.game.ticks and (k == 1 or o.ticks < k * steps)


def test_command_line_and_bindings():
    from simple_dqn_amd import main
    from simple_dqn_amd.environment import LIBRARY_GAMES
    a = main.build_parser().parse_args(["--environment", "freeway", "--eval_envs", "32", "--train_envs", "32", "--replay_size", "20000"])
    assert (a.environment, a.eval_envs, a.freeway_ticks, a.breakout_balls, a.catch_balls) == ("freeway", 32, 500, 3, 10)
    assert main.check_train_envs(a) == 32 and main.check_dynamics(a) == (1, 0.0) and main.check_freeway_ticks(a) == 500
    a = main.build_parser().parse_args(["--environment", "freeway", "--freeway_ticks", "120", "--frame_skip", "4", "--repeat_action_probability", "0.25"])
    assert a.freeway_ticks == 120 and main.check_dynamics(a) == (4, 0.25)
    assert sd.FreewayEnvironment(a, seed=1).balls_per_episode == 120 and sd.FreewayEnvironment(a, seed=1).get_dynamics()["frame_skip"] == 4
    for bad in ("0", "-3"):
        args = main.build_parser().parse_args(["--environment", "freeway", "--freeway_ticks", bad, "--random_steps", "0", "--epochs", "0"])
        with pytest.raises(ValueError) as ei:
            main.run(args)                                               # refused before anything touches a device
        assert "--freeway_ticks" in str(ei.value)
    assert LIBRARY_GAMES["freeway"] is sd.FreewayEnvironment and sorted(LIBRARY_GAMES) == ["breakout", "catch", "freeway"]
    assert "FreewayEnvironment" in sd.__all__ and sd.FreewayEnvironment.__mro__[1] is sd.CatchEnvironment.__mro__[1]
    assert _env(84, 84, 0, None).balls_per_episode == 500
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in ("sdqn_env_get_state_freeway", "sdqn_env_set_state_freeway"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name + "(" in hdr
    assert "sdqn_env_state_freeway;" in hdr
    S = _lib.EnvStateFreeway
    assert C.sizeof(S) == 56 and (S.row.offset, S.ticks.offset, S.crossings.offset, S.terminal.offset, S.pad0.offset) == (0, 4, 8, 12, 16)
    assert (S.cars.offset, S.timers.offset, S.periods.offset, S.rng.offset) == (24, 32, 40, 48)
    assert C.sizeof(_lib.EnvState) == 32 and C.sizeof(_lib.EnvStateBreakout) == 48


def test_nothing_above_the_library_names_the_game():
    """Agent, DeepQNetwork and Statistics hand the handle to the library: they do not branch on a game's name"""
    for f in ("agent.py", "deepqnetwork.py", "statistics.py", "replay_memory.py"):
        src = open(os.path.join(ROOT, "simple_dqn_amd", f)).read()
        code = "\n".join(line.split("#")[0] for line in src.split("\n") if "raise ValueError" not in line)
        assert "freeway" not in code.lower() and "Freeway" not in src, f


def test_isa_census_of_the_freeway_kernels():
    """registers, LDS and scratch of the three freeway kernels as the compiler reports them (tools/isa_census.py), next to the six
    existing ones, which are what they were (DESIGN.md §20's and §23's tables)"""
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_env.hip")
    names = [r["name"] for r in rows]
    kernels = ["%s_%s_kernel" % (g, k) for g in ("catch", "breakout", "freeway") for k in ("render", "eval", "collect")]
    for kernel in kernels:
        assert len([n for n in names if kernel in n]) == 1, (kernel, names)
    assert len(rows) == 9
    for r in rows:
        print("%s: vgpr %d agpr %d lds %d scratch %d" % (r["name"], r["vgpr"], r["agpr"], r["lds"], r["scratch"]))
        assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] < 128, r
    for kernel in ("freeway_eval_kernel", "freeway_collect_kernel"):
        k = [r for r in rows if kernel in r["name"]][0]
        assert k["vgpr"] + k["agpr"] <= 64 and k["lds"] == 16, k         # VIEW_WORDS + 1 ints of LDS; half the 128 registers
    k = [r for r in rows if "freeway_render_kernel" in r["name"]][0]
    assert k["vgpr"] + k["agpr"] <= 64 and k["lds"] == 0, k
    assert "atomic" not in open(os.path.join(isa_census.CSRC, "env_freeway.h")).read().lower()


def test_device_renderer_text_equals_the_host_renderer(tmp_path):
    """cursor / advance / pixel walked in 16-byte chunks as render_chunk walks them, against the host renderer's filled rectangles,
    byte for byte, at ten geometries x 3 000 states, for all three games: a stand-alone host program (the headers are plain C++)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "freeway_render_walk")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simple_dqn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "freeway_render_walk.cpp"), "-o", exe])
    out = subprocess.run([exe, "3000"], stdout=subprocess.PIPE, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    for game in ("freeway", "breakout", "catch"):
        assert "%s: 3000 states at each of 10 geometries" % game in out.stdout
