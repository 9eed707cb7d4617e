"""The game "breakout" without a device: the library's host functions against the independent oracle
(tests/breakout_oracle.py) bit for bit over long random trajectories and from hand-made states, the refusals of the new entry points,
the command line and bindings, and the ISA census of the breakout kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
from breakout_oracle import WALL, BreakoutOracle, brick_bit  # noqa: E402

SIDE_GEOMETRIES = [(12, 12), (36, 38), (96, 96)]
SEEDS = [1, 2, 3]
STEPS = 20000
TRAJECTORY_BALLS = 30


def _env(H, W, seed, balls=3, cls=None):
    args = type("A", (), dict(screen_height=H, screen_width=W))()
    return (cls or sd.BreakoutEnvironment)(args, seed=seed, balls_per_episode=balls)


@pytest.mark.parametrize("seed", SEEDS)
def test_long_trajectory_equals_the_oracle(seed):
    """20 000 pseudo-random actions: the state POD, reward, terminal and every byte of the 84 x 84 frame at every step; every 50th step
    the frame at 12 x 12, 36 x 38 (cells 3 x 3, two remainder columns) and 96 x 96.  The ORACLE's trajectory must contain every rule:
    30 balls per episode, because a random policy's wall of a 3-ball episode hardly ever opens as far as the top wall (seeds 1, 2, 3 at 30
    balls: >= 39 top-wall reflections, >= 50 terminals, >= 119 boxed-in hits each on the oracle alone; the refill needs a better player
    and is a set-state case below)."""
    env, o = _env(84, 84, seed * 7919 + 1, TRAJECTORY_BALLS), BreakoutOracle(84, 84, seed * 7919 + 1, TRAJECTORY_BALLS)
    side = [(_env(H, W, 0), BreakoutOracle(H, W, 0)) for H, W in SIDE_GEOMETRIES]
    pol = np.random.RandomState(seed)
    actions = pol.randint(0, 3, STEPS)
    assert env.numActions() == 3 and env.name() == "breakout"
    assert env.get_state() == o.state() and np.array_equal(env.getScreen(), o.screen())
    for t in range(STEPS):
        a = int(actions[t])
        r, ro = env.act(a), o.act(a)
        assert (r, env.isTerminal()) == (ro, o.terminal), (seed, t)
        st = env.get_state()
        assert st == o.state(), (seed, t)
        assert np.array_equal(env.getScreen(), o.screen()), (seed, t)
        assert not (st["row"] in (1, 2, 3) and st["bricks"] & brick_bit(st["row"], st["col"])) and st["row"] <= 10
        if t % 50 == 0:
            for e2, o2 in side:
                e2.set_state(st); o2.set_state(o.state())
                assert np.array_equal(e2.getScreen(), o2.screen()), (seed, t, e2.dims)
        if o.terminal:
            env.restart(); o.restart()
            assert env.get_state() == o.state() and not env.isTerminal()
    ev = o.events
    print("seed %d: %s" % (seed, ev))
    for k in ("brick", "boxed", "paddle_left", "paddle_middle", "paddle_right", "side_wall", "top_wall", "lost", "terminal"):
        assert ev[k] >= 1, (k, ev)


def _one_step(state, action, balls=3):
    env, o = _env(84, 84, 5, balls), BreakoutOracle(84, 84, 5, balls)
    base = dict(env.get_state(), **state)
    env.set_state(base); o.set_state(base)
    assert env.get_state() == o.state() == base and np.array_equal(env.getScreen(), o.screen())
    r, ro = env.act(action), o.act(action)
    assert (r, env.isTerminal()) == (ro, o.terminal)
    assert env.get_state() == o.state() and np.array_equal(env.getScreen(), o.screen())
    return r, env.get_state()


def test_set_state_cases():
    # one brick left, hit from below by a ball inside the (empty) wall: 36 again, the ball leaves the new wall downwards
    r, st = _one_step(dict(row=2, col=4, dx=1, dy=-1, bricks=brick_bit(1, 5)), 0)
    assert (r, st["bricks"], st["row"], st["col"], st["dy"]) == (1, WALL, 4, 5, 1)
    # one brick left, hit from above: 36 again, the ball keeps row 0 and goes up
    r, st = _one_step(dict(row=0, col=4, dx=1, dy=1, bricks=brick_bit(1, 5)), 0)
    assert (r, st["bricks"], st["row"], st["col"], st["dy"]) == (1, WALL, 0, 5, -1)
    # one brick left, hit from below the wall: the ball keeps row 4
    r, st = _one_step(dict(row=4, col=6, dx=-1, dy=-1, bricks=brick_bit(3, 5)), 0)
    assert (r, st["bricks"], st["row"], st["col"], st["dy"]) == (1, WALL, 4, 5, 1)
    # a brick above and a brick beside the ball (the boxed-in case): one breaks, the ball keeps its cell, dx and dy flip
    r, st = _one_step(dict(row=3, col=8, dx=1, dy=-1, bricks=WALL & ~brick_bit(3, 8)), 0)
    assert (r, st["row"], st["col"], st["dx"], st["dy"], st["bricks"]) == (1, 3, 8, -1, 1, WALL & ~brick_bit(3, 8) & ~brick_bit(2, 9))
    # ball at row 0 moving up: the top wall sends it to row 1 ... when no brick stands there
    r, st = _one_step(dict(row=0, col=3, dx=1, dy=-1, bricks=WALL & ~brick_bit(1, 4)), 0)
    assert (r, st["row"], st["col"], st["dy"]) == (0, 1, 4, 1)
    # ... and into a brick of row 1 when one does: it breaks, the ball keeps row 0 and goes up again
    r, st = _one_step(dict(row=0, col=3, dx=1, dy=-1, bricks=WALL), 0)
    assert (r, st["row"], st["col"], st["dy"], st["bricks"]) == (1, 0, 4, -1, WALL & ~brick_bit(1, 4))
    # corners with dx pointing into the wall
    r, st = _one_step(dict(row=0, col=0, dx=-1, dy=-1, bricks=0xFFF << 12), 0)
    assert (r, st["row"], st["col"], st["dx"], st["dy"]) == (0, 1, 1, 1, 1)
    r, st = _one_step(dict(row=0, col=11, dx=1, dy=-1, bricks=0xFFF << 12), 0)
    assert (r, st["row"], st["col"], st["dx"], st["dy"]) == (0, 1, 10, -1, 1)
    r, st = _one_step(dict(row=10, col=11, dx=1, dy=1, paddle=9), 0)           # bottom right corner: lands on the paddle's middle cell
    assert (r, st["row"], st["col"], st["dx"], st["dy"], st["balls"]) == (0, 10, 10, -1, -1, 0)
    r, st = _one_step(dict(row=10, col=0, dx=-1, dy=1, paddle=4), 0)            # bottom left corner, no paddle there: lost
    assert (r, st["row"], st["dy"], st["balls"], st["terminal"]) == (0, 4, 1, 1, 0)
    # above the paddle's left, middle and right cells
    r, st = _one_step(dict(row=10, col=3, dx=1, dy=1, paddle=4), 0)
    assert (st["row"], st["col"], st["dx"], st["dy"]) == (10, 4, -1, -1)
    r, st = _one_step(dict(row=10, col=4, dx=1, dy=1, paddle=4), 0)
    assert (st["row"], st["col"], st["dx"], st["dy"]) == (10, 5, 1, -1)
    r, st = _one_step(dict(row=10, col=6, dx=-1, dy=1, paddle=4), 0)
    assert (st["row"], st["col"], st["dx"], st["dy"]) == (10, 5, -1, -1)
    r, st = _one_step(dict(row=10, col=7, dx=-1, dy=1, paddle=4), 0)
    assert (st["row"], st["col"], st["dx"], st["dy"]) == (10, 6, 1, -1)
    # the paddle moves first: the ball beside it is caught by the move, and the last ball ends the episode
    r, st = _one_step(dict(row=10, col=8, dx=-1, dy=1, paddle=4), 2)
    assert (st["row"], st["col"], st["dx"], st["paddle"]) == (10, 7, 1, 5)
    r, st = _one_step(dict(row=10, col=8, dx=-1, dy=1, paddle=4, balls=2), 1)
    assert (r, st["balls"], st["terminal"], st["row"], st["bricks"]) == (0, 3, 1, 4, WALL)


def test_refusals():
    lib, h = sd.load(), C.c_void_p()
    for name in (b"pong", b"Breakout", b"", b"catch "):
        assert lib.sdqn_env_create(C.byref(h), name, 84, 84, 0, 3) == -1
        assert b"catch" in lib.sdqn_last_error() and b"breakout" in lib.sdqn_last_error()
    assert lib.sdqn_env_create(C.byref(h), b"breakout", 84, 84, 0, 0) == -1
    for H, W in ((11, 84), (84, 11)):
        with pytest.raises(AssertionError):
            _env(H, W, 0)
    b, c = _env(84, 84, 1), _env(84, 84, 1, 10, sd.CatchEnvironment)
    assert b.name() == "breakout" and c.name() == "catch"
    cs, bs = _lib.EnvState(), _lib.EnvStateBreakout()
    assert lib.sdqn_env_get_state(b._h, C.byref(cs)) == -1 and lib.sdqn_env_set_state(b._h, C.byref(cs)) == -1
    assert lib.sdqn_env_get_state_breakout(c._h, C.byref(bs)) == -1 and lib.sdqn_env_set_state_breakout(c._h, C.byref(bs)) == -1
    assert lib.sdqn_env_get_state(c._h, C.byref(cs)) == 0 and lib.sdqn_env_get_state_breakout(b._h, C.byref(bs)) == 0
    with pytest.raises(AssertionError):
        b.act(3)
    with pytest.raises(AssertionError):
        b.act(-1)
    good = dict(b.get_state(), row=5, col=5, dx=1, dy=-1, paddle=3, balls=1, terminal=0, bricks=WALL)
    b.set_state(good)
    assert b.get_state() == good
    for bad in (dict(row=11), dict(row=-1), dict(col=12), dict(col=-1), dict(dx=0), dict(dx=2), dict(dx=-2), dict(dy=0), dict(dy=2),
                dict(paddle=10), dict(paddle=-1), dict(balls=-1), dict(terminal=2), dict(terminal=-1), dict(pad=1),
                dict(bricks=WALL | (1 << 36)), dict(bricks=1 << 63), dict(row=2, col=7), dict(row=1, col=0, bricks=1)):
        with pytest.raises(AssertionError):
            b.set_state(dict(good, **bad))
        assert b.get_state() == good                                     # a refused state changes nothing
    b.set_state(dict(good, row=2, col=7, bricks=WALL & ~brick_bit(2, 7)))  # the same cell without its brick is fine


def test_state_round_trip_and_restart():
    env, o = _env(60, 52, 99), BreakoutOracle(60, 52, 99)
    for t in range(157):
        env.act(t % 3); o.act(t % 3)
    saved = env.get_state()
    tail = [(env.act(t % 3), env.get_state()) for t in range(300)]
    env.set_state(saved)
    assert env.get_state() == saved == o.state() and np.array_equal(env.getScreen(), o.screen())
    assert [(env.act(t % 3), env.get_state()) for t in range(300)] == tail
    env.restart(); o.set_state(env.get_state())
    st = env.get_state()
    assert (st["row"], st["dy"], st["paddle"], st["balls"], st["terminal"], st["bricks"]) == (4, 1, 4, 0, 0, WALL)
    s = env.getScreen()                                                  # cells 5 x 4: columns 48..51 are never written
    assert not s[:, 48:].any() and (s == 64).sum() == 36 * 20 and (s == 128).sum() == 3 * 20 and (s == 255).sum() == 20
    assert np.array_equal(s, o.screen())


def test_command_line_and_bindings():
    from simple_dqn_amd import main
    a = main.build_parser().parse_args(["--environment", "breakout", "--eval_envs", "32", "--train_envs", "32", "--replay_size", "20000"])
    assert (a.environment, a.eval_envs, a.breakout_balls, a.catch_balls) == ("breakout", 32, 3, 10)
    assert main.check_train_envs(a) == 32
    assert main.build_parser().parse_args(["--environment", "breakout", "--breakout_balls", "5"]).breakout_balls == 5
    assert "BreakoutEnvironment" in sd.__all__ and sd.BreakoutEnvironment.__mro__[1] is sd.CatchEnvironment.__mro__[1]
    assert _env(84, 84, 0, None).balls_per_episode == 3
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in ("sdqn_env_get_state_breakout", "sdqn_env_set_state_breakout", "sdqn_env_name"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name + "(" in hdr
    assert "sdqn_env_state_breakout;" in hdr
    S = _lib.EnvStateBreakout
    assert C.sizeof(S) == 48 and S.bricks.offset == 32 and S.rng.offset == 40 and S.dy.offset == 12 and S.paddle.offset == 16
    assert C.sizeof(_lib.EnvState) == 32


def test_isa_census_of_the_breakout_kernels():
    """registers, LDS and scratch of the breakout kernels as the compiler reports them (tools/isa_census.py)"""
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_env.hip")
    names = [r["name"] for r in rows]
    for kernel in ("breakout_render_kernel", "breakout_eval_kernel", "breakout_collect_kernel",
                   "catch_render_kernel", "catch_eval_kernel", "catch_collect_kernel"):
        assert len([n for n in names if kernel in n]) == 1, (kernel, names)
    for r in rows:
        print("%s: vgpr %d agpr %d lds %d scratch %d" % (r["name"], r["vgpr"], r["agpr"], r["lds"], r["scratch"]))
    for kernel in ("breakout_eval_kernel", "breakout_collect_kernel"):
        k = [r for r in rows if kernel in r["name"]][0]
        assert k["scratch"] == 0 and k["vgpr"] + k["agpr"] <= 128 and k["lds"] <= 64, k
    assert not [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    src = "".join(open(os.path.join(isa_census.CSRC, f)).read() for f in ("sdqn_env.hip", "env_catch.h", "env_breakout.h"))
    assert "atomic" not in src.lower()
