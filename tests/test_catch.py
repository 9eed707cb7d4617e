"""The game "catch" without a device: the library's host functions against the independent oracle, bit for bit; properties
of the game itself; the command line; the ISA census of the new translation unit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
from catch_oracle import CatchOracle, SplitMix, argmax_first, explore_threshold, mix, stream_seed  # noqa: E402

GEOMETRIES = [(84, 84), (96, 96), (60, 52), (12, 12)]
BASELINE_BALLS = 20000


@functools.lru_cache(maxsize=None)
def random_baseline(balls=BASELINE_BALLS, seed=2016):
    """Mean reward per ball of the uniform-random policy on the ORACLE: the baseline of the learning test (tests/test_gpu_catch.py).
    Actions come from their own splitmix64 stream so the figure is a constant of (balls, seed)."""
    env, pol = CatchOracle(84, 84, seed), SplitMix(seed ^ 0xABCDEF)
    total = landed = 0
    while landed < balls:
        r = env.act(pol.next() % 3)
        if r:
            total += r
            landed += 1
        if env.terminal:
            env.restart()
    return total / float(landed)


def _env(H, W, seed, balls=10):
    args = type("A", (), dict(screen_height=H, screen_width=W))()
    return sd.CatchEnvironment(args, seed=seed, balls_per_episode=balls)


def test_splitmix64_known_answers():
    # the published splitmix64 test vector (seed 1234567): first outputs of the reference implementation
    g = SplitMix(1234567)
    assert [g.next() for _ in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert mix(0) == 0 and stream_seed(0, 0, 0) != stream_seed(0, 0, 1) != stream_seed(0, 1, 0)
    assert explore_threshold(0.0) == 0 and explore_threshold(1.0) == 2 ** 53 and explore_threshold(0.5) == 2 ** 52


@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_host_functions_equal_the_oracle(H, W):
    """>= 20 seeds x >= 2000 pseudo-random actions: reward, terminal, the state POD and every frame byte; restart in mid-episode"""
    for seed in range(20):
        env, o = _env(H, W, seed * 7919 + 1), CatchOracle(H, W, seed * 7919 + 1)
        pol = np.random.RandomState(seed)
        assert env.numActions() == 3
        assert env.get_state() == o.state() and np.array_equal(env.getScreen(), o.screen())
        frames = 0
        for t in range(2000):
            a = int(pol.randint(3))
            r, ro = env.act(a), o.act(a)
            assert (r, env.isTerminal()) == (ro, o.terminal), (seed, t)
            assert env.get_state() == o.state(), (seed, t)
            if t % 7 == 0 or ro or seed == 0:                         # every frame for one seed, a sample + every landing for the others
                assert np.array_equal(env.getScreen(), o.screen()), (seed, t)
                frames += 1
            if o.terminal or t in (333, 1500):                       # 333 / 1500: restart with balls in flight
                env.restart(); o.restart()
                assert env.get_state() == o.state() and not env.isTerminal()
                assert np.array_equal(env.getScreen(), o.screen())
        assert frames > 280


def test_remainder_pixels_stay_zero_and_cells_are_where_they_belong():
    env = _env(60, 52, 5)                                            # cells 5 x 4: 60 x 48 used, columns 48..51 never written
    for t in range(300):
        env.act(t % 3)
        s = env.getScreen()
        assert not s[:, 48:].any()
        st = env.get_state()
        assert (s == 255).sum() == 5 * 4 and (s == 128).sum() == 5 * 4 * 3
        assert s[st["row"] * 5, st["col"] * 4] == 255 and s[59, st["paddle"] * 4] == 128


def test_state_round_trip_and_refusals():
    env, o = _env(84, 84, 99), CatchOracle(84, 84, 99)
    for t in range(57):
        env.act(t % 3); o.act(t % 3)
    saved = env.get_state()
    tail = [(env.act(t % 3), env.get_state()) for t in range(200)]
    env.set_state(saved)
    assert env.get_state() == saved == o.state()
    assert np.array_equal(env.getScreen(), o.screen())
    assert [(env.act(t % 3), env.get_state()) for t in range(200)] == tail
    for bad in (dict(row=12), dict(col=-1), dict(paddle=10), dict(dx=2), dict(terminal=3)):
        with pytest.raises(AssertionError):
            env.set_state(dict(saved, **bad))
    for H, W in ((11, 84), (84, 11)):
        with pytest.raises(AssertionError):
            _env(H, W, 0)
    lib, h = sd.load(), C.c_void_p()
    assert lib.sdqn_env_create(C.byref(h), b"pong", 84, 84, 0, 10) == -1
    assert lib.sdqn_env_create(C.byref(h), b"catch", 84, 84, 0, 0) == -1
    with pytest.raises(AssertionError):
        env.act(3)


def test_environment_does_not_touch_the_samplers_generators():
    import random
    w0 = C.c_uint64(); sd.load().sdqn_mt_words(C.byref(w0))
    random.seed(5); st = random.getstate()
    env = _env(84, 84, 1)
    for t in range(500):
        env.act(t % 3)
    env.restart()
    w1 = C.c_uint64(); sd.load().sdqn_mt_words(C.byref(w1))
    assert random.getstate() == st and w0.value == w1.value


def test_tracking_policy_catches_every_ball():
    """every ball is reachable (11 paddle moves before it lands, at most 9 needed): a policy that goes to the landing column misses none"""
    o = CatchOracle(84, 84, 31)
    caught = 0
    while caught < 3000:
        target = min(max(o.landing_column() - 1, 0), 9)
        r = o.act(0 if o.paddle == target else (1 if o.paddle > target else 2))
        assert r >= 0
        caught += r
        if o.terminal:
            o.restart()


def test_random_policy_baseline():
    b = random_baseline()
    print("random-policy mean reward per ball over %d balls: %.4f" % (BASELINE_BALLS, b))
    assert -0.65 < b < -0.25              # a 3-of-12 paddle placed without skill: about 1 - 2 * 9/12 = -0.5, a little better by the walls
    assert random_baseline() == b


def test_argmax_rule():
    nan = float("nan")
    assert argmax_first([1.0, 3.0, 3.0]) == 1 and argmax_first([nan, 5.0, 1.0]) == 0 and argmax_first([1.0, nan, nan]) == 1
    for q in ([1.0, 3.0, 3.0], [nan, 5.0, 1.0], [1.0, nan, nan], [2.0, 2.0, 2.0]):
        assert argmax_first(q) == int(np.argmax(q))


def test_command_line():
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", "catch", "--eval_envs", "32"])
    assert (a.environment, a.eval_envs, a.catch_balls) == ("catch", 32, 10)
    d = build_parser().parse_args([])
    assert (d.environment, d.eval_envs, d.catch_balls, d.num_actions, d.test_steps) == ("synthetic", 0, 10, 4, 125000)
    assert "CatchEnvironment" in sd.__all__
    for name in ("sdqn_env_create", "sdqn_env_step", "sdqn_env_eval", "sdqn_net_act_step_env", "sdqn_env_render_device"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name)
    assert C.sizeof(_lib.EnvState) == 32 and _lib.EnvState.rng.offset == 24


def test_isa_census_of_the_environment_kernels():
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_env.hip")
    names = " ".join(r["name"] for r in rows)
    assert "catch_render_kernel" in names and "catch_eval_kernel" in names
    assert not [(r["name"], r["scratch"]) for r in rows if r["scratch"]]
    src = open(os.path.join(isa_census.CSRC, "sdqn_env.hip")).read() + open(os.path.join(isa_census.CSRC, "env_catch.h")).read()
    assert "atomic" not in src.lower()
