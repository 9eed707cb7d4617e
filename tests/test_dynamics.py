"""Frame skip and sticky actions without a device: the library's host functions against tests/dynamics_oracle.py bit for
bit, the defaults against the unwrapped oracles, terminals inside a skip, the sticky rate, state round trips, refusals, the C ABI and
the ISA census of the environment kernels."""
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
from catch_oracle import SplitMix, stream_seed  # noqa: E402
from dynamics_oracle import GAMES, single_game  # noqa: E402
from util import make_args  # noqa: E402

ENVS = {"catch": sd.CatchEnvironment, "breakout": sd.BreakoutEnvironment}
DYNAMICS = [(1, 0.0), (4, 0.0), (1, 0.25), (3, 0.25), (8, 0.9)]
STEPS = 2000


def _env(game, H, W, seed, balls, k=1, p=0.0):
    args = type("A", (), dict(screen_height=H, screen_width=W, frame_skip=k, repeat_action_probability=p))()
    return ENVS[game](args, seed=seed, balls_per_episode=balls)


def _same(env, o, where):
    d = env.get_dynamics()
    assert env.get_state() == o.state(), where
    assert (d["prev_action"], d["sticky_rng"]) == (o.prev, o.sticky.state), where
    assert np.array_equal(env.getScreen(), o.screen()), where


@pytest.mark.parametrize("k,p", DYNAMICS)
@pytest.mark.parametrize("H,W", [(12, 12), (84, 84)])
@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_host_step_equals_the_oracle(game, H, W, k, p):
    """2 000 agent steps of a fixed pseudo-random action sequence: reward, terminal, the whole state, prev, the sticky generator and
    the frame after every step; at (1, 0) also against the oracle without the wrapper, and the sticky generator never moves"""
    seed, balls = 4242 + k, 2
    env, o = _env(game, H, W, seed, balls, k, p), single_game(game, H, W, seed, balls, k, p)
    plain = GAMES[game](H, W, seed, balls) if (k, p) == (1, 0.0) else None
    d0 = env.get_dynamics()
    assert d0 == dict(frame_skip=k, repeat_action_probability=p, prev_action=0, sticky_rng=stream_seed(seed, 0, 2))
    assert (env.frame_skip, env.repeat_action_probability) == (k, p)
    _same(env, o, "start")
    actions = np.random.RandomState(7 * k + 1).randint(0, 3, STEPS)
    rewards, episodes = set(), 0
    for t in range(STEPS):
        a = int(actions[t])
        r, ro = env.act(a), o.act(a)
        assert (r, env.isTerminal()) == (ro, o.terminal), t
        assert abs(r) <= k
        _same(env, o, t)
        if plain is not None:
            assert plain.act(a) == r and plain.state() == env.get_state() and np.array_equal(plain.screen(), env.getScreen()), t
            assert env.get_dynamics()["sticky_rng"] == d0["sticky_rng"]
        rewards.add(r)
        if o.terminal:
            episodes += 1
            env.restart(); o.restart()
            if plain is not None:
                plain.restart()
            assert env.get_dynamics()["prev_action"] == 0
            _same(env, o, ("restart", t))
    assert episodes > 5 and len(rewards) > 1
    if p > 0:
        assert 0 < o.stuck < o.ticks and env.get_dynamics()["sticky_rng"] != d0["sticky_rng"]
    else:
        assert o.stuck == 0 and env.get_dynamics()["sticky_rng"] == d0["sticky_rng"]
    assert o.ticks <= k * STEPS and (k == 1) == (o.ticks == STEPS)     # k > 1: some agent step was cut short by a terminal


@pytest.mark.parametrize("game,k", [("breakout", 8), ("breakout", 3), ("catch", 8)])
def test_a_terminal_inside_a_skip_ends_the_agent_step(game, k):
    """one ball per episode: the tick that sets terminal is the agent step's last, R is the partial sum, prev is 0 after the restart"""
    env, o = _env(game, 84, 84, 11, 1, k, 0.0), single_game(game, 84, 84, 11, 1, k, 0.0)
    tick = GAMES[game](84, 84, 11, 1)                                # the same game advanced tick by tick
    cut = 0
    for t in range(600):
        a = (t * 5 + t // 7) % 3
        r = env.act(a)
        assert r == o.act(a) and env.isTerminal() == o.terminal
        partial, n = 0, 0
        while n < k:
            partial += tick.act(a); n += 1
            if tick.terminal:
                break
        assert r == partial and tick.state() == env.get_state(), t
        assert env.get_dynamics()["prev_action"] == a
        if o.terminal:
            cut += n < k
            env.restart(); o.restart(); tick.restart()
            assert env.get_dynamics()["prev_action"] == 0 and env.get_state() == tick.state()
    assert cut > 3                                                   # terminals did fall inside a skip


def test_sticky_rate():
    """20 000 ticks at p = 0.25, k = 1, the chosen action drawn anew (uniformly over the three) at every step from a stream of its
    own: a tick executes something else than the chosen action when it sticks (0.25) to a previous action that differs from it (2/3)"""
    seed, ticks = 2016, 20000
    lo, hi = 0.25 * (1 - 1 / 3.0) - 0.02, 0.25 * (1 - 1 / 3.0) + 0.02
    pol = SplitMix(seed ^ 0xABCDEF)
    actions = [pol.next() % 3 for _ in range(ticks)]
    o = single_game("catch", 84, 84, seed, 10, 1, 0.25)
    for a in actions:                                                # the oracle alone, first: the seed is inside the band
        o.act(a)
        if o.terminal:
            o.restart()
    share = o.stuck / float(o.ticks)
    print("oracle: %d of %d ticks executed another action than the chosen one: %.4f (band %.4f .. %.4f)" % (o.stuck, o.ticks, share, lo, hi))
    assert o.ticks == ticks and lo <= share <= hi
    env = _env("catch", 84, 84, seed, 10, 1, 0.25)
    stuck = 0
    for a in actions:
        env.act(a)
        stuck += env.get_dynamics()["prev_action"] != a              # k = 1: prev is what this tick executed
        if env.isTerminal():
            env.restart()
    assert stuck == o.stuck and lo <= stuck / float(ticks) <= hi


@pytest.mark.parametrize("game", ["catch", "breakout"])
def test_dynamics_state_round_trip(game):
    env = _env(game, 84, 84, 99, 3, 3, 0.25)
    for t in range(57):
        env.act(t % 3)
        if env.isTerminal():
            env.restart()
    st, dyn = env.get_state(), env.get_dynamics()
    assert dyn["sticky_rng"] != stream_seed(99, 0, 2)

    def tail(e):
        out = []
        for t in range(300):
            out.append((e.act((t * 7) % 3), e.isTerminal(), e.get_state(), e.get_dynamics()))
            if e.isTerminal():
                e.restart()
        return out
    ref = tail(env)
    other = _env(game, 84, 84, 5, 3, 3, 0.25)                        # another game, another seed: restored from the two records
    other.set_state(st)
    other.set_dynamics_state(dyn["prev_action"], dyn["sticky_rng"])
    assert other.get_state() == st and other.get_dynamics() == dyn
    assert tail(other) == ref
    before = env.get_dynamics()
    env.set_state(st)                                                # get_state / set_state keep their meaning: they leave the dynamics alone
    assert env.get_state() == st and env.get_dynamics() == before
    with pytest.raises(AssertionError) as ei:
        env.set_dynamics_state(3, 0)
    assert "prev_action" in str(ei.value)
    with pytest.raises(AssertionError):
        env.set_dynamics_state(-1, 0)


def test_refusals_name_their_argument():
    lib = sd.load()
    env = _env("catch", 84, 84, 1, 10)
    for k, p, word in ((0, 0.0, "frame_skip"), (9, 0.0, "frame_skip"), (1, -0.01, "repeat_action_probability"),
                       (1, 1.0, "repeat_action_probability"), (1, float("nan"), "repeat_action_probability")):
        assert lib.sdqn_env_set_dynamics(env._h, k, p) == -1
        assert word in lib.sdqn_last_error().decode(), (k, p)
        with pytest.raises(AssertionError):
            _env("breakout", 84, 84, 1, 3, k, p)
    assert env.get_dynamics() == dict(frame_skip=1, repeat_action_probability=0.0, prev_action=0, sticky_rng=stream_seed(1, 0, 2))
    k, p = C.c_int(), C.c_double()
    for rc in (lib.sdqn_env_set_dynamics(None, 2, 0.0), lib.sdqn_env_get_dynamics(None, C.byref(k), C.byref(p), None, None),
               lib.sdqn_env_set_dynamics_state(None, 0, 0)):
        assert rc == -1 and "NULL" in lib.sdqn_last_error().decode()
    _lib.check(lib.sdqn_env_set_dynamics(env._h, 8, 0.5))            # in range: served, and every output of get is optional
    _lib.check(lib.sdqn_env_get_dynamics(env._h, C.byref(k), C.byref(p), None, None))
    assert (k.value, p.value) == (8, 0.5)
    _lib.check(lib.sdqn_env_get_dynamics(env._h, None, None, None, None))


def test_command_line_and_check_dynamics():
    from simple_dqn_amd import main
    d = main.build_parser().parse_args([])
    assert (d.frame_skip, d.repeat_action_probability) == (1, 0.0) and main.check_dynamics(d) == (1, 0.0)
    a = main.build_parser().parse_args(["--environment", "breakout", "--frame_skip", "4", "--repeat_action_probability", "0.25"])
    assert main.check_dynamics(a) == (4, 0.25)
    assert main.check_dynamics(make_args(environment="synthetic")) == (1, 0.0)          # a namespace without the flags: the defaults
    base = ["--random_steps", "0", "--epochs", "0"]
    for extra, word in ((["--environment", "synthetic", "--frame_skip", "2"], "--frame_skip"),
                        (["--environment", "gym", "--repeat_action_probability", "0.25"], "--repeat_action_probability"),
                        (["--environment", "catch", "--frame_skip", "0"], "--frame_skip"),
                        (["--environment", "catch", "--frame_skip", "9"], "--frame_skip"),
                        (["--environment", "breakout", "--repeat_action_probability", "1.0"], "--repeat_action_probability"),
                        (["--environment", "breakout", "--repeat_action_probability", "-0.1"], "--repeat_action_probability")):
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:
            main.check_dynamics(args)
        assert word in str(ei.value), (extra, str(ei.value))
        # main.run refuses first: on a machine without a device anything later would be an SdqnError, never this ValueError
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert word in str(ei.value)


def test_symbols():
    for name in ("sdqn_env_set_dynamics", "sdqn_env_get_dynamics", "sdqn_env_set_dynamics_state"):
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name)
    assert C.sizeof(_lib.EnvState) == 32 and C.sizeof(_lib.EnvStateBreakout) == 48          # the state structs are what they were


# LDS bytes per kernel as the build of the parent commit (the tree before the dynamics) reports them through tools/isa_census.py, read
# from a build of that commit made with the same compiler when this test was written: the view hand-off of the lockstep kernels
# (VIEW_WORDS + 1 ints: 16 bytes for catch, 24 for breakout), nothing in the render kernels.
PARENT_LDS = {"catch_render_kernel": 0, "breakout_render_kernel": 0, "catch_eval_kernel": 16, "catch_collect_kernel": 16,
              "breakout_eval_kernel": 24, "breakout_collect_kernel": 24}


def test_isa_census_of_the_environment_kernels():
    """the six kernels of sdqn_env.hip: no scratch, the parent's LDS, fewer than 128 VGPRs (the count that would halve the residency
    of a 512-thread workgroup): the frame-skip loop is scalar work of one thread and stays a loop"""
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_env.hip")
    seen = {}
    for r in rows:
        for name in PARENT_LDS:
            if name in r["name"]:
                seen[name] = r
    assert sorted(seen) == sorted(PARENT_LDS), [r["name"] for r in rows]
    for name, r in sorted(seen.items()):
        print("%s: vgpr %d agpr %d lds %d scratch %d" % (name, r["vgpr"], r["agpr"], r["lds"], r["scratch"]))
        assert r["scratch"] == 0, name
        assert r["lds"] == PARENT_LDS[name], name
        assert r["vgpr"] + r["agpr"] < 128, name
