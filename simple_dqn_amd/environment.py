"""Environment interface of /root/reference/src/environment.py:7-33 plus a synthetic implementation.

The reference's ALE / gym wrappers (environment.py:35-144) are emulator I/O and out of scope
(SURVEY.md §2.1); SyntheticEnvironment offers the same six methods on seeded uint8 frames so the
Agent loop and the benchmarks run without an emulator.
"""
import ctypes as C

import numpy as np


class Environment:
    def numActions(self):
        raise NotImplementedError

    def restart(self):
        raise NotImplementedError

    def act(self, action):
        raise NotImplementedError

    def getScreen(self):
        raise NotImplementedError

    def isTerminal(self):
        raise NotImplementedError

    def setMode(self, mode):
        pass


class SyntheticEnvironment(Environment):
    """Seeded uint8 frames, rewards in {-1, 0, 1}, terminal with probability terminal_prob.  frame_pool > 0 (default 256): the frames are
    drawn from a pool of that many frames generated once (an emulator's screen buffer costs nothing to read either; generating 7 KB of
    random bytes per step was 10 us of the 38 us an acting step took and said nothing about the library); frame_pool = 0 generates a new
    frame every step (the behaviour of rounds 1-3)."""

    def __init__(self, args=None, num_actions=4, seed=0, terminal_prob=0.005, screen_height=84, screen_width=84, frame_pool=256):
        h = getattr(args, "screen_height", screen_height)
        w = getattr(args, "screen_width", screen_width)
        self.dims = (h, w)
        self._n = num_actions
        self._rng = np.random.RandomState(seed)
        self._tp = terminal_prob
        self._terminal = False
        self._screen = np.zeros(self.dims, dtype=np.uint8)
        self._pool = self._rng.randint(0, 256, size=(frame_pool,) + self.dims, dtype=np.uint8) if frame_pool else None
        self.mode = "train"

    def _frame(self):
        if self._pool is None:
            return self._rng.randint(0, 256, size=self.dims, dtype=np.uint8)
        return self._pool[self._rng.randint(len(self._pool))]

    def numActions(self):
        return self._n

    def restart(self):
        self._terminal = False
        self._screen = self._frame()

    def act(self, action):
        assert 0 <= action < self._n
        self._screen = self._frame()
        self._terminal = bool(self._rng.rand() < self._tp)
        return int(self._rng.randint(-1, 2))

    def getScreen(self):
        return self._screen

    def isTerminal(self):
        return self._terminal

    def setMode(self, mode):
        self.mode = mode


class LibraryEnvironment(Environment):
    """A game that lives in the library (include/sdqn.h sdqn_env_*): everything here runs on the host; `_h` lets
    DeepQNetwork.act_step_env / evaluate / collect step and render the game inside the library.  The generator is the environment's own
    (never Python's `random`).  A subclass names its game, its state struct and state calls, and its balls-per-episode option
    (freeway: its ticks-per-episode option).
    `args.frame_skip` (1..8, default 1) and `args.repeat_action_probability` (in [0, 1), default 0) are the game's dynamics
    (DESIGN.md §23): act(), DeepQNetwork.act_step_env and the copies of evaluate / collect all play under them."""
    game = None                                                      # name given to sdqn_env_create
    balls_option, balls_default = None, 10                           # the command line's balls-per-episode flag of this game
    _state_struct, _get_state, _set_state = None, None, None

    def __init__(self, args=None, seed=0, balls_per_episode=None, screen_height=84, screen_width=84, frame_skip=None,
                 repeat_action_probability=None):
        from . import _lib
        self._libmod, self._lib = _lib, _lib.load()
        h = getattr(args, "screen_height", screen_height)
        w = getattr(args, "screen_width", screen_width)
        if balls_per_episode is None:
            balls_per_episode = getattr(args, self.balls_option, self.balls_default)
        self.dims = (h, w)
        self.balls_per_episode = int(balls_per_episode)
        hd = C.c_void_p()
        _lib.check(self._lib.sdqn_env_create(C.byref(hd), self.game.encode(), h, w, int(seed) & 0xFFFFFFFFFFFFFFFF, self.balls_per_episode))
        self._h = hd
        if frame_skip is None:
            frame_skip = getattr(args, "frame_skip", 1)
        if repeat_action_probability is None:
            repeat_action_probability = getattr(args, "repeat_action_probability", 0.0)
        self.frame_skip, self.repeat_action_probability = int(frame_skip), float(repeat_action_probability)
        if (self.frame_skip, self.repeat_action_probability) != (1, 0.0):
            _lib.check(self._lib.sdqn_env_set_dynamics(hd, self.frame_skip, self.repeat_action_probability))
        self._screen = np.zeros(self.dims, dtype=np.uint8)
        self._screen_ok = False
        self._terminal = False
        self._r, self._t = C.c_int(), C.c_int()
        self.mode = "train"

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and self._lib is not None:
            self._lib.sdqn_env_destroy(h)

    def name(self):
        """the game's name as the library reports it"""
        n = C.c_char_p()
        self._libmod.check(self._lib.sdqn_env_name(self._h, C.byref(n)))
        return n.value.decode()

    def numActions(self):
        n = C.c_int()
        self._libmod.check(self._lib.sdqn_env_num_actions(self._h, C.byref(n)))
        return n.value

    def restart(self):
        self._libmod.check(self._lib.sdqn_env_restart(self._h))
        self._terminal, self._screen_ok = False, False

    def act(self, action):
        self._libmod.check(self._lib.sdqn_env_step(self._h, int(action), C.byref(self._r), C.byref(self._t)))
        self._terminal, self._screen_ok = bool(self._t.value), False
        return self._r.value

    def _stepped(self, terminal):
        """the library stepped the game itself (DeepQNetwork.act_step_env)"""
        self._terminal, self._screen_ok = bool(terminal), False

    def getScreen(self):
        if not self._screen_ok:
            self._screen = np.empty(self.dims, dtype=np.uint8)          # (a new array per frame, like an emulator's getScreen)
            self._libmod.check(self._lib.sdqn_env_screen(self._h, self._libmod.ptr(self._screen, C.c_uint8)))
            self._screen_ok = True
        return self._screen

    def isTerminal(self):
        return self._terminal

    def setMode(self, mode):
        self.mode = mode

    def get_state(self):
        st = getattr(self._libmod, self._state_struct)()
        self._libmod.check(getattr(self._lib, self._get_state)(self._h, C.byref(st)))
        return dict((k, getattr(st, k)) for k, _ in st._fields_)

    def set_state(self, state):
        st = getattr(self._libmod, self._state_struct)(**state)
        self._libmod.check(getattr(self._lib, self._set_state)(self._h, C.byref(st)))
        self._terminal, self._screen_ok = bool(st.terminal), False

    def get_dynamics(self):
        """frame_skip, repeat_action_probability and what get_state() leaves out of an exact copy of the game: the action the last
        tick executed and the sticky generator"""
        k, p, prev, rng = C.c_int(), C.c_double(), C.c_int(), C.c_uint64()
        self._libmod.check(self._lib.sdqn_env_get_dynamics(self._h, C.byref(k), C.byref(p), C.byref(prev), C.byref(rng)))
        return dict(frame_skip=k.value, repeat_action_probability=p.value, prev_action=prev.value, sticky_rng=rng.value)

    def set_dynamics_state(self, prev_action, sticky_rng):
        self._libmod.check(self._lib.sdqn_env_set_dynamics_state(self._h, int(prev_action), int(sticky_rng) & 0xFFFFFFFFFFFFFFFF))

    def render_device(self):
        """test hook: the current frame as the render kernel produces it"""
        out = np.empty(self.dims, dtype=np.uint8)
        self._libmod.check(self._lib.sdqn_env_render_device(self._h, self._libmod.ptr(out, C.c_uint8)))
        return out


class CatchEnvironment(LibraryEnvironment):
    """The game "catch" of the library (csrc/env_catch.h): a ball falls through a 12 x 12 court, a 3-cell paddle on the
    bottom row moves with actions 0 stay / 1 left / 2 right; +1 for a ball caught, -1 for a ball missed, an episode is
    `balls_per_episode` balls."""
    game = "catch"
    balls_option, balls_default = "catch_balls", 10
    _state_struct, _get_state, _set_state = "EnvState", "sdqn_env_get_state", "sdqn_env_set_state"


class BreakoutEnvironment(LibraryEnvironment):
    """The game "breakout" of the library (csrc/env_breakout.h): the court, paddle and actions of catch, three rows of
    bricks that stay destroyed, a ball that moves diagonally and turns back from walls, bricks and the paddle; +1 for a brick broken
    and nothing else, an episode is `balls_per_episode` lost balls."""
    game = "breakout"
    balls_option, balls_default = "breakout_balls", 3
    _state_struct, _get_state, _set_state = "EnvStateBreakout", "sdqn_env_get_state_breakout", "sdqn_env_set_state_breakout"


class FreewayEnvironment(LibraryEnvironment):
    """The game "freeway" of the library (csrc/env_freeway.h): a chicken on column 6 of the same court walks from row 11
    to row 0 with actions 0 stay / 1 up / 2 down through ten rows of traffic, one car per row, each with its own period and direction;
    +1 for a crossing and nothing else, a hit sends the chicken back to row 11, an episode is `balls_per_episode` game ticks
    (`--freeway_ticks`, 500: the library's balls-per-episode argument carries the episode length for this game)."""
    game = "freeway"
    balls_option, balls_default = "freeway_ticks", 500
    _state_struct, _get_state, _set_state = "EnvStateFreeway", "sdqn_env_get_state_freeway", "sdqn_env_set_state_freeway"


LIBRARY_GAMES = {"catch": CatchEnvironment, "breakout": BreakoutEnvironment, "freeway": FreewayEnvironment}     # --environment values that live in the library


def _to_gray_resized(obs, height, width):
    """cv2.resize(cv2.cvtColor(obs, COLOR_RGB2GRAY), (w, h)) of environment.py:139 without cv2: ITU-R 601 luma,
    then bilinear interpolation with half-pixel centres (cv2.INTER_LINEAR's sampling grid)."""
    obs = np.asarray(obs)
    if obs.ndim == 3:
        g = obs[..., 0] * 0.299 + obs[..., 1] * 0.587 + obs[..., 2] * 0.114
    else:
        g = obs.astype(np.float64)
    H, W = g.shape
    if (H, W) == (height, width):
        return np.clip(np.rint(g), 0, 255).astype(np.uint8)
    ys = (np.arange(height) + 0.5) * H / height - 0.5
    xs = (np.arange(width) + 0.5) * W / width - 0.5
    y0 = np.clip(np.floor(ys).astype(int), 0, H - 1); y1 = np.clip(y0 + 1, 0, H - 1); fy = np.clip(ys - np.floor(ys), 0, 1)
    x0 = np.clip(np.floor(xs).astype(int), 0, W - 1); x1 = np.clip(x0 + 1, 0, W - 1); fx = np.clip(xs - np.floor(xs), 0, 1)
    fy = np.where(ys < 0, 0.0, fy)[:, None]; fx = np.where(xs < 0, 0.0, fx)[None, :]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x1] * fx
    bot = g[y1][:, x0] * (1 - fx) + g[y1][:, x1] * fx
    return np.clip(np.rint(top * (1 - fy) + bot * fy), 0, 255).astype(np.uint8)


class GymEnvironment(Environment):
    """py3 restatement of /root/reference/src/environment.py:112-144 for `gymnasium` (or classic `gym`) when one of
    them is installed — neither is in this image, so this adapter is exercised against a stand-in module only
    (tests/test_environment.py).  Emulator I/O is outside the hot path (optional part)."""

    def __init__(self, env_id, args, make=None):
        if make is None:
            try:
                import gymnasium as gym
            except ImportError:
                import gym
            make = gym.make
        self.gym = make(env_id)
        self.obs = None
        self.terminal = None
        self.screen_width = args.screen_width
        self.screen_height = args.screen_height
        self.mode = "train"

    def numActions(self):
        n = getattr(self.gym.action_space, "n", None)
        assert n is not None, "a Discrete action space is required"          # environment.py:127
        return int(n)

    def restart(self):
        r = self.gym.reset()
        self.obs = r[0] if isinstance(r, tuple) else r                         # gymnasium returns (obs, info)
        self.terminal = False

    def act(self, action):
        r = self.gym.step(action)
        if len(r) == 5:                                                       # gymnasium: terminated, truncated
            self.obs, reward, terminated, truncated, _ = r
            self.terminal = bool(terminated or truncated)
        else:                                                                 # classic gym, environment.py:135
            self.obs, reward, self.terminal, _ = r
            self.terminal = bool(self.terminal)
        return reward

    def getScreen(self):
        assert self.obs is not None
        return _to_gray_resized(self.obs, self.screen_height, self.screen_width)

    def isTerminal(self):
        assert self.terminal is not None
        return self.terminal

    def setMode(self, mode):
        self.mode = mode
