"""Pure-Python restatement of the games' dynamics — frame skip and sticky actions — written from DESIGN.md §23 (not by calling the
library), on top of the existing oracles, which it wraps by import and leaves as they are: the yardstick of tests/test_dynamics.py and
tests/test_gpu_dynamics.py.

The parameters: frame_skip k, an integer 1 <= k <= 8 (default 1); repeat_action_probability p, 0 <= p < 1 (default 0);
thresh_p = ceil(p 2^53).  Each copy of a game keeps `prev`, the action executed on its last tick (0 after init and after every
restart: action 0 is "stay" in both games), and a third splitmix64 generator, the sticky stream: stream_seed(seed, e, 2) for copy e
of a vectorised call, stream_seed(seed, 0, 2) for a single game created with `seed`.  One agent step with chosen action a:

    R = 0
    repeat up to k times:
        if thresh_p > 0:
            u = next(sticky)
            exec = prev if (u >> 11) < thresh_p else a
        else:
            exec = a                      # p = 0 draws NOTHING
        R += game.act(exec)
        prev = exec
        caught / missed tallies as without dynamics, per tick
        stop after a tick that sets terminal

The agent step's reward is R (|R| <= k); only the state after the last tick is rendered; ring, trace and statistics record the chosen
action a; `steps` counts agent steps; stickiness is drawn per tick.

  DynamicsGame                 a CatchOracle / BreakoutOracle under (k, p)
  single_game                  ... as sdqn_env_create(seed) + sdqn_env_set_dynamics seeds it
  dynamics_eval_oracle         EvalOracle / BreakoutEvalOracle whose copies play under (k, p)
  dynamics_collect_oracle      CollectOracle / BreakoutCollectOracle whose copies play under (k, p)
"""
import numpy as np

from breakout_oracle import BreakoutCollectOracle, BreakoutEvalOracle, BreakoutOracle
from catch_oracle import ACTIONS, CatchOracle, EvalOracle, SplitMix, argmax_first, explore_threshold, stream_seed
from collect_oracle import CollectOracle

MAX_SKIP, STICKY_STREAM = 8, 2
GAMES = {"catch": CatchOracle, "breakout": BreakoutOracle}
EVAL = {"catch": EvalOracle, "breakout": BreakoutEvalOracle}
COLLECT = {"catch": CollectOracle, "breakout": BreakoutCollectOracle}


class DynamicsGame:
    """`game` (a CatchOracle or BreakoutOracle, used through act / restart / terminal only) under frame skip k and sticky actions p.
    Everything else (screen, state, landing_column, ...) is the wrapped game's."""

    def __init__(self, game, frame_skip=1, repeat_action_probability=0.0, sticky_seed=0):
        assert 1 <= frame_skip <= MAX_SKIP and 0.0 <= repeat_action_probability < 1.0
        self.game, self.k, self.thresh_p = game, int(frame_skip), explore_threshold(repeat_action_probability)
        self.prev, self.sticky = 0, SplitMix(sticky_seed)
        self.ticks = self.stuck = 0          # game ticks played; ticks whose executed action was not the chosen one
        self.caught = self.missed = 0        # of the last agent step: ticks with a positive reward, ticks that lost a ball

    def __getattr__(self, name):
        return getattr(self.game, name)

    def act(self, a):
        assert 0 <= a < ACTIONS
        R = self.caught = self.missed = 0
        for _ in range(self.k):
            ex = a
            if self.thresh_p > 0:
                u = self.sticky.next()
                if (u >> 11) < self.thresh_p:
                    ex = self.prev
            r = self.game.act(ex)
            self.prev = ex
            R += r
            self.caught += r > 0
            self.missed += bool(self.game.lost) if hasattr(self.game, "lost") else r < 0      # breakout: a lost ball; catch: r < 0
            self.ticks += 1
            self.stuck += ex != a
            if self.game.terminal:
                break
        return R

    def restart(self):
        self.game.restart()
        self.prev = 0

    def dynamics(self):
        return dict(frame_skip=self.k, prev_action=self.prev, sticky_rng=self.sticky.state)


def single_game(name, H, W, seed, balls_per_episode, frame_skip=1, repeat_action_probability=0.0):
    """the game of one environment handle created with `seed`: game generator `seed`, sticky generator stream_seed(seed, 0, 2)"""
    return DynamicsGame(GAMES[name](H, W, seed, balls_per_episode), frame_skip, repeat_action_probability, stream_seed(seed, 0, STICKY_STREAM))


class _DynamicsEval:
    """the step of EvalOracle / BreakoutEvalOracle with DynamicsGame copies: the same draw order of the acting generator, the agent step
    of the text above in place of one tick, tallies per tick"""

    def _wrap(self, seed, frame_skip, p):
        self.envs = [DynamicsGame(g, frame_skip, p, stream_seed(seed, e, STICKY_STREAM)) for e, g in enumerate(self.envs)]
        self.explored = 0

    def step(self, q):
        acts, rews, terms = np.zeros(self.N, np.uint8), np.zeros(self.N, np.int8), np.zeros(self.N, bool)
        for e in range(self.N):
            u = self.act_rng[e].next()
            explore = (u >> 11) < self.eps_t
            a = self.act_rng[e].next() % ACTIONS if explore else argmax_first(q[e])
            self.explored += explore
            env = self.envs[e]
            r = env.act(a)
            acts[e], rews[e], terms[e] = a, r, env.terminal           # the CHOSEN action, the summed reward
            t = self.tally
            t["steps"][e] += 1; t["reward"][e] += r; t["caught"][e] += env.caught; t["missed"][e] += env.missed
            if env.terminal:
                t["episodes"][e] += 1
                env.restart()
                self.states[e] = 0
            else:
                self.states[e, :-1] = self.states[e, 1:]
            self.states[e, -1] = env.screen()                          # only the state after the last tick is rendered
        return acts, rews, terms


def dynamics_eval_oracle(name, N, hist, H, W, epsilon, seed, balls_per_episode, frame_skip=1, repeat_action_probability=0.0):
    base = EVAL[name]
    o = type("Dynamics" + base.__name__, (_DynamicsEval, base), {})(N, hist, H, W, epsilon, seed, balls_per_episode)
    o._wrap(seed, frame_skip, repeat_action_probability)
    return o


def dynamics_collect_oracle(name, N, size, hist, H, W, seed, balls_per_episode, frame_skip=1, repeat_action_probability=0.0):
    """CollectOracle / BreakoutCollectOracle (the laned ring, its sampler and gather) with the copies playing under (k, p)"""
    o = COLLECT[name](N, size, hist, H, W, seed, balls_per_episode)
    o.games = dynamics_eval_oracle(name, N, hist, H, W, 1.0, seed, balls_per_episode, frame_skip, repeat_action_probability)
    return o
