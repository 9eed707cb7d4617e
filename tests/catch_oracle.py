"""Pure-Python / numpy restatement of the game "catch" and of the vectorised evaluation's seeding and draw order, written from
DESIGN.md §18 (not by calling the library): the yardstick of tests/test_catch.py and tests/test_gpu_catch.py."""
import math

import numpy as np

M64 = (1 << 64) - 1
CELLS, PADDLE, ACTIONS = 12, 3, 3
GOLDEN, STREAM_K = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


def mix(z):
    """splitmix64's finaliser"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class SplitMix:
    def __init__(self, state):
        self.state = state & M64

    def next(self):
        self.state = (self.state + GOLDEN) & M64
        return mix(self.state)


def stream_seed(seed, e, stream):
    """state of generator `stream` (0 game, 1 acting policy) of copy e of an evaluation seeded with `seed`"""
    return mix((seed + STREAM_K * (2 * e + stream + 1)) & M64)


def explore_threshold(epsilon):
    return math.ceil(epsilon * 2.0 ** 53)


class CatchOracle:
    def __init__(self, H=84, W=84, seed=0, balls_per_episode=10):
        assert H >= CELLS and W >= CELLS
        self.H, self.W, self.bpe = H, W, balls_per_episode
        self.rng = SplitMix(seed)
        self.restart()

    def _spawn(self):
        d = self.rng.next()
        self.row, self.col, self.dx = 0, d % CELLS, (d // CELLS) % 3 - 1

    def restart(self):
        self.balls, self.terminal, self.paddle = 0, False, 4
        self._spawn()

    def act(self, a):
        assert 0 <= a < ACTIONS
        if a == 1:
            self.paddle = max(self.paddle - 1, 0)
        elif a == 2:
            self.paddle = min(self.paddle + 1, CELLS - PADDLE)
        self.row += 1
        self.col += self.dx
        if self.col < 0:
            self.col, self.dx = -self.col, -self.dx
        if self.col > CELLS - 1:
            self.col, self.dx = 2 * (CELLS - 1) - self.col, -self.dx
        if self.row < CELLS - 1:
            return 0
        reward = 1 if self.paddle <= self.col <= self.paddle + PADDLE - 1 else -1
        self.balls += 1
        if self.balls >= self.bpe:
            self.terminal = True
        self._spawn()
        return reward

    def state(self):
        return dict(row=self.row, col=self.col, dx=self.dx, paddle=self.paddle, balls=self.balls, terminal=int(self.terminal),
                    rng=self.rng.state)

    def screen(self):
        ch, cw = self.H // CELLS, self.W // CELLS
        s = np.zeros((self.H, self.W), dtype=np.uint8)
        s[(CELLS - 1) * ch:CELLS * ch, self.paddle * cw:(self.paddle + PADDLE) * cw] = 128
        s[self.row * ch:(self.row + 1) * ch, self.col * cw:(self.col + 1) * cw] = 255
        return s

    def landing_column(self):
        """column in which the falling ball will reach row 11"""
        col, dx = self.col, self.dx
        for _ in range(CELLS - 1 - self.row):
            col += dx
            if col < 0:
                col, dx = -col, -dx
            if col > CELLS - 1:
                col, dx = 2 * (CELLS - 1) - col, -dx
        return col


def argmax_first(q):
    """np.argmax's rule: the first maximum, a NaN counts as one"""
    best = 0
    for k in range(1, len(q)):
        if q[k] > q[best] or (q[k] != q[k] and q[best] == q[best]):
            best = k
    return best


class EvalOracle:
    """N copies of the game as DeepQNetwork.evaluate plays them: copy e has a game generator stream_seed(seed, e, 0) and an acting
    generator stream_seed(seed, e, 1); a step draws u from the acting generator, explores when (u >> 11) < ceil(epsilon 2^53) with a
    second draw % 3, else takes the first maximum of its Q row; a terminal step restarts the copy with zeroed history."""

    def __init__(self, N, hist, H, W, epsilon, seed, balls_per_episode=10):
        self.N, self.hist, self.eps_t = N, hist, explore_threshold(epsilon)
        self.envs = [CatchOracle(H, W, stream_seed(seed, e, 0), balls_per_episode) for e in range(N)]
        self.act_rng = [SplitMix(stream_seed(seed, e, 1)) for e in range(N)]
        self.states = np.zeros((N, hist, H, W), dtype=np.uint8)
        for e in range(N):
            self.states[e, -1] = self.envs[e].screen()
        self.tally = dict((k, np.zeros(N, dtype=np.int64)) for k in ("steps", "reward", "caught", "missed", "episodes"))

    def step(self, q):
        """q [N, A]: the Q rows the policy sees; returns (actions, rewards, terminals) and advances the states"""
        acts, rews, terms = np.zeros(self.N, np.uint8), np.zeros(self.N, np.int8), np.zeros(self.N, bool)
        for e in range(self.N):
            u = self.act_rng[e].next()
            a = self.act_rng[e].next() % ACTIONS if (u >> 11) < self.eps_t else argmax_first(q[e])
            env = self.envs[e]
            r = env.act(a)
            acts[e], rews[e], terms[e] = a, r, env.terminal
            t = self.tally
            t["steps"][e] += 1; t["reward"][e] += r; t["caught"][e] += r > 0; t["missed"][e] += r < 0
            if env.terminal:
                t["episodes"][e] += 1
                env.restart()
                self.states[e] = 0
            else:
                self.states[e, :-1] = self.states[e, 1:]
            self.states[e, -1] = env.screen()
        return acts, rews, terms
