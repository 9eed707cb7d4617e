"""Pure-Python / numpy restatement of the game "breakout", of its renderer and of the draw order of vectorised evaluation and
collection on it, written from DESIGN.md §20 (not by calling the library): the yardstick of tests/test_breakout.py and
tests/test_gpu_breakout.py.  The generator and the seeding of the copies are catch's (tests/catch_oracle.py)."""
import numpy as np

from collect_oracle import CollectOracle
from catch_oracle import SplitMix, argmax_first, explore_threshold, stream_seed

CELLS, PADDLE, ACTIONS = 12, 3, 3
BRICK_ROWS, SPAWN_ROW = (1, 2, 3), 4
WALL = (1 << 36) - 1
TALLIES = ("steps", "reward", "caught", "missed", "episodes")


def brick_bit(r, c):
    return 1 << (12 * (r - 1) + c)


class BreakoutOracle:
    def __init__(self, H=84, W=84, seed=0, balls_per_episode=3):
        assert H >= CELLS and W >= CELLS
        self.H, self.W, self.bpe = H, W, balls_per_episode
        self.rng = SplitMix(seed)
        self.events = dict((k, 0) for k in ("brick", "boxed", "refill", "paddle_left", "paddle_middle", "paddle_right", "side_wall", "top_wall",
                                            "lost", "terminal"))
        self.lost = False                    # whether the last step lost a ball
        self.restart()

    def _spawn(self):
        d = self.rng.next()
        self.row, self.col, self.dx, self.dy = SPAWN_ROW, d % CELLS, (1 if (d // CELLS) & 1 else -1), 1

    def restart(self):
        self.balls, self.terminal, self.paddle, self.bricks = 0, False, 4, WALL
        self._spawn()

    def act(self, a):
        assert 0 <= a < ACTIONS
        ev = self.events
        self.lost = False
        if a == 1:
            self.paddle = max(self.paddle - 1, 0)
        elif a == 2:
            self.paddle = min(self.paddle + 1, CELLS - PADDLE)
        nc = self.col + self.dx
        if nc < 0 or nc > CELLS - 1:
            nc = -nc if nc < 0 else 2 * (CELLS - 1) - nc
            self.dx = -self.dx
            ev["side_wall"] += 1
        nr = self.row + self.dy
        if nr < 0:
            self.dy, nr = 1, self.row + 1
            ev["top_wall"] += 1
        if nr in BRICK_ROWS and self.bricks & brick_bit(nr, nc):
            self.bricks &= ~brick_bit(nr, nc)
            self.dy = -self.dy                                        # the ball keeps its row this step
            if self.row in BRICK_ROWS and self.bricks & brick_bit(self.row, nc):
                self.dx = -self.dx                                    # the cell beside it is a brick too: it keeps its column as well
                ev["boxed"] += 1
            else:
                self.col = nc
            ev["brick"] += 1
            if self.bricks == 0:
                self.bricks = WALL
                ev["refill"] += 1
                if self.row in BRICK_ROWS:                            # it would stand inside the new wall: it leaves it downwards
                    self.row, self.dy = SPAWN_ROW, 1
            return 1
        if nr == CELLS - 1:
            k = nc - self.paddle
            if 0 <= k < PADDLE:
                self.dy, self.row, self.col = -1, CELLS - 2, nc
                if k == 0:
                    self.dx = -1
                elif k == PADDLE - 1:
                    self.dx = 1
                ev[("paddle_left", "paddle_middle", "paddle_right")[k]] += 1
                return 0
            self.lost = True
            self.balls += 1
            ev["lost"] += 1
            if self.balls >= self.bpe:
                self.terminal = True
                ev["terminal"] += 1
            self._spawn()
            return 0
        self.row, self.col = nr, nc
        return 0

    def state(self):
        return dict(row=self.row, col=self.col, dx=self.dx, dy=self.dy, paddle=self.paddle, balls=self.balls, terminal=int(self.terminal),
                    pad=0, bricks=self.bricks, rng=self.rng.state)

    def set_state(self, st):
        self.row, self.col, self.dx, self.dy, self.paddle, self.balls = (st[k] for k in ("row", "col", "dx", "dy", "paddle", "balls"))
        self.terminal, self.bricks, self.rng = bool(st["terminal"]), st["bricks"], SplitMix(st["rng"])

    def screen(self):
        ch, cw = self.H // CELLS, self.W // CELLS
        s = np.zeros((self.H, self.W), dtype=np.uint8)
        for r in BRICK_ROWS:
            for c in range(CELLS):
                if self.bricks & brick_bit(r, c):
                    s[r * ch:(r + 1) * ch, c * cw:(c + 1) * cw] = 64
        s[(CELLS - 1) * ch:CELLS * ch, self.paddle * cw:(self.paddle + PADDLE) * cw] = 128
        s[self.row * ch:(self.row + 1) * ch, self.col * cw:(self.col + 1) * cw] = 255
        return s


class BreakoutEvalOracle:
    """N copies of breakout as DeepQNetwork.evaluate plays them — tests/catch_oracle.py's EvalOracle with this game: copy e has a game
    generator stream_seed(seed, e, 0) and an acting generator stream_seed(seed, e, 1); a step draws u from the acting generator,
    explores when (u >> 11) < ceil(epsilon 2^53) with a second draw % 3, else takes the first maximum of its Q row; a terminal step
    restarts the copy with zeroed history.  Tallies: caught = bricks broken, missed = balls lost."""

    def __init__(self, N, hist, H, W, epsilon, seed, balls_per_episode=3):
        self.N, self.hist, self.eps_t = N, hist, explore_threshold(epsilon)
        self.envs = [BreakoutOracle(H, W, stream_seed(seed, e, 0), balls_per_episode) for e in range(N)]
        self.act_rng = [SplitMix(stream_seed(seed, e, 1)) for e in range(N)]
        self.states = np.zeros((N, hist, H, W), dtype=np.uint8)
        for e in range(N):
            self.states[e, -1] = self.envs[e].screen()
        self.tally = dict((k, np.zeros(N, dtype=np.int64)) for k in TALLIES)
        self.explored = 0                    # steps whose action came from the second draw

    def step(self, q):
        """q [N, A]: the Q rows the policy sees; returns (actions, rewards, terminals) and advances the states"""
        acts, rews, terms = np.zeros(self.N, np.uint8), np.zeros(self.N, np.int8), np.zeros(self.N, bool)
        for e in range(self.N):
            u = self.act_rng[e].next()
            explore = (u >> 11) < self.eps_t
            a = self.act_rng[e].next() % ACTIONS if explore else argmax_first(q[e])
            self.explored += explore
            env = self.envs[e]
            r = env.act(a)
            acts[e], rews[e], terms[e] = a, r, env.terminal
            t = self.tally
            t["steps"][e] += 1; t["reward"][e] += r; t["caught"][e] += r > 0; t["missed"][e] += env.lost
            if env.terminal:
                t["episodes"][e] += 1
                env.restart()
                self.states[e] = 0
            else:
                self.states[e, :-1] = self.states[e, 1:]
            self.states[e, -1] = env.screen()
        return acts, rews, terms


class BreakoutCollectOracle(CollectOracle):
    """Vectorised collection of breakout into a ring of N lanes of L slots: tests/collect_oracle.py's CollectOracle (DESIGN.md §19's
    rule — lockstep number k writes copy e's transition (action, reward, terminal, the frame after the step, the restarted game's
    first frame at a terminal) into slot e L + p, then p = (p + 1) % L and f = min(f + 1, L) — and its lane sampler and gather) with
    the copies playing this game."""

    def __init__(self, N, size, hist, H, W, seed, balls_per_episode=3):
        assert size % N == 0
        self.N, self.L, self.hist, self.size = N, size // N, hist, size
        self.games = BreakoutEvalOracle(N, hist, H, W, 1.0, seed, balls_per_episode)
        self.screens = np.zeros((size, H, W), np.uint8)
        self.actions = np.zeros(size, np.uint8)
        self.rewards = np.zeros(size, np.int64)
        self.terminals = np.zeros(size, bool)
        self.f = self.p = 0
