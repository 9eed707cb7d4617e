"""Pure-Python / numpy restatement of the game "freeway", of its renderer and of the draw order of vectorised evaluation and collection
on it, written from DESIGN.md §25 (not by calling the library): the yardstick of tests/test_freeway.py and tests/test_gpu_freeway.py.
The generator and the seeding of the copies are catch's (tests/catch_oracle.py), the lane ring is tests/collect_oracle.py's."""
import numpy as np

from collect_oracle import CollectOracle
from catch_oracle import SplitMix, argmax_first, explore_threshold, stream_seed

CELLS, ACTIONS, COLUMN = 12, 3, 6
LANES = tuple(range(1, 11))               # the traffic rows
START_ROW, MAX_PERIOD = 11, 5
TALLIES = ("steps", "reward", "caught", "missed", "episodes")
EVENTS = ("walked_into_car", "hit_by_car", "wrap_right", "wrap_left", "crossing", "shuffle", "terminal")


def pack(values):
    """ten values, row 1 first -> the 64-bit word with row r in nibble r - 1"""
    assert len(values) == len(LANES)
    return sum(int(v) << (4 * i) for i, v in enumerate(values))


def unpack(word):
    return [(word >> (4 * i)) & 15 for i in range(len(LANES))]


class FreewayOracle:
    def __init__(self, H=84, W=84, seed=0, episode_ticks=500):
        assert H >= CELLS and W >= CELLS and episode_ticks >= 1
        self.H, self.W, self.episode_ticks = H, W, episode_ticks
        self.rng = SplitMix(seed)
        self.events = dict((k, 0) for k in EVENTS)
        self.lost = False                    # whether the last step's chicken was hit
        self.restart()

    def _shuffle(self):
        d = self.rng.next()
        self.col, self.period = {}, {}
        for r in LANES:
            self.period[r] = 1 + d % MAX_PERIOD
            d //= MAX_PERIOD
            self.col[r] = d % CELLS
            d //= CELLS
        if self.col[10] == COLUMN:
            self.col[10] = COLUMN + 1
        self.timer = dict(self.period)
        self.events["shuffle"] += 1

    def restart(self):
        self.row, self.ticks, self.crossings, self.terminal = START_ROW, 0, 0, False
        self._shuffle()

    def _car_here(self):
        return self.row in LANES and self.col[self.row] == COLUMN

    def act(self, a):
        assert 0 <= a < ACTIONS
        ev = self.events
        self.lost = False
        reward = 0
        if a == 1:
            self.row = max(self.row - 1, 0)
        elif a == 2:
            self.row = min(self.row + 1, CELLS - 1)
        if self.row == 0:
            reward = 1
            self.crossings += 1
            self.row = START_ROW
            ev["crossing"] += 1
            self._shuffle()                                           # the traffic does not move in the tick of a crossing
        else:
            if self._car_here():
                self.row, self.lost = START_ROW, True
                ev["walked_into_car"] += 1
            for r in LANES:
                self.timer[r] -= 1
                if self.timer[r] == 0:
                    self.col[r] += 1 if r % 2 else -1
                    if self.col[r] > CELLS - 1:
                        self.col[r] = 0
                        ev["wrap_right"] += 1
                    if self.col[r] < 0:
                        self.col[r] = CELLS - 1
                        ev["wrap_left"] += 1
                    self.timer[r] = self.period[r]
            if not self.lost and self._car_here():
                self.row, self.lost = START_ROW, True
                ev["hit_by_car"] += 1
        self.ticks += 1
        if self.ticks >= self.episode_ticks and not self.terminal:
            self.terminal = True
            ev["terminal"] += 1
        return reward

    def state(self):
        return dict(row=self.row, ticks=self.ticks, crossings=self.crossings, terminal=int(self.terminal), pad0=0, pad1=0,
                    cars=pack([self.col[r] for r in LANES]), timers=pack([self.timer[r] for r in LANES]),
                    periods=pack([self.period[r] for r in LANES]), rng=self.rng.state)

    def set_state(self, st):
        self.row, self.ticks, self.crossings, self.terminal = st["row"], st["ticks"], st["crossings"], bool(st["terminal"])
        self.col, self.timer, self.period = (dict(zip(LANES, unpack(st[k]))) for k in ("cars", "timers", "periods"))
        self.rng = SplitMix(st["rng"])

    def screen(self):
        ch, cw = self.H // CELLS, self.W // CELLS
        s = np.zeros((self.H, self.W), dtype=np.uint8)
        for r in LANES:
            s[r * ch:(r + 1) * ch, self.col[r] * cw:(self.col[r] + 1) * cw] = 128
        s[self.row * ch:(self.row + 1) * ch, COLUMN * cw:(COLUMN + 1) * cw] = 255
        return s


class FreewayEvalOracle:
    """N copies of freeway as DeepQNetwork.evaluate plays them — tests/catch_oracle.py's EvalOracle with this game: copy e has a game
    generator stream_seed(seed, e, 0) and an acting generator stream_seed(seed, e, 1); a step draws u from the acting generator,
    explores when (u >> 11) < ceil(epsilon 2^53) with a second draw % 3, else takes the first maximum of its Q row; a terminal step
    restarts the copy with zeroed history.  Tallies: caught = crossings, missed = hits.  (The third constructor argument of the
    evaluation oracles, balls_per_episode, carries the episode's ticks here, as in the library.)"""

    def __init__(self, N, hist, H, W, epsilon, seed, episode_ticks=500):
        self.N, self.hist, self.eps_t = N, hist, explore_threshold(epsilon)
        self.envs = [FreewayOracle(H, W, stream_seed(seed, e, 0), episode_ticks) for e in range(N)]
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


class FreewayCollectOracle(CollectOracle):
    """Vectorised collection of freeway into a ring of N lanes of L slots: tests/collect_oracle.py's CollectOracle (DESIGN.md §19's
    rule, its lane sampler and gather) with the copies playing this game."""

    def __init__(self, N, size, hist, H, W, seed, episode_ticks=500):
        assert size % N == 0
        self.N, self.L, self.hist, self.size = N, size // N, hist, size
        self.games = FreewayEvalOracle(N, hist, H, W, 1.0, seed, episode_ticks)
        self.screens = np.zeros((size, H, W), np.uint8)
        self.actions = np.zeros(size, np.uint8)
        self.rewards = np.zeros(size, np.int64)
        self.terminals = np.zeros(size, bool)
        self.f = self.p = 0


# ---- the dynamics on this game: tests/dynamics_oracle.py's rule, whose wrappers take any game with act / restart /
# terminal / lost, applied to the classes above (its own tables name the two earlier games and stay as they are)
def single_game(H, W, seed, episode_ticks, frame_skip=1, repeat_action_probability=0.0):
    """the game of one environment handle created with `seed` under (k, p)"""
    from dynamics_oracle import STICKY_STREAM, DynamicsGame
    return DynamicsGame(FreewayOracle(H, W, seed, episode_ticks), frame_skip, repeat_action_probability, stream_seed(seed, 0, STICKY_STREAM))


def dynamics_eval_oracle(N, hist, H, W, epsilon, seed, episode_ticks, frame_skip=1, repeat_action_probability=0.0):
    from dynamics_oracle import _DynamicsEval
    o = type("DynamicsFreewayEvalOracle", (_DynamicsEval, FreewayEvalOracle), {})(N, hist, H, W, epsilon, seed, episode_ticks)
    o._wrap(seed, frame_skip, repeat_action_probability)
    return o


def dynamics_collect_oracle(N, size, hist, H, W, seed, episode_ticks, frame_skip=1, repeat_action_probability=0.0):
    o = FreewayCollectOracle(N, size, hist, H, W, seed, episode_ticks)
    o.games = dynamics_eval_oracle(N, hist, H, W, 1.0, seed, episode_ticks, frame_skip, repeat_action_probability)
    return o


def random_policy_score(episodes=200, seed=1, episode_ticks=500):
    """crossings per episode of the uniformly random policy (actions from a splitmix64 stream of its own), on the oracle alone"""
    o, pol = FreewayOracle(12, 12, seed, episode_ticks), SplitMix(seed ^ 0xF4EE)
    crossings = hits = 0
    for _ in range(episodes):
        while not o.terminal:
            o.act(pol.next() % ACTIONS)
            hits += o.lost
        crossings += o.crossings
        o.restart()
    return crossings / float(episodes), hits / float(episodes)


if __name__ == "__main__":
    for s in (1, 2, 3):
        print("seed %d: random policy, 200 episodes of 500 ticks: %.3f crossings and %.2f hits per episode" % ((s,) + random_policy_score(seed=s)))
