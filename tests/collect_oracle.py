"""Pure-Python / numpy restatement of vectorised collection into a laned replay ring (--train_envs), written from the
design text on top of tests/catch_oracle.py (not by calling the library): the yardstick of tests/test_collect.py and
tests/test_gpu_collect.py.

  CollectOracle          N copies of catch played in lockstep as EvalOracle plays them; lockstep number k writes copy e's transition
                         (action, reward, terminal, the frame after the step — the restarted game's first frame at a terminal) into
                         slot e L + p of a ring of N lanes of L slots, then p = (p + 1) % L and f = min(f + 1, L)
  sample_indexes_lanes   the lane sampler on oracle.replay_numpy.MT19937: r = randint(0, N span - 1), span = f - n - hist + 1, lane
                         r // span, local l = hist + r % span, index lane L + l; rejected when l + n - 1 >= p and l - hist < p, or when
                         terminals[index - hist : index] holds a terminal; returns (indexes, draws)
  valid_indexes          every index that rule accepts
  gather                 (prestates, actions, rewards | returns, poststates, terminals | dones) of indexes: plain slices of the ring
"""
import numpy as np

import nstep_oracle
from catch_oracle import EvalOracle, explore_threshold


def accepts(l, lane, terminals, L, p, hist, n):
    if l + n - 1 >= p and l - hist < p:
        return False
    i = lane * L + l
    return not np.asarray(terminals[i - hist:i]).any()


def valid_indexes(terminals, N, L, f, p, hist, n):
    span = f - n - hist + 1
    return [e * L + l for e in range(N) for l in range(hist, hist + max(span, 0)) if accepts(l, e, terminals, L, p, hist, n)]


def sample_indexes_lanes(rng, terminals, N, L, f, p, hist, n, batch):
    span = f - n - hist + 1
    assert span > 0
    out, draws = [], 0
    while len(out) < batch:
        r = rng.randint(0, N * span - 1)
        draws += 1
        lane, l = r // span, hist + r % span
        if accepts(l, lane, terminals, L, p, hist, n):
            out.append(lane * L + l)
    return np.array(out, dtype=np.int64), draws


class CollectOracle:
    def __init__(self, N, size, hist, H, W, seed, balls_per_episode=10):
        assert size % N == 0
        self.N, self.L, self.hist, self.size = N, size // N, hist, size
        self.games = EvalOracle(N, hist, H, W, 1.0, seed, balls_per_episode)
        self.screens = np.zeros((size, H, W), np.uint8)
        self.actions = np.zeros(size, np.uint8)
        self.rewards = np.zeros(size, np.int64)
        self.terminals = np.zeros(size, bool)
        self.f = self.p = 0

    @property
    def tally(self):
        return self.games.tally

    def lockstep(self, epsilon, q=None):
        """one lockstep with exploration rate epsilon on the Q rows q [N, 3] (None: zeros, what a skipped forward leaves)"""
        g = self.games
        g.eps_t = explore_threshold(epsilon)
        a, r, t = g.step(np.zeros((self.N, 3)) if q is None else q)
        for e in range(self.N):
            s = e * self.L + self.p
            self.screens[s], self.actions[s], self.rewards[s], self.terminals[s] = g.states[e, -1], a[e], r[e], t[e]
        self.p = (self.p + 1) % self.L
        self.f = min(self.f + 1, self.L)
        return a, r, t

    def sample(self, rng, n, batch):
        return sample_indexes_lanes(rng, self.terminals, self.N, self.L, self.f, self.p, self.hist, n, batch)

    def gather(self, indexes, n=1, gamma=0.99, min_reward=-1.0, max_reward=1.0):
        h = self.hist
        for i in indexes:                                            # a sampled window is contiguous slots of ONE lane
            assert (i - h) // self.L == (i + n - 1) // self.L and i % self.L >= h
        pre = np.stack([self.screens[i - h:i] for i in indexes])
        post = np.stack([self.screens[i + n - h:i + n] for i in indexes])
        idx = np.asarray(indexes, dtype=np.int64)
        if n == 1:
            return pre, self.actions[idx], self.rewards[idx], post, self.terminals[idx]
        R, done = nstep_oracle.returns(self.rewards, self.terminals, idx, n, gamma, min_reward, max_reward)
        return pre, self.actions[idx], np.asarray(R, np.float64), post, np.asarray(done, bool)
