"""Bootstrapped DQN (--bootstrap_heads K) restated in numpy and Python integers (test helper, not product code).

The net has K A outputs; output row k A + a is Q-head k, action a.  For sample n taken from ring slot i_n:

    y_k      = r_c + (terminal ? 0 : gamma max_a Q_k(theta-, s')[a])          float64 from the network's own Q-values
    delta_k  = Q_k(theta, s)[a_n] - y_k  (y_k stored in the network's precision first), clipped by clip_error
    dq[n][k A + a_n] = m_k(i_n) clip(delta_k) / K, zero elsewhere
    cost term = (sum_k m_k 0.5 delta_k^2) / K;  cost = their mean;  maxq[n] = mean_k max_a Q_k(theta-, s')[a]
    (n_step > 1: R, done, gamma^n in the places of r_c, terminal, gamma)

    hash(s, a, b): s1 = s + G, o1 = mix(s1); s2 = (o1 ^ a) + G, o2 = mix(s2); s3 = (o2 ^ b) + G, result mix(s3)      (splitmix64, mod 2^64)
    m_k(i)   = 1 iff hash(mask_seed, i, k) >> 11 < ceil(ldexp(P, 53)); P = 1: all ones
    k(e, ep) = hash(head_seed, e, ep) mod K
    mask_seed / head_seed = mix(seed + D (2 * 0 + stream + 1)), stream 0 / 1
    vote: per-head first-maximum greedy action, the lowest action with the most votes
"""
import math

import numpy as np

from nstep_oracle import gamma_n, valid_mask
from oracle.dqn_numpy import CONV, OracleDQN, _col2im
from oracle.replay_numpy import ReplayOracle, synthetic_fill

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
STREAM = 0xD1B54A32D192ED03


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def bhash(seed, a, b):
    s = (seed + GOLDEN) & M64
    s = ((mix(s) ^ (a & M64)) + GOLDEN) & M64
    s = ((mix(s) ^ (b & M64)) + GOLDEN) & M64
    return mix(s)


def stream_seed(seed, stream):
    return mix((seed + STREAM * (stream + 1)) & M64)


def threshold(P):
    return int(math.ceil(math.ldexp(float(P), 53)))


def mask(seed, P, K, index):
    """m_k(index) for k < K as a uint8 array"""
    th = threshold(P)
    if th >= 1 << 53:
        return np.ones(K, np.uint8)
    ms = stream_seed(seed, 0)
    return np.array([1 if (bhash(ms, int(index), k) >> 11) < th else 0 for k in range(K)], np.uint8)


def head_of(seed, K, copy, episode):
    return 0 if K <= 1 else bhash(stream_seed(seed, 1), int(copy), int(episode)) % K


def vote(q_row, K, A):
    """(winning action, counts[A]) of the K per-head greedy actions; ties in the count go to the lowest action"""
    q = np.asarray(q_row).reshape(K, A)
    counts = np.zeros(A, np.int64)
    for k in range(K):
        counts[int(np.argmax(q[k]))] += 1                    # np.argmax: the first maximum, a NaN counts as one
    return int(np.argmax(counts)), counts


def head_slice(q_row, K, A, k):
    return np.asarray(q_row).reshape(K, A)[k]


class _Bootstrap:
    """OracleDQN over K A outputs with the targets and gradients above.  game_actions = A; indexes: the ring slots of the next
    gradients() call's samples (None: every mask is one, which needs mask_probability = 1)."""
    heads = 1
    game_actions = None
    mask_probability = 1.0
    mask_seed = 0
    indexes = None
    n_step = 1
    last_maxq = last_masks = last_cost_terms = last_d4 = None

    def masks(self, N):
        if self.indexes is None:
            assert threshold(self.mask_probability) >= 1 << 53, "masks need ring indexes"
            return np.ones((N, self.heads), np.uint8)
        assert len(self.indexes) == N
        return np.stack([mask(self.mask_seed, self.mask_probability, self.heads, i) for i in self.indexes])

    def gradients(self, minibatch):
        prestates, actions, rewards, poststates, terminals = minibatch
        N, K, A, t = prestates.shape[0], self.heads, self.game_actions, self.dtype
        assert K * A == self.num_actions
        postq = self.fprop(self.Wt, self._normalize(poststates))
        preq, (acts, cols_all, a3f, a4) = self.fprop(self.W, self._normalize(prestates), keep=True)
        if self.n_step > 1:
            r, gam = [float(x) for x in rewards], gamma_n(self.n_step, self.discount_rate)
        else:
            r, gam = [float(x) for x in np.clip(rewards, self.min_reward, self.max_reward)], self.discount_rate
        m = self.masks(N)
        targets = preq.copy()
        live = np.zeros(preq.shape, bool)
        maxq = np.zeros(N, np.float64)
        for n in range(N):
            for k in range(K):
                mk = float(postq[n, k * A:(k + 1) * A].max())
                maxq[n] += mk
                targets[n, k * A + int(actions[n])] = r[n] if terminals[n] else r[n] + gam * mk
                live[n, k * A + int(actions[n])] = bool(m[n, k])
            maxq[n] /= K
        deltas = preq - targets.astype(t)                                      # non-zero on the K taken-action rows
        terms = (0.5 * (np.where(live, deltas, t(0)) ** 2).sum(axis=1) / t(K)).astype(t)
        cost = t(terms.mean())
        if self.clip_error:
            deltas = np.clip(deltas, -self.clip_error, self.clip_error).astype(t)
        deltas = (np.where(live, deltas, t(0)) / t(K)).astype(t)
        self.last_maxq, self.last_masks, self.last_cost_terms = maxq, m, terms
        # ---- bprop: OracleDQN.gradients from here on
        g = [None] * 5
        g[4] = deltas.T @ a4
        d4 = self._hd((deltas @ self.W[4]) * (a4 > 0))
        self.last_d4 = d4
        g[3] = d4.T @ a3f
        d = self._hd((d4 @ self._h(self.W[3])) * (a3f > 0))
        for li in (2, 1, 0):
            R, S, Kc, st = CONV[li]
            a_out = acts[li + 1]
            d = d.reshape(a_out.shape)
            dmat = np.ascontiguousarray(d.reshape(N, Kc, -1).transpose(0, 2, 1))
            g[li] = np.einsum('nmc,nmk->ck', cols_all[li], dmat, optimize=True).astype(t)
            if li > 0:
                a_in = acts[li]
                dcols = dmat @ self._h(self.W[li]).T
                d = self._hd(_col2im(dcols, a_in.shape[1], a_in.shape[2], a_in.shape[3], R, S, st) * (a_in > 0))
        return g, cost, deltas, preq


class BootstrapOracle(_Bootstrap, OracleDQN):
    def __init__(self, game_actions, heads, *a, mask_probability=1.0, mask_seed=0, n_step=1, **kw):
        OracleDQN.__init__(self, heads * game_actions, *a, **kw)
        self.heads, self.game_actions = int(heads), int(game_actions)
        self.mask_probability, self.mask_seed, self.n_step = float(mask_probability), int(mask_seed), int(n_step)

    def predict_heads(self, states_u8):
        return self.predict(states_u8).reshape(-1, self.heads, self.game_actions)


def seed_with_empty_mask(P, K, indexes, first=0, tries=1000):
    """the first seed >= first under which some slot of `indexes` has an all-zero mask -> (seed, that slot)"""
    for seed in range(first, first + tries):
        for i in indexes:
            if not mask(seed, P, K, i).any():
                return seed, int(i)
    raise AssertionError("no seed with an all-zero mask among %d slots" % len(indexes))


# ---- the ring the GPU tests train from (tests/test_gpu_bootstrap.py) and the all-zero-mask case chosen on it ------------------------------
RING_SIZE = 300


def fill_ring(m, A, seed=3):
    """a full, wrapped ring of synthetic frames (product memory or ReplayOracle alike): terminals every ~20 slots, rewards outside the clip range too"""
    synthetic_fill(m, seed, num_actions=A)
    rng = np.random.RandomState(seed + 1)
    m.terminals[:] = rng.rand(m.size) < 0.05
    m.rewards[:] = rng.randint(-3, 4, m.size)


def valid_slots(om, n=1):
    return np.nonzero(valid_mask(om.terminals, om.count, om.current, om.history_length, om.size, n))[0]


def empty_mask_case(P=0.5, K=6, A=3):
    """(seed, slot): a valid slot of that ring whose K masks are all zero under seed"""
    om = ReplayOracle(RING_SIZE, 84, 84, 4, 32)
    fill_ring(om, A)
    return seed_with_empty_mask(P, K, [int(i) for i in valid_slots(om)])
