"""Prioritized experience replay restated in numpy (test helper, not product code).

  valid_mask      the indexes replay_memory.py:54-68 accepts, vectorised; accepts() is the rule index by index
  SumTree         leaves (float32) and 64-ary levels of fp64 sums, each node the butterfly fold of its 64 children
  sample          stratified draw t_n = (n + u_n) S / B, descent with a sequential fp64 prefix per level (np.cumsum)
  weights         (p_n / min_m p_m)^-beta
  PEROracle*      OracleDQN / OracleDQNBN (and their Double DQN forms) whose gradients() weight the clipped deltas of the taken
                  action, whose cost is mean(0.5 w delta^2), and which keep |delta| (last_abs_delta) for the new priorities
"""
import numpy as np

from double_dqn_oracle import _DoubleDQN
from oracle.dqn_bn_numpy import OracleDQNBN
from oracle.dqn_numpy import OracleDQN

FAN = 64


def accepts(i, terminals, count, current, hist):
    """replay_memory.py:59-66 for one index"""
    if i < hist or i > count - 1:
        return False
    if i >= current and i - hist < current:
        return False
    return not np.asarray(terminals[i - hist:i]).any()


def valid_mask(terminals, count, current, hist, size):
    t = np.zeros(size + 1, dtype=np.int64)
    t[1:] = np.cumsum(np.asarray(terminals[:size], dtype=bool))
    i = np.arange(size)
    lo = np.clip(i - hist, 0, size)
    ok = (i >= hist) & (i < count) & ~((i >= current) & (i - hist < current))
    ok &= (t[i] - t[lo]) == 0
    return ok


def fold(m):
    m = np.asarray(m, dtype=np.float64)
    while m.shape[-1] > 1:
        h = m.shape[-1] // 2
        m = m[..., :h] + m[..., h:]
    return m[..., 0]


def _pad(x, n):
    out = np.zeros(n, dtype=np.float64)
    out[:len(x)] = x
    return out


class SumTree:
    def __init__(self, leaf):
        self.levels = [np.asarray(leaf, dtype=np.float32)]
        x = self.levels[0].astype(np.float64)
        while len(x) > FAN:
            m = -(-len(x) // FAN)
            x = fold(_pad(x, m * FAN).reshape(m, FAN))
            self.levels.append(x)

    @property
    def total(self):
        return float(fold(_pad(self.levels[-1].astype(np.float64), FAN)))

    def descend(self, x):
        x = np.array(x, dtype=np.float64)
        n = len(x)
        top = len(self.levels) - 1
        base = np.zeros(n, dtype=np.int64)
        for L in range(top, -1, -1):
            lv = self.levels[L].astype(np.float64)
            cnt = len(lv) if L == top else FAN
            k = base[:, None] + np.arange(cnt)[None, :]
            c = np.where(k < len(lv), lv[np.minimum(k, len(lv) - 1)], 0.0)
            inc = np.cumsum(c, axis=1)                         # sequential: inc[k] = inc[k - 1] + c[k]
            exc = np.concatenate([np.zeros((n, 1)), inc[:, :-1]], axis=1)
            hit = (c > 0) & (x[:, None] < inc)
            first = np.where(hit.any(1), hit.argmax(1), -1)
            nz = c > 0
            last = cnt - 1 - nz[:, ::-1].argmax(1)
            j = np.where(first >= 0, first, last)
            x = x - exc[np.arange(n), j]
            chosen = base + j
            if L == 0:
                return chosen
            base = chosen * FAN


def uniforms(rng, B):
    """u_n = random.random() in batch order (2 MT words each)"""
    return np.array([rng.random() for _ in range(B)], dtype=np.float64)


def sample(leaf, u):
    tree = SumTree(leaf)
    B = len(u)
    S = tree.total
    t = np.array([(n + float(u[n])) * S / B for n in range(B)], dtype=np.float64)
    return tree.descend(t)


def weights(p, beta):
    p = np.asarray(p, dtype=np.float64)
    return (p / p.min()) ** (-beta)


def new_priority(abs_delta, alpha, eps):
    return np.float32((np.abs(np.asarray(abs_delta, dtype=np.float64)) + eps) ** alpha)


def write_back(raw, leaf, valid, idx, p):
    """last occurrence in batch order wins"""
    for i, v in zip(idx, p):
        raw[i] = v
        leaf[i] = v if valid[i] else 0.0


class _PER:
    weights = None              # [B] importance weights of the next gradients() call (None: all 1)
    last_abs_delta = None

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        t = np.array(super().td_targets(preq, maxpostq, actions, rewards, terminals), dtype=self.dtype)
        n, a = np.arange(len(actions)), np.asarray(actions, dtype=np.int64)
        d = (preq[n, a] - t[n, a]).astype(self.dtype)
        self.last_abs_delta = np.abs(d)
        dc = np.clip(d, -self._clip, self._clip).astype(self.dtype) if self._clip else d
        w = np.ones(len(d), self.dtype) if self.weights is None else np.asarray(self.weights, self.dtype)
        self._per_cost = self.dtype((w * (0.5 * (d * d))).mean())
        t[n, a] = preq[n, a] - (w * dc).astype(self.dtype)        # the parent's delta on the taken action becomes w * clip(delta)
        return t

    def gradients(self, minibatch):
        self._clip = self.clip_error
        self.clip_error = 0
        try:
            g, _, deltas, preq = super().gradients(minibatch)
        finally:
            self.clip_error = self._clip
        return g, self._per_cost, deltas, preq


class PEROracle(_PER, OracleDQN):
    pass


class PEROracleBN(_PER, OracleDQNBN):
    pass


class PEROracleDDQN(_PER, _DoubleDQN, OracleDQN):
    pass
