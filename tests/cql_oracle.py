"""Conservative Q-learning restated in numpy (test helper, not product code).

CQL(H) in its discrete form (Kumar, Zhou, Tucker and Levine 2020) adds alpha (logsumexp_k Q(theta, s)[k] - Q(theta, s)[a]) to the loss of
deepqnetwork.py's train step and changes nothing else.  With q = Q(theta, s_n) as stored, a = a_n, y the standard target (n-step: R,
done, gamma^n in their places) and w = 1 or the importance weight of a prioritized memory:

    m      = max_k q[k]                       lse = m + log(sum_k exp(q[k] - m))       (float64 from the stored values)
    pi[k]  = exp(q[k] - lse)
    delta  = q[a] - T(y)                      dc = clip(delta)                          (clip first, then weight)
    dq[k]  = w T(alpha (pi[k] - 1[k == a]))  +  1[k == a] w dc
    cost_terms[n] = w 0.5 delta^2  +  w T(alpha (lse - q[a]))
    priority = (|delta| + eps)^alpha_per of the unclipped delta

T is the network's number type: the softmax is computed in float64 and rounded once.  `cql_alpha = 0` is the parent's step.
"""
import math

import numpy as np

from nstep_oracle import _NStep
from oracle.dqn_numpy import OracleDQN


def lse(row):
    """m + log(sum_k exp(q[k] - m)) of one row in Python floats (= float64), the sum in action order"""
    m = max(float(x) for x in row)
    s = 0.0
    for x in row:
        s += math.exp(float(x) - m)
    return m + math.log(s)


def cql_sample(q_row, action, y, alpha, clip_error=0.0, weight=1.0, dtype=np.float32):
    """(dq row, cost term, delta) of one sample, every operation in `dtype` but the softmax (float64, rounded once)"""
    T = np.dtype(dtype).type
    q = np.asarray(q_row, dtype=T)
    A, a, w = len(q), int(action), T(weight)
    L = lse(q)
    d = T(q[a] - T(y))
    dc = T(min(max(d, T(-clip_error)), T(clip_error))) if clip_error else d
    dq = np.zeros(A, dtype=T)
    for k in range(A):
        t = T(w * T(float(alpha) * (math.exp(float(q[k]) - L) - (1.0 if k == a else 0.0))))
        dq[k] = T(t + T(w * dc)) if k == a else t
    cost = T(T(w * T(T(0.5) * T(d * d))) + T(w * T(float(alpha) * (L - float(q[a])))))
    return dq, cost, d


def cql_batch(q, actions, targets_taken, alpha, clip_error, weights, dtype):
    rows = [cql_sample(q[i], actions[i], targets_taken[i], alpha, clip_error, 1.0 if weights is None else weights[i], dtype)
            for i in range(len(actions))]
    return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=dtype), np.array([r[2] for r in rows], dtype=dtype))


class _CQL:
    cql_alpha = 1.0
    weights = None              # [B] importance weights of the next gradients() call (None: all 1)
    last_abs_delta = None       # |delta| of the taken actions, unclipped: what the new priorities are made of
    last_dq = None              # [B][A] the head's dq rows
    last_cost_terms = None      # [B]
    last_y = None               # [B] the targets of the taken actions as stored in the network's precision
    last_lse = None             # [B] float64

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        t = np.array(super().td_targets(preq, maxpostq, actions, rewards, terminals), dtype=self.dtype)
        n, a = np.arange(len(actions)), np.asarray(actions, dtype=np.int64)
        y = t[n, a]
        dq, cost, d = cql_batch(preq, a, y, self.cql_alpha, self._clip, self.weights, self.dtype)
        self.last_y, self.last_dq, self.last_cost_terms, self.last_abs_delta = y, dq, cost, np.abs(d)
        self.last_lse = np.array([lse(row) for row in preq], dtype=np.float64)
        self._cql_cost = self.dtype(cost.mean())
        return (preq - dq).astype(self.dtype)                 # the parent's deltas = preq - targets become the dq rows

    def gradients(self, minibatch):
        self._clip = self.clip_error
        self.clip_error = 0
        try:
            g, _, deltas, preq = super().gradients(minibatch)
        finally:
            self.clip_error = self._clip
        return g, self._cql_cost, deltas, preq


class CQLOracle(_CQL, OracleDQN):
    pass


class CQLOracleNStep(_CQL, _NStep, OracleDQN):
    pass
