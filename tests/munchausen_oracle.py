"""Munchausen DQN restatement of the numpy oracles (test helper, not product code).

Munchausen DQN (Vieillard, Pietquin and Geist 2020) changes how deepqnetwork.py's train step computes its targets (:119-143) and nothing
else.  With qbar(s) = Q(theta-, s) and pi = softmax(qbar / tau):

    lse(q) = v + tau log(sum_a exp((q[a] - v) / tau)),  v = max_a q[a]            (sum in action order)
    V[n]   = lse(qbar(s'_n))
    m[n]   = alpha clip(qbar(s_n)[a_n] - lse(qbar(s_n)), l0, 0)
    y[n]   = (r_c[n] + m[n]) + (terminal ? 0 : gamma V[n])

in float64 from the network's own Q-values (n-step: R, done, gamma^n in the places of r_c, terminal, gamma).  qbar is the parent's
`fprop` of the TARGET weights, on the prestates and on the poststates; without a target net theta- aliases theta.  `munchausen = False`
is the parent's step (tests switch the option between steps).
"""
import math

import numpy as np

from nstep_oracle import _NStep, gamma_n
from oracle.dqn_numpy import OracleDQN
from per_oracle import _PER


def lse(q, tau):
    """lse of one Q row in Python floats (= float64), the sum in action order"""
    q = [float(x) for x in q]
    v = max(q)
    s = 0.0
    for x in q:
        s += math.exp((x - v) / tau)
    return v + tau * math.log(s)


def soft_value(q, tau):
    return np.array([lse(row, tau) for row in q], dtype=np.float64)


def bonus(q, actions, alpha, tau, clip):
    """alpha clip(tau ln pi(a | s), clip, 0) per row"""
    out = []
    for row, a in zip(q, actions):
        lp = float(row[int(a)]) - lse(row, tau)
        out.append(alpha * min(max(lp, clip), 0.0))
    return np.array(out, dtype=np.float64)


class _Munchausen:
    munchausen = True
    munchausen_alpha, munchausen_tau, munchausen_clip = 0.9, 0.03, -1.0
    last_V = None                  # lse(qbar(s')) of the last gradients() call, float64
    last_bonus = None              # m
    last_pre_target_q = None       # qbar(s)
    last_post_target_q = None      # qbar(s')
    last_y = None                  # the targets of the taken actions, float64 (before they are stored in the network's precision)

    def gradients(self, minibatch):
        if self.munchausen:
            self.last_pre_target_q = self.fprop(self.Wt, self._normalize(minibatch[0]))
            self.last_post_target_q = self.fprop(self.Wt, self._normalize(minibatch[3]))     # :119-120, as the parent computes it
        return super().gradients(minibatch)

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        if not self.munchausen:
            return super().td_targets(preq, maxpostq, actions, rewards, terminals)
        alpha, tau, l0 = self.munchausen_alpha, self.munchausen_tau, self.munchausen_clip
        self.last_V = soft_value(self.last_post_target_q, tau)
        self.last_bonus = bonus(self.last_pre_target_q, actions, alpha, tau, l0)
        n = int(getattr(self, "n_step", 1))
        if n > 1:
            r, gam = [float(x) for x in rewards], gamma_n(n, self.discount_rate)        # R, clipped per step already
        else:
            r, gam = [float(x) for x in np.clip(rewards, self.min_reward, self.max_reward)], self.discount_rate
        targets = preq.copy()
        y = np.zeros(len(actions), dtype=np.float64)
        for i, action in enumerate(actions):
            rm = r[i] + float(self.last_bonus[i])
            y[i] = rm if terminals[i] else rm + gam * float(self.last_V[i])
            targets[i, action] = y[i]
        self.last_y = y
        return targets


class MunchausenOracle(_Munchausen, OracleDQN):
    pass


class MunchausenOracleNStep(_Munchausen, _NStep, OracleDQN):
    pass


class MunchausenOraclePER(_PER, _Munchausen, OracleDQN):
    pass


class MunchausenOraclePERNStep(_PER, _Munchausen, _NStep, OracleDQN):
    pass
