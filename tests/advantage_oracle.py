"""Advantage-learning restatement of the numpy oracles (test helper, not product code).

Advantage Learning and Persistent Advantage Learning (Bellemare, Ostrovski, Guez, Thomas and Munos 2016, "Increasing the Action Gap")
change how deepqnetwork.py's train step computes its targets (:119-143) and nothing else.  With qbar(s) = Q(theta-, s):

    gap(q, a) = max_k q[k] - q[a]                                    (>= 0, exactly 0 when a is a maximiser)
    y_std[n]  = r_c[n] + (terminal ? 0 : gamma max_a qbar(s'_n)[a])
    y_AL[n]   = y_std[n] - alpha gap(qbar(s_n), a_n)                 (on terminal transitions too)
    y_PAL[n]  = terminal ? y_AL[n] : max(y_AL[n], y_std[n] - alpha gap(qbar(s'_n), a_n))

in float64 from the network's own Q-values (n-step: R, done, gamma^n in the places of r_c, terminal, gamma).  qbar is the parent's
`fprop` of the TARGET weights, on the prestates and on the poststates; without a target net theta- aliases theta.
`advantage_learning = 0` is the parent's step (tests switch the option between steps).
"""
import numpy as np

from nstep_oracle import _NStep, gamma_n
from oracle.dqn_numpy import OracleDQN
from per_oracle import _PER


def gap(q, actions):
    """max_k q[k] - q[a] per row in Python floats (= float64)"""
    return np.array([max(float(x) for x in row) - float(row[int(a)]) for row, a in zip(q, actions)], dtype=np.float64)


class _AdvantageLearning:
    advantage_learning = 0.9       # alpha; 0: the parent's targets
    persistent_advantage = False   # y_PAL instead of y_AL
    last_pre_target_q = None       # qbar(s) of the last gradients() call
    last_post_target_q = None      # qbar(s')
    last_gap_pre = None            # gap(qbar(s), a), float64
    last_gap_post = None           # gap(qbar(s'), a)
    last_y_std = None              # the standard targets of the taken actions, float64
    last_y = None                  # the targets of the taken actions, float64 (before they are stored in the network's precision)
    last_pal_took_post = None      # bool per sample: y_PAL chose the poststate's gap (always False on terminal rows and without PAL)

    def gradients(self, minibatch):
        if self.advantage_learning:
            self.last_pre_target_q = self.fprop(self.Wt, self._normalize(minibatch[0]))
            self.last_post_target_q = self.fprop(self.Wt, self._normalize(minibatch[3]))     # :119-120, as the parent computes it
        return super().gradients(minibatch)

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        alpha = float(self.advantage_learning)
        if not alpha:
            return super().td_targets(preq, maxpostq, actions, rewards, terminals)
        self.last_gap_pre = gap(self.last_pre_target_q, actions)
        self.last_gap_post = gap(self.last_post_target_q, actions)
        n = int(getattr(self, "n_step", 1))
        if n > 1:
            r, gam = [float(x) for x in rewards], gamma_n(n, self.discount_rate)        # R, clipped per step already
        else:
            r, gam = [float(x) for x in np.clip(rewards, self.min_reward, self.max_reward)], self.discount_rate
        targets = preq.copy()
        y, ystd = np.zeros(len(actions), dtype=np.float64), np.zeros(len(actions), dtype=np.float64)
        took = np.zeros(len(actions), dtype=bool)
        for i, action in enumerate(actions):
            ystd[i] = r[i] if terminals[i] else r[i] + gam * float(maxpostq[i])
            y[i] = ystd[i] - alpha * float(self.last_gap_pre[i])
            if self.persistent_advantage and not terminals[i]:
                yp = ystd[i] - alpha * float(self.last_gap_post[i])
                if yp > y[i]:
                    y[i], took[i] = yp, True
            targets[i, action] = y[i]
        self.last_y_std, self.last_y, self.last_pal_took_post = ystd, y, took
        return targets


class AdvantageOracle(_AdvantageLearning, OracleDQN):
    pass


class AdvantageOracleNStep(_AdvantageLearning, _NStep, OracleDQN):
    pass


class AdvantageOraclePER(_PER, _AdvantageLearning, OracleDQN):
    pass


class AdvantageOraclePERNStep(_PER, _AdvantageLearning, _NStep, OracleDQN):
    pass
