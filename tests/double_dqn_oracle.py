"""Double DQN restatement of the numpy oracles (test helper, not product code).

Double Q-learning (van Hasselt, Guez and Silver 2016) changes one line of deepqnetwork.py's train step (:124): the bootstrap value of
sample n is the TARGET net's Q at the action the ONLINE net rates highest on the poststate,

    a*[n]       = argmax_a Q(theta, post)[n, a]          (first maximum, numpy argmax)
    maxpostq[n] = Q(theta-, post)[n, a*[n]]

Everything else (targets, clip, cost, backward, optimizer) is the parent's.  Q(theta, post) is the parent's `fprop` of the online
weights: the network's own precision and, with batch_norm, inference mode with the online running statistics as they stand BEFORE the
step's training-mode forward moves them.  Without a target net (theta- aliases theta) the result is standard DQN.
"""
import numpy as np

from oracle.dqn_bn_numpy import OracleDQNBN
from oracle.dqn_numpy import OracleDQN


class _DoubleDQN:
    last_online_postq = None       # Q(theta, post) of the last gradients() call (None: no target net, standard DQN)
    last_target_postq = None
    last_maxpostq = None
    choose = None                  # optional (online_postq, target_postq) -> actions, replacing the argmax (tests: follow a device's near-tie choice)

    def gradients(self, minibatch):
        post = minibatch[3]
        if self.target_enabled:
            x = self._normalize(post)
            self.last_online_postq = self.fprop(self.W, x)            # before the parent's forward (BN: pre-step running statistics)
            self.last_target_postq = self.fprop(self.Wt, x)           # :119-120, as the parent computes it
        else:
            self.last_online_postq = self.last_target_postq = None
        return super().gradients(minibatch)

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        if self.last_online_postq is not None:
            a = self.last_online_postq.argmax(axis=1) if self.choose is None else self.choose(self.last_online_postq, self.last_target_postq)
            maxpostq = self.last_target_postq[np.arange(len(a)), a]
        self.last_maxpostq = np.array(maxpostq)
        return super().td_targets(preq, maxpostq, actions, rewards, terminals)


class DoubleDQNOracle(_DoubleDQN, OracleDQN):
    pass


class DoubleDQNOracleBN(_DoubleDQN, OracleDQNBN):
    pass
