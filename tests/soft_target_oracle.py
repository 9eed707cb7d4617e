"""Soft (Polyak) target updates, --target_tau, restated in numpy: the blend in float32 / float64 exactly as the library
specifies it (three operations, each rounded once), an fp64 DQN oracle whose target follows it, and the Agent's hard-update schedule."""
import numpy as np

from oracle.dqn_numpy import OracleDQN


def blend(theta, theta_t, tau, dtype=np.float32):
    """theta- + tau_f * (theta - theta-) in `dtype`: d, m and the sum are separate numpy operations, so each is rounded once"""
    w, wt = np.asarray(theta, dtype=dtype), np.asarray(theta_t, dtype=dtype)
    t = dtype(tau)
    d = w - wt
    m = t * d
    return wt + m


def blend32_through_fp64(theta, theta_t, tau):
    """what a contracted / wider evaluation would give: the same float32 inputs and tau_f, the arithmetic in double, ONE rounding"""
    w, wt = np.asarray(theta, np.float32).astype(np.float64), np.asarray(theta_t, np.float32).astype(np.float64)
    return (wt + np.float64(np.float32(tau)) * (w - wt)).astype(np.float32)


class SoftTargetOracle(OracleDQN):
    """OracleDQN whose every train step is followed by one blend of its target net (in the oracle's own dtype)"""

    def __init__(self, *a, tau=0.0, **kw):
        super().__init__(*a, **kw)
        self.tau = tau

    def soft_update(self, tau=None):
        tau = self.tau if tau is None else tau
        if self.Wt is not self.W:
            self.Wt = [blend(w, wt, tau, self.dtype) for w, wt in zip(self.W, self.Wt)]

    def train(self, minibatch, epoch=0):
        out = super().train(minibatch, epoch)
        if self.tau > 0:
            self.soft_update()
        return out


def hard_updates(calls, train_steps, target_steps, target_tau, start=0):
    """Environment steps (counted over all Agent.train calls, from `start`) at which Agent.train makes a hard target update:
    target_tau == 0: the reference's `i % target_steps == 0` of every call; target_tau > 0: only total_train_steps == 0."""
    out, total = [], start
    for _ in range(calls):
        for i in range(train_steps):
            if target_steps and ((total == 0) if target_tau > 0 else (i % target_steps == 0)):
                out.append(total)
            total += 1
    return out
