"""--clip_grad_norm in numpy: the oracle's train step with the clip between `gradients` and `optimize`.

    norm  = sqrt(sum_i g_i^2) / bsz                fp64, over every layer's gradient SUM (the L2 norm of the mean gradient)
    scale = min(1, G / (norm + 1e-6))              fp64, then rounded once to the network's precision
    g_i  <- g_i * scale   if scale < 1             one multiply in the network's precision; otherwise (or norm not finite) g is untouched

oracle/ is imported and left as it is."""
import math

import numpy as np

from oracle.dqn_numpy import OracleDQN

CLIP_EPS = 1e-6


def grad_norm(grads, bsz):
    """L2 norm of the mean gradient, accumulated in fp64 from the stored values"""
    return math.sqrt(sum(float(np.square(np.asarray(g, np.float64)).sum()) for g in grads)) / float(bsz)


def clip_scale(norm, max_norm, dtype=np.float64):
    """the factor as it is applied: min(1, G / (norm + 1e-6)) in fp64, rounded once to dtype (1 for a non-finite norm)"""
    if not math.isfinite(norm):
        return np.dtype(dtype).type(1)
    return np.dtype(dtype).type(min(1.0, float(max_norm) / (norm + CLIP_EPS)))


def clip_gradients(grads, bsz, max_norm, dtype):
    """-> (grads clipped in dtype, norm, scale); the very same arrays when nothing is clipped"""
    norm = grad_norm(grads, bsz)
    scale = clip_scale(norm, max_norm, dtype)
    if not scale < 1:
        return grads, norm, scale
    t = np.dtype(dtype).type
    return [(np.asarray(g, t) * scale).astype(t) for g in grads], norm, scale


class ClipMixin:
    """train = gradients, clip, optimize; max norm in self.clip_grad_norm (0: off), the last step's (norm, scale) kept"""
    clip_grad_norm = 0.0
    last_norm = last_scale = None

    def train(self, minibatch, epoch=0):
        grads, cost, _, _ = self.gradients(minibatch)
        bsz = minibatch[0].shape[0]
        if self.clip_grad_norm > 0:
            grads, self.last_norm, self.last_scale = clip_gradients(grads, bsz, self.clip_grad_norm, self.dtype)
        self.optimize(grads, bsz, epoch)
        self.train_iterations += 1
        self.last_cost = cost
        if self.callback:
            self.callback.on_train(cost)
        return cost


class ClipOracle(ClipMixin, OracleDQN):
    def __init__(self, *a, clip_grad_norm=0.0, **kw):
        OracleDQN.__init__(self, *a, **kw)
        self.clip_grad_norm = float(clip_grad_norm)
