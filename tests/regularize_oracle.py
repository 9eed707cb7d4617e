"""Oracle of decoupled weight decay and L2-init regularisation (--weight_decay WD, --l2_init LAMBDA), written from the feature's
statement, on arrays of float32 weights of any shape (the rule is a function of one weight and its anchor alone, so no layout enters here).

  factors  kf = float32(1.0 - lr WD), cf = float32(lr LAMBDA), the arithmetic in float64 (Python floats), rounded once
  rule     v = theta;  WD > 0: v = v * kf;  LAMBDA > 0: v = v + cf * (anchor - v)   — numpy float32 arithmetic: every operation rounded on its own
           A coefficient of 0 skips its line (no multiplication by one, no anchor read)
  ranges   WD >= 0, LAMBDA >= 0, lr WD < 1, lr LAMBDA <= 1; a NaN is outside
  norms    per layer sum theta^2 and sum (theta - anchor)^2 over float64 terms (the square of a float32 is exact in float64), math.fsum: the
           correctly rounded sum, which any float64 summation of n non-negative terms meets within (n - 1) 2^-53 relative
"""
import math

import numpy as np

from redo_oracle import OFFS


def size(A):
    return OFFS[4] + 512 * A


def edges(A):
    """flat index of the first entry of layer 1..5 and one past the last"""
    return tuple(OFFS) + (size(A),)


def factors(wd, lam, lr):
    return np.float32(1.0 - float(lr) * float(wd)), np.float32(float(lr) * float(lam))


def in_range(wd, lam, lr):
    return bool(wd >= 0.0 and lam >= 0.0 and lr * wd < 1.0 and lr * lam <= 1.0)


def apply(wd, lam, lr, theta, anchor=None):
    """the new weights (a new array; theta is left alone)"""
    assert in_range(wd, lam, lr)
    kf, cf = factors(wd, lam, lr)
    v = np.array(theta, dtype=np.float32)
    with np.errstate(all="ignore"):
        if wd > 0.0:
            v = (v * kf).astype(np.float32)
        if lam > 0.0:
            a = np.asarray(anchor, dtype=np.float32)
            d = (a - v).astype(np.float32)
            m = (cf * d).astype(np.float32)
            v = (v + m).astype(np.float32)
    return v


def blend(theta, theta_t, tau):
    """soft target update: theta- + tau (theta - theta-), three float32 operations (soft_target_oracle's rule, restated for the chain tests)"""
    t = np.float32(tau)
    d = (np.asarray(theta, np.float32) - np.asarray(theta_t, np.float32)).astype(np.float32)
    return (np.asarray(theta_t, np.float32) + (t * d).astype(np.float32)).astype(np.float32)


def sums(theta_flat, anchor_flat, A):
    """([5] sum theta^2, [5] sum (theta - anchor)^2 or nan) per layer of the flat internal buffer, correctly rounded"""
    e = edges(A)
    th = np.asarray(theta_flat, np.float32).astype(np.float64)
    norms = [math.fsum((th[e[l]:e[l + 1]] ** 2).tolist()) for l in range(5)]
    if anchor_flat is None:
        return norms, [float("nan")] * 5
    d = th - np.asarray(anchor_flat, np.float32).astype(np.float64)
    return norms, [math.fsum((d[e[l]:e[l + 1]] ** 2).tolist()) for l in range(5)]
