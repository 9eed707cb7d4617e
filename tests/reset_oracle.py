"""Oracle of periodic resets with shrink-and-perturb (--reset_interval), written from the feature's statement, on the
library's flat internal buffers [W1i | W2i | W3i | W4i | W5i] (redo_oracle.to_internal / from_internal convert from and to the layouts
DeepQNetwork.get_layer returns; the event is a function of an entry's flat index and its layer alone, so no layout enters here).

  factor   alpha_l = 0 for the last `layers` of the five layers, ALPHA for the others
  entry    alpha_l == 1: untouched | alpha_l == 0: theta = phi | else theta = fma(a, theta, float32(b phi)), a = float32(ALPHA),
           b = float32(1.0 - ALPHA) with the subtraction in float64.  The target net: the same with the same phi.  Optimizer states: +0.0
           wherever alpha_l < 1
  draw     phi = (u 2^-23 - 1) k in float32, k = float32(sqrt(3 / fan_in)), fan_in 256, 512, 576, 3136, 512; u = the top 24 bits of
           mix(key + G (i + 1)), key = mix((mix(seed + G) ^ DOMAIN) + G (event + 1)) — redo_oracle.key without the DOMAIN
  fma      a theta is exact in float64 (two 24-bit significands).  Its sum with float32(b phi) is taken in float64 ROUNDED TO ODD (the
           error of the float64 addition is recovered exactly by Knuth's two-sum and, where it is not zero, the sum is truncated toward zero
           and its last bit set), so that the following rounding to float32 is the only one that counts: 53 bits are more than 24 + 2, the
           condition under which round-to-odd followed by round-to-nearest equals one round-to-nearest of the exact value
"""
import math

import numpy as np

from redo_oracle import G, M64, OFFS, _mix_np, mix

DOMAIN = 0x52455345545F5350
FAN_IN = (256, 512, 576, 3136, 512)
LAYERS = 5


def size(A):
    return OFFS[4] + 512 * A


def edges(A):
    """flat index of the first entry of layer 1..5 and one past the last"""
    return tuple(OFFS) + (size(A),)


def key(seed, event):
    return mix((mix(seed + G) ^ DOMAIN) + G * (event + 1))


def word(seed, event, index):
    return mix(key(seed, event) + G * (index + 1))


def bound(layer):
    """k of layer 1..5"""
    return np.float32(math.sqrt(3.0 / FAN_IN[layer - 1]))


def draw(seed, event, index, layer):
    """(word, float32 value) of one entry, in Python integers and one float32 operation at a time"""
    w = word(seed, event, index)
    u = w >> 40
    t = np.float32(np.float32(u) * np.float32(2.0 ** -23)) - np.float32(1.0)
    return w, np.float32(np.float32(t) * bound(layer))


def draws(seed, event, indexes, layer):
    """the same draw for an array of flat indexes (uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        idx = np.asarray(indexes).astype(np.uint64)
        w = _mix_np(np.uint64(key(seed, event)) + np.uint64(G) * (idx + np.uint64(1)))
    u = (w >> np.uint64(40)).astype(np.float32)
    return (u * np.float32(2.0 ** -23) - np.float32(1.0)) * bound(layer)


def fma32(a, x, c):
    """float32 fma(a, x, c) of a float32 scalar a and float32 arrays x, c: one rounding of the exact a x + c (see the module's note)"""
    p = np.float64(a) * x.astype(np.float64)                   # exact
    q = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + q
        bb = s - p
        err = (p - (s - bb)) + (q - bb)                        # two-sum: p + q == s + err exactly (finite values)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
    if fix.any():
        bits = s.view(np.int64).copy()
        # truncate toward zero where the rounding went away from zero (err and s of opposite signs), then make the last bit odd
        away = fix & ((err < 0.0) == (s > 0.0))
        bits[away] -= 1                                        # (sign-magnitude: one ulp toward zero; s != 0 where err != 0)
        bits[fix] |= 1
        s = bits.view(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return s.astype(np.float32)


def alphas(layers, alpha):
    """the five layers' factors"""
    return tuple(0.0 if l > LAYERS - layers else float(alpha) for l in range(1, LAYERS + 1))


def touched(layers, alpha, A):
    """boolean [size(A)]: the entries whose alpha_l < 1"""
    m = np.zeros(size(A), bool)
    e = edges(A)
    for l, al in enumerate(alphas(layers, alpha)):
        if al < 1.0:
            m[e[l]:e[l + 1]] = True
    return m


def apply(layers, alpha, seed, event, A, theta, theta_t=None, states=()):
    """One event on flat internal float32 buffers.  theta_t None: no target net.  Returns (theta, theta_t or None, [states]) as new arrays;
    nothing is changed in place."""
    a, b = np.float32(alpha), np.float32(1.0 - float(alpha))
    nets = [np.array(theta, dtype=np.float32, copy=True)] + ([] if theta_t is None else [np.array(theta_t, dtype=np.float32, copy=True)])
    sts = [np.array(s, dtype=np.float32, copy=True) for s in states]
    e = edges(A)
    for l, al in enumerate(alphas(layers, alpha)):
        if al == 1.0:
            continue
        lo, hi = e[l], e[l + 1]
        phi = draws(seed, event, np.arange(lo, hi), l + 1)
        for w in nets:
            w[lo:hi] = phi if al == 0.0 else fma32(a, w[lo:hi], (b * phi).astype(np.float32))
        for s in sts:
            s[lo:hi] = np.float32(0.0)
    return nets[0], (nets[1] if theta_t is not None else None), sts
