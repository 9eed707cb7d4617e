"""Oracle of dormant-neuron recycling (--redo_interval), written from the feature's statement, in the reference's (Neon)
weight layouts — what DeepQNetwork.get_layer returns:

  layer 0  W1 (256, 32)      rows (c, r, s)
  layer 1  W2 (512, 64)      rows (c, r, s), c = row // 16
  layer 2  W3 (576, 64)      rows (c, r, s), c = row // 9
  layer 3  W4 (512, 3136)    columns (f, pix), f = col // 49
  layer 4  W5 (A, 512)

The library's flat buffers hold W1i [(c,r,s)][32], W2i [(r,s,c)][64], W3i [(r,s,c)][64], W4i [(pix,f)][512], W5i [A][512] one behind the other
(to_internal / from_internal below); a draw is keyed by the entry's index in that flat buffer.

  score    m_l[j] = mean over rows of |a_l[row][j]|, s_l[j] = m_l[j] / mean_k m_l[k], all zeros when the layer mean is 0.  The sums are taken
           in extended precision (np.longdouble: 64 mantissa bits on x86) and rounded to float64 once, so the oracle's own error is a few
           2^-53 and the bound rows * 2^-52 on an fp64 sum in any order is the device's to use
  dormant  s <= tau
  recycle  incoming weights of a dormant unit: (2 u / 2^24 - 1) * k in float32, u = top 24 bits of one splitmix64 word keyed by (seed, event,
           flat index), k = float32(sqrt(3 / fan_in)); every weight of the next layer that multiplies a dormant unit: +0.0 (wins over a draw);
           optimizer state at all those positions: +0.0
"""
import math

import numpy as np

UNITS = (32, 64, 64, 512)
EDGES = (0, 32, 96, 160, 672)
FAN_IN = (256, 512, 576, 3136)
SIZES = (256 * 32, 512 * 64, 576 * 64, 3136 * 512)
OFFS = (0, 8192, 8192 + 32768, 8192 + 32768 + 36864, 8192 + 32768 + 36864 + 1605632)
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
def mix(z):
    """splitmix64's finaliser on a Python integer"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, event):
    return mix(mix(seed + G) + G * (event + 1))


def word(seed, event, index):
    return mix(key(seed, event) + G * (index + 1))


def bound(layer):
    """k of layer 1..4"""
    return np.float32(math.sqrt(3.0 / FAN_IN[layer - 1]))


def draw(seed, event, index, layer):
    """(word, float32 value) of one entry, in Python integers and one float32 operation at a time"""
    w = word(seed, event, index)
    u = w >> 40
    t = np.float32(np.float32(u) * np.float32(2.0 ** -23)) - np.float32(1.0)
    return w, np.float32(np.float32(t) * bound(layer))


def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, event, indexes, layer):
    """the same draw for an array of flat indexes (uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        idx = np.asarray(indexes).astype(np.uint64)
        w = _mix_np(np.uint64(key(seed, event)) + np.uint64(G) * (idx + np.uint64(1)))
    u = (w >> np.uint64(40)).astype(np.float32)
    return (u * np.float32(2.0 ** -23) - np.float32(1.0)) * bound(layer)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def to_internal(ws):
    """five Neon-layout arrays -> the flat internal buffer"""
    w1, w2, w3, w4, w5 = ws
    return np.concatenate([np.asarray(w1).reshape(-1),
                           np.asarray(w2).reshape(32, 16, 64).transpose(1, 0, 2).reshape(-1),
                           np.asarray(w3).reshape(64, 9, 64).transpose(1, 0, 2).reshape(-1),
                           np.asarray(w4).reshape(512, 64, 49).transpose(2, 1, 0).reshape(-1),
                           np.asarray(w5).reshape(-1)]).astype(np.float32)


def from_internal(flat, A):
    o = OFFS
    return [flat[o[0]:o[1]].reshape(256, 32).copy(),
            flat[o[1]:o[2]].reshape(16, 32, 64).transpose(1, 0, 2).reshape(512, 64).copy(),
            flat[o[2]:o[3]].reshape(9, 64, 64).transpose(1, 0, 2).reshape(576, 64).copy(),
            flat[o[3]:o[4]].reshape(49, 64, 512).transpose(2, 1, 0).reshape(512, 3136).copy(),
            flat[o[4]:o[4] + A * 512].reshape(A, 512).copy()]


def flat_index_maps(A):
    """per layer, an integer array shaped like the Neon weights: every entry's index in the flat internal buffer"""
    idx = [np.arange(o, o + n, dtype=np.int64) for o, n in zip(OFFS[:4], SIZES)] + [np.arange(OFFS[4], OFFS[4] + A * 512, dtype=np.int64)]
    flat = np.concatenate(idx)
    return from_internal(flat, A)


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------
def scores64(acts):
    """acts: four arrays [rows][units] -> four float64 score vectors"""
    out = []
    for a in acts:
        a = np.asarray(a)
        m = (np.abs(a.astype(np.longdouble)).sum(axis=0) / np.longdouble(a.shape[0]))
        mean = m.sum() / np.longdouble(m.size)
        out.append((m / mean).astype(np.float64) if mean > 0 else np.zeros(m.size, np.float64))
    return out


def scores(acts):
    """... rounded to float32, concatenated: what the library's 672-value buffer holds"""
    return np.concatenate(scores64(acts)).astype(np.float32)


def dormant(score_vec, tau):
    s = np.asarray(score_vec, dtype=np.float32).astype(np.float64)
    return [s[EDGES[l]:EDGES[l + 1]] <= tau for l in range(4)]


def apply(score_vec, tau, seed, event, weights, states=()):
    """One event.  weights: five Neon-layout arrays; states: any number of such lists (optimizer states).  Returns (new weights, new states,
    masks) with masks = per layer {"redrawn", "zeroed"} boolean arrays in the Neon shapes; nothing is changed in place."""
    d = dormant(score_vec, tau)
    A = weights[4].shape[0]
    fidx = flat_index_maps(A)
    # (which unit an entry feeds, which unit it multiplies) as broadcastable masks in the Neon shapes
    feeds = [np.broadcast_to(d[0][None, :], (256, 32)), np.broadcast_to(d[1][None, :], (512, 64)), np.broadcast_to(d[2][None, :], (576, 64)),
             np.broadcast_to(d[3][:, None], (512, 3136)), np.zeros((A, 512), bool)]
    mult = [np.zeros((256, 32), bool), np.broadcast_to(np.repeat(d[0], 16)[:, None], (512, 64)), np.broadcast_to(np.repeat(d[1], 9)[:, None], (576, 64)),
            np.broadcast_to(np.repeat(d[2], 49)[None, :], (512, 3136)), np.broadcast_to(d[3][None, :], (A, 512))]
    new_w, masks = [], []
    for l in range(5):
        zeroed = mult[l].copy()
        redrawn = feeds[l] & ~zeroed
        w = np.array(weights[l], dtype=np.float32, copy=True)
        if l < 4 and redrawn.any():
            w[redrawn] = draws(seed, event, fidx[l][redrawn], l + 1)
        w[zeroed] = np.float32(0.0)
        new_w.append(w)
        masks.append({"redrawn": redrawn, "zeroed": zeroed})
    new_s = []
    for st in states:
        cur = []
        for l in range(5):
            s = np.array(st[l], dtype=np.float32, copy=True)
            s[masks[l]["redrawn"] | masks[l]["zeroed"]] = np.float32(0.0)
            cur.append(s)
        new_s.append(cur)
    return new_w, new_s, masks
