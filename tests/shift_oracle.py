"""--random_shift restated in numpy from DESIGN.md §34 (not from the kernel): the key mix, the draws, the shift.

  stream  splitmix64: mix(z) = the finaliser, next(s): s += GOLD, return mix(s)
          k  = mix(seed + GOLD (t + 1));  s0 = mix(k + ODD (2 n + s + 1))      (mod 2^64)
          dy = next % (2P + 1) - P, dx likewise from the following output
  shift   out[f, y, x] = in[f, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)] for every frame f of the state
"""
import numpy as np

M64 = (1 << 64) - 1
GOLD, ODD = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, step, n, s, P):
    """(dy, dx) of sample n, state s (0 prestate, 1 poststate) of shifted step `step`"""
    k = mix((seed + GOLD * (step + 1)) & M64)
    g = mix((k + ODD * (2 * n + s + 1)) & M64)
    out = []
    for _ in range(2):
        g = (g + GOLD) & M64
        out.append(int(mix(g) % (2 * P + 1)) - P)
    return out[0], out[1]


def draws(seed, step, B, P):
    """int8 [B][2][2]: (dy, dx) per sample and state, the layout of DeepQNetwork.last_shifts()"""
    return np.array([[draw(seed, step, n, s, P) for s in (0, 1)] for n in range(B)], np.int8)


def shift(state, dy, dx):
    """state u8 [hist][H][W] -> the shifted state, through clamped index vectors"""
    H, W = state.shape[-2:]
    ys = np.clip(np.arange(H) + int(dy), 0, H - 1)
    xs = np.clip(np.arange(W) + int(dx), 0, W - 1)
    return np.take(np.take(state, ys, axis=-2), xs, axis=-1)


def shift_minibatch(pre, post, seed, step, P):
    """(shifted prestates, shifted poststates, draws) of one step's minibatch [B][hist][H][W]"""
    d = draws(seed, step, len(pre), P)
    spre = np.stack([shift(pre[n], *d[n, 0]) for n in range(len(pre))])
    spost = np.stack([shift(post[n], *d[n, 1]) for n in range(len(post))])
    return spre, spost, d


def forced_seed(B, P, step=0, limit=1000):
    """the first seed < limit under which some sample of step `step` draws (-P, -P) and another (+P, +P), in either state; None if none does"""
    for seed in range(limit):
        d = draws(seed, step, B, P).reshape(B, 2, 2)
        lo = {n for n in range(B) for s in (0, 1) if tuple(d[n, s]) == (-P, -P)}
        hi = {n for n in range(B) for s in (0, 1) if tuple(d[n, s]) == (P, P)}
        if any(a != b for a in lo for b in hi):
            return seed
    return None
