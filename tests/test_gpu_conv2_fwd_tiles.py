"""conv2_fwd below B = 128 (fp32) runs on tiles of 48 x 32 (gemm_engine.h: gemm_tile_m48; write-through form at B <= 32, plain stores
above): at B = 32, 216 workgroups, one per CU, instead of 324.  The stage is checked in place, the way tests/test_gpu_fc4_dgrad_tiles.py
checks fc4_dgrad: one train step from seeded weights and a seeded minibatch, then the stage's operands (a1 of both nets — a Rectlin
output, about half zeros — and W2 of both nets) and its output a2 are read back and the product is redone in numpy, in fp64 and in plain
fp32 — and on the engine's 32 x 32 body (tuning hook nw:1 = 16), whose bits the 48-row tiles reproduce."""
import functools

import numpy as np
import pytest

from oracle.dqn_numpy import OracleDQN, xavier_weights
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu
A = 4
K1, PIX1, K2, PIX2, CRS2 = 32, 400, 64, 81, 512


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


@functools.lru_cache(maxsize=None)
def _weights():
    ws, wt = xavier_weights(A, 41), xavier_weights(A, 42)
    # W2 in the stage's orientation: Neon rows (c, r, s) -> k = (r, s, c), the order of an im2col row of the NHWC a1
    inner = lambda w: np.ascontiguousarray(w[1].reshape(K1, 16, K2).transpose(1, 0, 2).reshape(CRS2, K2))
    return ws, wt, inner(ws), inner(wt)


def _step(sd, B, wide=False):
    ws, wt, _, _ = _weights()
    args = make_args(batch_size=B)
    net = sd.DeepQNetwork(A, args)
    if wide:
        net.set_option("nw:1", 16)      # tuning hook: conv2_fwd on the engine's 32 x 32 body, 16 waves per tile (LAT_NW16)
    if args.target_steps:
        net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.train(random_minibatch(B, A, 43, reward_range=(-3, 4)))
    a1 = net.debug_read("a1", 2 * B * PIX1 * K1).reshape(2, B, 20, 20, K1)
    a2 = net.debug_read("a2", 2 * B * PIX2 * K2).reshape(2, B * PIX2, K2)
    return a1, a2, bool(args.target_steps)


def _patches(a1, dtype):
    """im2col rows of conv2 (4 x 4 taps, stride 2) of the NHWC a1: [net][B * 81][(r, s, c) = 512]"""
    x = a1.astype(dtype)
    p = np.stack([x[:, :, r:r + 18:2, s:s + 18:2, :] for r in range(4) for s in range(4)], axis=4)      # [z][n][p][q][tap][c]
    return p.reshape(2, -1, CRS2)


@pytest.mark.parametrize("B", [1, 2, 17, 31, 32, 33, 127])
def test_stage(sd, B):
    a1, a2, target = _step(sd, B)
    _, _, w_on, w_tg = _weights()
    w = np.stack([w_on, w_tg if target else w_on])
    z1, z2 = float((a1 == 0).mean()), float((a2 == 0).mean())
    print("B=%d: a1 zero fraction %.2f, a2 zero fraction %.2f" % (B, z1, z2))
    assert 0.1 < z1 < 0.9 and 0.1 < z2 < 0.9 and np.abs(a2).max() > 0 and a2.min() >= 0
    # (a) not further from fp64 than plain fp32 numpy is (both nets)
    ref64 = np.maximum(np.matmul(_patches(a1, np.float64), w.astype(np.float64)), 0)
    ref32 = np.maximum(np.matmul(_patches(a1, np.float32), w), 0)
    err, err32, top = float(np.abs(a2 - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    print("B=%d: max |a2 - fp64| %.3e, numpy fp32 %.3e, max |a2| %.3e" % (B, err, err32, top))
    assert err <= 1.5 * err32 + 1e-7 * top
    # (b) a second run from the same state gives the same bits
    again = _step(sd, B)
    assert np.array_equal(again[0].view(np.uint32), a1.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), a2.view(np.uint32))
    # (c) the 48 x 32 tiles add the same k in the same order as the 32 x 32 body (m48_map.h on n16_map.h's kslot): the same bits, both nets
    wide = _step(sd, B, wide=True)
    assert np.array_equal(wide[0].view(np.uint32), a1.view(np.uint32))
    for z in range(2):
        assert np.array_equal(wide[1][z].view(np.uint32), a2[z].view(np.uint32)), "net %d" % z


def test_whole_step_gradients(sd):
    """The stage in the step: one B = 32 train step against the oracle's gradients, every layer (all of them hang on a2)."""
    B = 32
    ws, wt, _, _ = _weights()
    args = make_args(batch_size=B)
    net = sd.DeepQNetwork(A, args)
    if args.target_steps:
        net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.set_option("keep_gradients", 1)
    o = OracleDQN(A, batch_size=B, weights=ws, clip_error=args.clip_error, discount_rate=args.discount_rate,
                  min_reward=args.min_reward, max_reward=args.max_reward, target_steps=args.target_steps)
    o.Wt = [x.copy() for x in wt] if args.target_steps else o.W
    mb = random_minibatch(B, A, 44, reward_range=(-3, 4))
    g = o.gradients(mb)[0]
    net.train(mb)
    for i in range(5):
        gg = net.get_layer(i, which=3)
        assert np.abs(gg - g[i]).max() < 1e-4 * max(1e-3, np.abs(g[i]).max()), "grad layer %d" % i
