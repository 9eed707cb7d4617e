"""fc4_dgrad below B = 128 (fp32) runs on 196 tiles of 32 x 16 (gemm_engine.h: gemm_tile_n16; write-through form at B <= 32, plain
stores above).  The stage is checked in place, the way tests/test_gpu_dqn.py::test_forward_stages checks the forward stages: one train
step from seeded weights and a seeded minibatch, then the stage's operands (d4, a3 — about half of each is zero: Rectlin — and W4) and
its outputs (dense d3, padded d3p) are read back and the product is redone in numpy, in fp64 and in plain fp32 — and on the engine's
32 x 32 body, whose bits the narrow tiles reproduce."""
import functools

import numpy as np
import pytest

from oracle.dqn_numpy import OracleDQN, xavier_weights
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu
NIN4, NFC, PD3, K3 = 3136, 512, 11, 64


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


@functools.lru_cache(maxsize=None)
def _weights(A):
    ws, wt = xavier_weights(A, 41), xavier_weights(A, 42)
    # W4 in the stage's orientation: d3[b, (pix, f)] = sum_k d4[b, k] * W4neon[k, (f, pix)]
    w = np.ascontiguousarray(ws[3].reshape(NFC, K3, 49).transpose(0, 2, 1).reshape(NFC, NIN4))
    return ws, wt, w


def _step(sd, A, B, wide=False):
    ws, wt, _ = _weights(A)
    args = make_args(batch_size=B)
    net = sd.DeepQNetwork(A, args)
    if wide:
        net.set_option("nw:5", 16)      # tuning hook: fc4_dgrad on the engine's 32 x 32 body, 16 waves per tile (LAT_NW16)
    if args.target_steps:
        net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.train(random_minibatch(B, A, 43, reward_range=(-3, 4)))
    d4 = net.debug_read("d4", B * NFC).reshape(B, NFC)
    a3 = net.debug_read("a3", 2 * B * NIN4).reshape(2, B, NIN4)[0]
    d3 = net.debug_read("d3", B * NIN4).reshape(B, NIN4)
    d3p = net.debug_read("d3p", B * PD3 * PD3 * K3).reshape(B, PD3, PD3, K3)
    return d4, a3, d3, d3p


@pytest.mark.parametrize("A", [4, 18])
@pytest.mark.parametrize("B", [1, 2, 17, 31, 32, 33, 127])
def test_stage(sd, A, B):
    d4, a3, d3, d3p = _step(sd, A, B)
    w = _weights(A)[2]
    z4, z3 = float((d4 == 0).mean()), float((a3 <= 0).mean())
    print("B=%d A=%d: d4 zero fraction %.2f, a3 <= 0 fraction %.2f" % (B, A, z4, z3))
    assert 0.2 < z4 < 0.8 and 0.2 < z3 < 0.8 and (a3 == 0).any() and np.abs(d4).max() > 0
    # (a) masked elements and the padded border are exactly zero
    off = a3 <= 0
    assert not d3[off].any()
    border = d3p.copy()
    border[:, 2:9, 2:9, :] = 0
    assert not border.any()
    # (b) the padded plane's interior is the dense copy, bit for bit (n = (pix = p * 7 + q, f))
    assert np.array_equal(d3p[:, 2:9, 2:9, :].reshape(B, NIN4).view(np.uint32), d3.view(np.uint32))
    # (c) not further from fp64 than plain fp32 numpy is
    ref64 = d4.astype(np.float64) @ w.astype(np.float64)
    ref64[off] = 0
    ref32 = d4 @ w
    ref32[off] = 0
    err, err32, top = float(np.abs(d3 - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    print("B=%d A=%d: max |d3 - fp64| %.3e, numpy fp32 %.3e, max |d3| %.3e" % (B, A, err, err32, top))
    assert err <= 1.5 * err32 + 1e-7 * top
    # (d) a second run from the same state gives the same bits
    again = _step(sd, A, B)
    assert np.array_equal(again[2].view(np.uint32), d3.view(np.uint32)) and np.array_equal(again[3].view(np.uint32), d3p.view(np.uint32))
    # (e) the 32 x 16 tiles add the same k in the same order as the 32 x 32 body (n16_map.h: kslot): the same bits
    wide = _step(sd, A, B, wide=True)
    assert np.array_equal(wide[0].view(np.uint32), d4.view(np.uint32)) and np.array_equal(wide[1].view(np.uint32), a3.view(np.uint32))
    assert np.array_equal(wide[2].view(np.uint32), d3.view(np.uint32)) and np.array_equal(wide[3].view(np.uint32), d3p.view(np.uint32))


def test_whole_step_gradients(sd):
    """The stage in the step: one B = 32 train step against the oracle's gradients, every layer (conv1..conv3 hang on d3)."""
    A, B = 4, 32
    ws, wt, _ = _weights(A)
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
