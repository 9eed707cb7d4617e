"""The 48 x 32 tile body of the latency engine (gemm_engine.h: gemm_tile_m48, conv2_fwd below B = 128) on the CPU: tests/emul/emul_m48.cpp
runs a simulated workgroup through the very maps the kernel uses (simple_dqn_amd/csrc/m48_map.h: the 16 x 16 x 4 fragment and accumulator
lanes on n16_map.h's k-slot map, the eight combine panels used twice, the epilogue's elements per thread) and through Conv2Fwd's own index
functions and store."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PIX1, K1, PIX2, K2, CRS2 = 400, 32, 81, 64, 512


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libsdqn_emul_m48.so")
    src = os.path.join(HERE, "emul", "emul_m48.cpp")
    hdrs = [os.path.join(HERE, "..", "simple_dqn_amd", "csrc", h) for h in ("problems.h", "n16_map.h", "m48_map.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_chunk_is_covered_exactly_once(emul):
    """One wave's 32-deep chunk: the 48 instructions form every product A[row][k] * B[k][col] of the 48 x 32 x 32 block exactly once, A and
    B agree on k in every k-slot (and with n16_map.h's kslot), every product lands in the register that claims its (row, col)."""
    count = np.zeros((48, 32, 32), np.int32)
    assert emul.m48_chunk_cover(_ip(count)) == 0
    assert count.min() == 1 and count.max() == 1


def _run(emul, B, a1, w2, ids):
    M = B * PIX2
    a2 = np.full((2, M, K2), np.nan, np.float32)
    cnt = np.zeros((2, M, K2), np.int32)
    conf = np.zeros(4, np.int32)
    order = np.zeros(16, np.int32)
    bad = emul.m48_conv2_fwd(B, _fp(a1), _fp(w2), _fp(a2), ids, _ip(cnt), _ip(conf), _ip(order))
    assert bad == 0          # no thread read a panel slot nobody wrote, and every thread added the waves in thread 0's order
    return a2, cnt, conf, order


@pytest.fixture(scope="module")
def w2():
    return (np.random.RandomState(12).standard_normal((2, CRS2, K2)) * 0.05).astype(np.float32)


@pytest.mark.parametrize("B", [1, 31, 33])
def test_epilogue_hits_every_address_exactly_once(emul, w2, B):
    """ceil(81 B / 48) row tiles x 2 column tiles x 2 nets (B = 1, 31, 33: 81, 2 511 and 2 673 rows, ragged last tiles — 33, 15 and 33 rows —
    and tiles that straddle samples): the epilogue stores every (net, m, n) exactly once, and with the element's id as the value every a2
    address receives exactly its own element — the [net][m][64] address the 32 x 32 body's store uses."""
    a1 = np.ones((2, B * PIX1, K1), np.float32)
    a2, cnt, _, _ = _run(emul, B, a1, w2, 1)
    assert cnt.min() == 1 and cnt.max() == 1
    ids = (np.arange(2 * B * PIX2 * K2, dtype=np.int64) + 1).astype(np.float32).reshape(2, B * PIX2, K2)
    assert np.array_equal(a2, ids)


@pytest.mark.parametrize("B", [1, 31, 33])
def test_values_order_and_banks(emul, w2, B):
    rng = np.random.RandomState(200 + B)
    a1 = np.maximum(rng.standard_normal((2, B * PIX1, K1)), 0).astype(np.float32)          # a Rectlin output: about half zeros
    a2, cnt, conf, order = _run(emul, B, a1, w2, 0)
    # the two-half combine adds the sixteen partial tiles in wave order
    assert order.tolist() == list(range(16))
    # the same k in the same order as the 32 x 32 body (fmaf-chain model of both MFMA forms): the same bits
    same = np.empty_like(a2)
    emul.n32_conv2_fwd_ref(B, _fp(a1), _fp(w2), _fp(same))
    assert np.array_equal(a2.view(np.uint32), same.view(np.uint32))
    # against fp64: im2col rows of net z (4 x 4 taps, stride 2, 32 channels) x W2[z]
    x = a1.reshape(2, B, 20, 20, K1).astype(np.float64)
    pat = np.stack([x[:, :, r:r + 18:2, s:s + 18:2, :] for r in range(4) for s in range(4)], axis=4)      # [z][n][p][q][tap][c]
    ref = np.einsum("zmk,zkn->zmn", pat.reshape(2, B * PIX2, CRS2), w2.astype(np.float64))
    # an fp32 sum of 32 products per chunk, then of 16 partial sums: at most 48 roundings on the way of any term, 2^-24 each (a priori bound)
    bound = 48 * 2.0 ** -24 * np.einsum("zmk,zkn->zmn", np.abs(pat.reshape(2, B * PIX2, CRS2)), np.abs(w2).astype(np.float64)).max()
    assert np.abs(a2 - np.maximum(ref, 0)).max() <= bound
    assert (a2 == 0).any() and (a2 > 0).any()
    # combine panels at pitch 36: neither the stores (rows 4 apart x 16 columns per group) nor the reads (one row per group) meet a conflict;
    # the A panel (n16_map.h's B panel: pitch 17, rows permuted by krow): neither its transposing stores nor its fragment reads
    assert conf.tolist() == [0, 0, 0, 0], conf
