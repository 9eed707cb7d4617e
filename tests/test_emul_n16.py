"""The 32 x 16 tile body of the latency engine (gemm_engine.h: gemm_tile_n16, fc4_dgrad below B = 128) on the CPU: tests/emul/emul_n16.cpp
runs a simulated workgroup through the very maps the kernel uses (simple_dqn_amd/csrc/n16_map.h: loader items, the two LDS panels, the
16 x 16 x 4 fragment and accumulator lanes, the combine panel, the epilogue's element per thread) and through Fc4Dgrad's own index
functions and store."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NIN4, NFC, PD3, K3, Q3 = 3136, 512, 11, 64, 7


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libsdqn_emul_n16.so")
    src = os.path.join(HERE, "emul", "emul_n16.cpp")
    hdrs = [os.path.join(HERE, "..", "simple_dqn_amd", "csrc", h) for h in ("problems.h", "n16_map.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_chunk_is_covered_exactly_once_without_bank_conflicts(emul):
    """One wave's 32-deep chunk: the 16 instructions form every product A[row][k] * B[k][col] of the 32 x 16 x 32 block exactly once, A and
    B agree on k in every k-slot, every product lands in the register that claims its (row, col) — and neither the panel stores nor the
    fragment reads meet a bank conflict (the pitches 33 / 17 and the row permutation of n16_map.h are chosen for that)."""
    count = np.zeros((32, 16, 32), np.int32)
    conf = np.zeros(3, np.int32)
    bad = emul.n16_chunk_cover(_ip(count), _ip(conf))
    assert bad == 0
    assert count.min() == 1 and count.max() == 1
    assert conf.tolist() == [0, 0, 0], conf


def _run(emul, B, d4, w4i, a3, ids):
    d3 = np.full((B, NIN4), np.nan, np.float32)
    d3p = np.zeros((B, PD3, PD3, K3), np.float32)            # the border is zeroed once at allocation and never written
    cnt = np.zeros((B, NIN4), np.int32)
    conf = np.zeros(2, np.int32)
    assert emul.n16_fc4_dgrad(B, _fp(d4), _fp(w4i), _fp(a3), _fp(d3), _fp(d3p), ids, _ip(cnt), _ip(conf)) == 0
    return d3, d3p, cnt, conf


@pytest.fixture(scope="module")
def w4i():
    return (np.random.RandomState(11).standard_normal((NIN4, NFC)) * 0.05).astype(np.float32)


@pytest.mark.parametrize("B", [1, 31, 33])
def test_epilogue_hits_every_address_exactly_once(emul, w4i, B):
    """196 column tiles x ceil(B / 32) row tiles: the epilogue stores every (m, n) of the B x 3136 result exactly once (ragged last row
    tile included), and with the element's id as the value every d3 address and every interior d3p address receives exactly its own
    element; the d3p border stays zero."""
    d4 = np.ones((B, NFC), np.float32)
    a3 = np.ones((B, NIN4), np.float32)
    d3, d3p, cnt, _ = _run(emul, B, d4, w4i, a3, 1)
    assert cnt.min() == 1 and cnt.max() == 1
    ids = (np.arange(B * NIN4, dtype=np.int64) + 1).astype(np.float32).reshape(B, NIN4)
    assert np.array_equal(d3, ids)
    assert np.array_equal(d3p[:, 2:9, 2:9, :].reshape(B, NIN4), ids)             # n = (pix = p * 7 + q, f)
    border = d3p.copy()
    border[:, 2:9, 2:9, :] = 0
    assert not border.any()


@pytest.mark.parametrize("B", [1, 31, 33])
def test_values_and_mask(emul, w4i, B):
    rng = np.random.RandomState(100 + B)
    d4 = rng.standard_normal((B, NFC)).astype(np.float32)
    d4[rng.rand(B, NFC) < 0.5] = 0
    a3 = rng.standard_normal((B, NIN4)).astype(np.float32)
    a3[rng.rand(B, NIN4) < 0.2] = 0
    d3, d3p, cnt, conf = _run(emul, B, d4, w4i, a3, 0)
    ref = d4.astype(np.float64) @ w4i.astype(np.float64).T
    ref[a3 <= 0] = 0
    # an fp32 sum of 32 products per chunk, then of 16 partial sums: at most 48 roundings on the way of any term, 2^-24 each (a priori bound)
    bound = 48 * 2.0 ** -24 * (np.abs(d4).astype(np.float64) @ np.abs(w4i).astype(np.float64).T).max()
    assert np.abs(d3 - ref).max() <= bound
    assert not d3[a3 <= 0].any()
    # the same k in the same order as the 32 x 32 body (fmaf-chain model of both MFMA forms): the same bits
    same = np.empty((B, NIN4), np.float32)
    emul.n32_fc4_dgrad_ref(B, _fp(d4), _fp(w4i), _fp(a3), _fp(same))
    assert np.array_equal(d3.view(np.uint32), same.view(np.uint32))
    assert np.array_equal(d3p[:, 2:9, 2:9, :].reshape(B, NIN4), d3)
    # combine panel: the stores may meet a 2-way conflict (free on ds_write_b32), the 16 reads per thread none
    assert conf[1] == 0 and conf[0] <= 8 * 2, conf
