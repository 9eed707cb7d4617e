"""--n_step on the CPU: the library's host sampler against the numpy restatement (tests/nstep_oracle.py), the validity rule, the return
loop and the command line."""
import ctypes as C

import numpy as np
import pytest

import nstep_oracle as N
import simple_dqn_amd as sd
from oracle.replay_numpy import MT19937, ReplayOracle
from simple_dqn_amd import _lib
from simple_dqn_amd.replay_memory import nstep_returns


def _rings(n_rings, seed, size_lo=24, size_hi=400):
    """(terminals, count, current, hist, size): partly filled rings and full ones with `current` anywhere inside"""
    rng = np.random.RandomState(seed)
    for t in range(n_rings):
        size = int(rng.randint(size_lo, size_hi))
        hist = int(rng.randint(1, 5))
        term = rng.rand(size) < [0.0, 0.03, 0.15][t % 3]
        if t % 2:
            count, current = size, int(rng.randint(0, size))
        else:
            count = int(rng.randint(hist + 17, size + 1))
            current = count % size
        yield term, count, current, hist, size


def _lib_sample_n(lib, seed, term, count, current, hist, n, batch):
    mt = (C.c_uint32 * _lib.MT_WORDS)()
    _lib.check(lib.sdqn_mt_seed(mt, seed))
    out = np.empty(batch, np.int64)
    draws = C.c_int64()
    t8 = np.ascontiguousarray(term, dtype=np.uint8)
    _lib.check(lib.sdqn_sample_indices_n(mt, _lib.ptr(t8, C.c_uint8), count, current, hist, n, batch, _lib.ptr(out, C.c_int64),
                                         C.byref(draws)))
    return out, draws.value


def test_oracle_n1_equals_reference_sampler():
    for k, (term, count, current, hist, size) in enumerate(_rings(24, 0)):
        mem = ReplayOracle(size, 4, 4, hist, 32)
        mem.terminals[:] = term
        mem.count, mem.current = count, current
        if not N.valid_mask(term, count, current, hist, size, 1).any():
            continue
        ref = mem.sample_indexes(MT19937(100 + k))
        rng = MT19937(100 + k)
        idx, draws = N.sample_indexes(rng, term, count, current, hist, 1, 32)
        assert list(idx) == list(ref), k
        # the same number of MT words: both generators are in the same state afterwards
        rng2 = MT19937(100 + k)
        mem.sample_indexes(rng2)
        assert rng.getstate() == rng2.getstate(), k


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_library_sampler_equals_oracle(n):
    lib = sd.load()
    checked = 0
    for k, (term, count, current, hist, size) in enumerate(_rings(30, 10 + n)):
        if count < hist + n or not N.valid_mask(term, count, current, hist, size, n).any():
            continue
        idx, draws = _lib_sample_n(lib, 7 + k, term, count, current, hist, n, 32)
        o_idx, o_draws = N.sample_indexes(MT19937(7 + k), term, count, current, hist, n, 32)
        assert np.array_equal(idx, o_idx), (n, k)
        assert draws == o_draws, (n, k)
        assert N.valid_mask(term, count, current, hist, size, n)[idx].all()
        if n == 1:
            mt = (C.c_uint32 * _lib.MT_WORDS)()
            _lib.check(lib.sdqn_mt_seed(mt, 7 + k))
            out, d1 = np.empty(32, np.int64), C.c_int64()
            t8 = np.ascontiguousarray(term, dtype=np.uint8)
            _lib.check(lib.sdqn_sample_indices(mt, _lib.ptr(t8, C.c_uint8), count, current, hist, 32, _lib.ptr(out, C.c_int64),
                                               C.byref(d1)))
            assert np.array_equal(out, idx) and d1.value == draws
        checked += 1
    assert checked >= 10


def test_n_step_changes_the_sample():
    """n = 3 rejects windows that n = 1 accepts: on a full ring the two samplers part ways"""
    lib = sd.load()
    term = np.zeros(100, bool)
    a, _ = _lib_sample_n(lib, 3, term, 100, 50, 4, 1, 256)
    b, _ = _lib_sample_n(lib, 3, term, 100, 50, 4, 3, 256)
    assert not np.array_equal(a, b)
    assert not ((b + 2 >= 50) & (b - 4 < 50)).any()


def test_library_sampler_refusals():
    lib = sd.load()
    term = np.zeros(50, np.uint8)
    mt = (C.c_uint32 * _lib.MT_WORDS)()
    _lib.check(lib.sdqn_mt_seed(mt, 1))
    out = np.empty(4, np.int64)
    for n, count in ((0, 50), (17, 50), (3, 6)):           # out of range, and count < hist + n
        rc = lib.sdqn_sample_indices_n(mt, _lib.ptr(term, C.c_uint8), count, 0, 4, n, 4, _lib.ptr(out, C.c_int64), None)
        assert rc == -1, (n, count)                        # SDQN_ERR_ARG
    assert lib.sdqn_sample_indices_n(mt, _lib.ptr(term, C.c_uint8), 7, 7 % 50, 4, 3, 4, _lib.ptr(out, C.c_int64), None) == 0
    assert (out == 4).all()


def test_validity_mask_equals_rejection_rule():
    for n in (1, 2, 3, 7, 16):
        for k, (term, count, current, hist, size) in enumerate(_rings(30, 50 + n)):
            m = N.valid_mask(term, count, current, hist, size, n)
            ref = np.array([N.accepts(i, term, count, current, hist, n) for i in range(size)])
            assert np.array_equal(m, ref), (n, k)


def test_returns_hand_worked():
    g = 0.5
    rew = np.array([1, 2, -3, 5, 1, 0, 1, 1], dtype=np.int64)
    term = np.zeros(8, bool)
    R, d = N.returns(rew, term, [0], 3, g, -10, 10)
    assert R[0] == 1 + 0.5 * 2 + 0.25 * -3 and not d[0]
    term0 = term.copy(); term0[2] = True                     # terminal at k = 0
    R, d = N.returns(rew, term0, [2], 3, g, -10, 10)
    assert R[0] == -3.0 and d[0]
    termm = term.copy(); termm[3] = True                     # in the middle
    R, d = N.returns(rew, termm, [2], 4, g, -10, 10)
    assert R[0] == -3 + 0.5 * 5 and d[0]
    terml = term.copy(); terml[4] = True                     # at k = n - 1
    R, d = N.returns(rew, terml, [2], 3, g, -10, 10)
    assert R[0] == -3 + 0.5 * 5 + 0.25 * 1 and d[0]
    R, d = N.returns(rew, term, [3], 2, g, -1, 1)            # per-step clip: 5 counts as 1
    assert R[0] == 1 + 0.5 * 1 and not d[0]
    R, d = N.returns(rew, term, [3], 1, 0.99, -1, 1)         # n = 1: clip(r) itself
    assert R[0] == 1.0 and not d[0]
    assert N.gamma_n(3, 0.99) == 0.99 * 0.99 * 0.99 and N.gamma_n(1, 0.99) == 0.99


def test_package_returns_equal_oracle_bit_for_bit():
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 5, 16):
        rew = rng.randint(-3, 4, 500).astype(np.int64)
        term = rng.rand(500) < 0.1
        idx = rng.randint(4, 500 - n + 1, 256)
        R, d = nstep_returns(rew, term, idx, n, 0.99, -1.0, 1.0)
        oR, od = N.returns(rew, term, idx, n, 0.99, -1.0, 1.0)
        assert R.dtype == np.float64 and d.dtype == np.bool_
        assert np.array_equal(R.view(np.int64), oR.view(np.int64)), n
        assert np.array_equal(d, od), n


def test_nstep_targets_oracle_n1_identity():
    """with n = 1 the n-step target form equals the standard one bit for bit (0.0 + 1.0 r = r, 1.0 gamma = gamma)"""
    rew = np.array([-2, 0, 1, 3], dtype=np.int64)
    term = np.array([False, True, False, False])
    R, d = N.returns(rew, term, [0, 1, 2, 3], 1, 0.99, -1.0, 1.0)
    assert np.array_equal(R, np.clip(rew, -1, 1).astype(np.float64)) and np.array_equal(d, term)


def test_parser_default_and_flag():
    from simple_dqn_amd import main as M
    assert M.build_parser().parse_args([]).n_step == 1
    assert M.build_parser().parse_args(["--n_step", "3"]).n_step == 3
