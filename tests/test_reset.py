"""Periodic resets with shrink-and-perturb (--reset_interval) without a device: the library's host restatement (csrc/reset.h
through sdqn_reset_apply_host / sdqn_reset_draw) against tests/reset_oracle.py, bit for bit; the draw's domain against ReDo's; the command
line's ranges and refusals; the C ABI's symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reset_oracle as O
from util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD5678
RULES = [(2, 1.0), (2, 0.5), (0, 0.5), (5, 0.0), (1, 0.25)]
OPTIMIZERS = ("rmsprop", "adam", "adadelta")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def random_buffers(A, seed):
    """theta, theta_t: normals of the weights' scale with a few values whose shrunk sum is inexact in every way (huge, tiny, zero, negative
    zero); state > 0, state2 any sign"""
    rng = np.random.RandomState(seed)
    n = O.size(A)
    theta = (rng.standard_normal(n) * 0.05).astype(np.float32)
    theta_t = (rng.standard_normal(n) * 0.05).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-38, -1e-42, 3e38, -3e38, 1.0, 2.0 ** -24], np.float32)
    for buf in (theta, theta_t):
        for lo in O.edges(A)[:5]:
            buf[lo:lo + special.size] = special
    state = (np.abs(rng.standard_normal(n)) + 0.5).astype(np.float32)
    state2 = rng.standard_normal(n).astype(np.float32)
    return theta, theta_t, state, state2


@pytest.mark.parametrize("A", [1, 4, 18])
@pytest.mark.parametrize("optimizer", OPTIMIZERS)
@pytest.mark.parametrize("layers,alpha", RULES)
def test_host_restatement_matches_the_oracle(layers, alpha, optimizer, A):
    from simple_dqn_amd.deepqnetwork import reset_apply_host
    before = random_buffers(A, 100 + A)
    got = [b.copy() for b in before]
    reset_apply_host(layers, alpha, SEED, 3, A, optimizer, *got)
    two = optimizer != "rmsprop"
    want_w, want_t, want_s = O.apply(layers, alpha, SEED, 3, A, before[0], before[1], before[2:4] if two else before[2:3])
    assert np.array_equal(bits(got[0]), bits(want_w)) and np.array_equal(bits(got[1]), bits(want_t))
    assert np.array_equal(bits(got[2]), bits(want_s[0]))
    # the second state is the optimizer's business: rmsprop has none, and what is handed in stays as it is
    assert np.array_equal(bits(got[3]), bits(want_s[1] if two else before[3]))
    m = O.touched(layers, alpha, A)
    assert m.sum() == {(2, 1.0): 3136 * 512 + 512 * A, (1, 0.25): O.size(A), (2, 0.5): O.size(A), (0, 0.5): O.size(A), (5, 0.0): O.size(A)}[(layers, alpha)]
    for k in range(4):                                         # alpha_l == 1: the same bits in all four buffers
        assert np.array_equal(bits(got[k])[~m], bits(before[k])[~m]), k
    assert not bits(got[2])[m].any() and (not two or not bits(got[3])[m].any())      # +0.0, sign bit included
    # a fully reset layer is identical in both nets; a shrunk one is not
    al = O.alphas(layers, alpha)
    e = O.edges(A)
    for l in range(5):
        same = np.array_equal(bits(got[0][e[l]:e[l + 1]]), bits(got[1][e[l]:e[l + 1]]))
        assert same == (al[l] == 0.0), l
        if al[l] == 0.0:
            assert np.array_equal(bits(got[0][e[l]:e[l + 1]]), bits(O.draws(SEED, 3, np.arange(e[l], e[l + 1]), l + 1))), l


def test_without_a_target_net_there_is_one_write():
    from simple_dqn_amd.deepqnetwork import reset_apply_host
    theta, _, state, _ = random_buffers(4, 5)
    want_w, none, want_s = O.apply(1, 0.25, SEED, 2, 4, theta, None, (state,))
    a, s = theta.copy(), state.copy()
    reset_apply_host(1, 0.25, SEED, 2, 4, "rmsprop", a, a, s)               # aliased
    b = theta.copy()
    reset_apply_host(1, 0.25, SEED, 2, 4, "rmsprop", b, None, None)         # absent, and no state at all
    assert none is None and np.array_equal(bits(a), bits(want_w)) and np.array_equal(bits(b), bits(want_w)) and np.array_equal(bits(s), bits(want_s[0]))


def test_nan_is_healed_where_the_layer_is_redrawn_and_kept_where_it_is_shrunk():
    from simple_dqn_amd.deepqnetwork import reset_apply_host
    A = 4
    theta, theta_t, state, state2 = random_buffers(A, 6)
    e = O.edges(A)
    spots = [e[0] + 17, e[2] + 5, e[3] + 12345, e[4] + 7, e[5] - 1]           # conv1, conv3 (shrunk at (2, 0.5)); fc4, fc5 (redrawn)
    vals = np.array([np.nan, np.inf, np.nan, -np.inf, np.nan], np.float32)
    theta[spots] = vals
    theta_t[spots[::-1]] = vals
    state[spots] = np.nan
    reset_apply_host(2, 0.5, SEED, 1, A, "adam", theta, theta_t, state, state2)
    assert np.isnan(theta[spots[0]]) and np.isinf(theta[spots[1]]) and np.isinf(theta_t[spots[1]]) and np.isnan(theta_t[spots[0]])
    assert np.isfinite(theta[e[3]:]).all() and np.isfinite(theta_t[e[3]:]).all()
    assert np.isfinite(theta).sum() == theta.size - 2 and not state.view(np.uint32).any()
    want_w, want_t, _ = O.apply(2, 0.5, SEED, 1, A, *_nan_inputs(A, spots, vals))
    assert np.array_equal(bits(theta), bits(want_w)) and np.array_equal(bits(theta_t), bits(want_t))


def _nan_inputs(A, spots, vals):
    theta, theta_t, _, _ = random_buffers(A, 6)
    theta[spots] = vals
    theta_t[spots[::-1]] = vals
    return theta, theta_t


def test_oracle_fma_is_one_rounding():
    """the float64 emulation against exact rational arithmetic, on sums built to sit on a float32 tie after a float64 rounding"""
    from fractions import Fraction
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(2000) * 0.05).astype(np.float32)
    c = (rng.standard_normal(2000) * 0.03).astype(np.float32)
    # a x = 1 + 2^-24 + 2^-40 exactly is not representable; take x = 1 + 2^-23, a = 1 - 2^-24 ... and tiny addends beyond float64's reach
    x[:4] = np.array([1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23, 3.0, 1.5], np.float32)
    c[:4] = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -80, -2.0 ** -90], np.float32)
    for a in (np.float32(0.5), np.float32(0.25), np.float32(1.0 - 2.0 ** -24), np.float32(1.0 / 3.0)):
        got = O.fma32(a, x, c)
        for k in range(x.size):
            exact = Fraction(float(a)) * Fraction(float(x[k])) + Fraction(float(c[k]))
            lo = np.float32(float(exact))                      # Python rounds a Fraction to float64 correctly; near a tie check both sides
            cand = sorted({lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}, key=lambda v: abs(Fraction(float(v)) - exact))
            d0, d1 = abs(Fraction(float(cand[0])) - exact), abs(Fraction(float(cand[1])) - exact)
            best = cand[0] if d0 != d1 else (cand[0] if not (int(np.float32(cand[0]).view(np.uint32)) & 1) else cand[1])
            assert np.float32(got[k]).view(np.uint32) == np.float32(best).view(np.uint32), (float(a), k)


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
def test_draw_bits_and_bounds():
    from simple_dqn_amd.deepqnetwork import reset_draw
    e = O.edges(18)
    cases = [(0, 0, 0, 1), (SEED, 1, 8191, 1), (SEED, 2, 8192, 2), (2 ** 64 - 1, 7, 40960, 3), (SEED, 2 ** 40, 77824, 4), (5, 3, e[4], 5),
             (SEED, 9, e[5] - 1, 5)]
    for seed, event, index, layer in cases:
        w, v = reset_draw(seed, event, index, layer)
        ow, ov = O.draw(seed, event, index, layer)
        assert w == ow and bits(np.float32(v)) == bits(np.float32(ov)), (seed, event, index)
        assert np.array_equal(bits(O.draws(seed, event, [index], layer)), bits(np.array([ov])))
        assert reset_draw(seed, event, index, layer)[0] == w                                 # the same arguments repeat
    assert reset_draw(SEED, 1, 5, 1)[0] != reset_draw(SEED + 1, 1, 5, 1)[0]                  # two seeds differ
    assert reset_draw(SEED, 1, 5, 1)[0] != reset_draw(SEED, 2, 5, 1)[0]
    assert [float(O.bound(l)) for l in (1, 2, 3, 4, 5)] == [float(np.float32(np.sqrt(3.0 / f))) for f in (256, 512, 576, 3136, 512)]
    # every draw of an event lies inside [-k, k) of its layer; u = 0 and u = 2^24 - 1 are the ends.  The mean of n draws of U(-k, k) has
    # standard deviation k / sqrt(3 n): six of them (2e-9 by chance) hold a sign or scale mistake out, not the generator's quality
    for l in range(5):
        x = O.draws(SEED, 1, np.arange(e[l], e[l + 1]), l + 1)
        k = O.bound(l + 1)
        assert x.min() >= -k and x.max() < k and abs(float(x.astype(np.float64).mean())) < 6 * float(k) / np.sqrt(3.0 * x.size), l
        lib = np.array([reset_draw(SEED, 1, i, l + 1)[1] for i in range(e[l], e[l] + 64)], np.float32)
        assert np.array_equal(bits(lib), bits(x[:64])), l
    assert float(np.float32(np.float32(0.0) * np.float32(2.0 ** -23) - np.float32(1.0)) * O.bound(4)) == -float(O.bound(4))


def test_fc5_bound_is_what_the_network_draws_fc5_from():
    """DeepQNetwork.__init__ draws every layer from U(-k, k), k = sqrt(3 / fan_in), fan_in = shape[1] for the two affine layers: 512 for fc5"""
    from oracle.dqn_numpy import layer_shapes
    for A in (1, 4, 18):
        assert [s[0] if i < 3 else s[1] for i, s in enumerate(layer_shapes(A, 4, 84, 84))] == list(O.FAN_IN)


def test_reset_and_redo_never_share_a_word():
    from simple_dqn_amd.deepqnetwork import redo_draw, reset_draw
    rng = np.random.RandomState(11)
    events = rng.randint(1, 1000, 4096)
    idx = rng.randint(0, 1683456, 4096)
    events[:64] = np.arange(1, 65); idx[:64] = 0                                             # the first events at the first entry
    layer = [1 + int(np.searchsorted(O.edges(4)[1:5], i, side="right")) for i in idx]
    seen_redo, seen_reset = set(), set()
    for e_, i, l in zip(events, idx, layer):
        wr, wd = reset_draw(SEED, int(e_), int(i), l)[0], redo_draw(SEED, int(e_), int(i), min(l, 4))[0]
        assert wr != wd, (e_, i)
        seen_reset.add(wr); seen_redo.add(wd)
    assert not (seen_reset & seen_redo)                                                       # nor across the sampled (e, i)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from simple_dqn_amd.main import build_parser
    return build_parser().parse_args(list(argv))


def test_flags_and_their_ranges():
    from simple_dqn_amd.main import check_reset
    a = _parse()
    assert (a.reset_interval, a.reset_layers, a.shrink_perturb) == (0, 2, 1.0)
    assert check_reset(a) == (0, 2, 1.0)
    assert check_reset(make_args()) == (0, 2, 1.0)                         # a namespace without the flags: off
    assert check_reset(_parse("--reset_interval", "40000", "--reset_layers", "1", "--shrink_perturb", "0.5")) == (40000, 1, 0.5)
    assert check_reset(_parse("--reset_layers", "0", "--shrink_perturb", "1")) == (0, 0, 1.0)      # nothing to do, but nothing asked either
    for argv, word in ((("--reset_interval", "-1"), "--reset_interval -1"), (("--reset_layers", "6"), "--reset_layers 6"),
                       (("--reset_layers", "-1"), "--reset_layers"), (("--shrink_perturb", "1.5"), "--shrink_perturb 1.5"),
                       (("--shrink_perturb", "-0.1"), "--shrink_perturb"), (("--shrink_perturb", "nan"), "--shrink_perturb")):
        with pytest.raises(ValueError, match=word):
            check_reset(_parse(*argv))


REFUSED = [(("--batch_norm", "true"), "--batch_norm"), (("--noisy_nets", "true"), "--noisy_nets"), (("--datatype", "float64"), "float64"),
           (("--screen_height", "96", "--screen_width", "96"), "84 x 84"),
           (("--reset_layers", "0", "--shrink_perturb", "1"), "--reset_layers 0 --shrink_perturb 1")]


@pytest.mark.parametrize("other,word", REFUSED)
def test_refusals_in_both_orders_before_the_device(other, word):
    from simple_dqn_amd.main import run
    ours = ("--reset_interval", "5")
    for argv in (ours + other, other + ours):
        with pytest.raises(ValueError, match=word) as e:                   # (this box has no device: touching one raises something else)
            run(_parse(*argv, "--random_steps", "0", "--train_steps", "0", "--test_steps", "0", "--epochs", "0"))
        assert "--reset_interval 5" in str(e.value)


def test_everything_else_composes_on_the_command_line():
    from simple_dqn_amd.main import check_redo, check_reset
    for argv in (("--dueling", "true"), ("--prioritized_replay", "true", "--n_step", "3"), ("--double_dqn", "true"), ("--datatype", "float16"),
                 ("--bootstrap_heads", "2"), ("--quantiles", "4"), ("--munchausen", "true"), ("--cql_alpha", "1"), ("--random_shift", "4"),
                 ("--clip_grad_norm", "10"), ("--target_tau", "0.01"), ("--advantage_learning", "0.9"), ("--optimizer", "adam"),
                 ("--redo_interval", "1000"), ("--target_steps", "0")):
        a = _parse("--reset_interval", "10", "--shrink_perturb", "0.5", *argv)
        assert check_reset(a) == (10, 2, 0.5) and check_redo(a)[0] in (0, 1000)


def test_library_refuses_bad_arguments_without_a_device():
    import simple_dqn_amd as sd
    from simple_dqn_amd.deepqnetwork import reset_apply_host, reset_draw
    err = (AssertionError, sd.SdqnError)
    theta = np.zeros(O.size(4), np.float32)
    for layers, alpha, word in ((6, 0.5, "reset_layers"), (-1, 0.5, "reset_layers"), (2, 1.5, "shrink_perturb"), (2, -0.5, "shrink_perturb"),
                                (2, float("nan"), "shrink_perturb")):
        with pytest.raises(err, match=word):
            reset_apply_host(layers, alpha, 0, 1, 4, "rmsprop", theta)
    with pytest.raises(err):
        reset_apply_host(2, 0.5, 0, 1, 19, "rmsprop", np.zeros(O.size(19), np.float32))
    with pytest.raises(err, match="state2"):
        reset_apply_host(2, 0.5, 0, 1, 4, "adam", theta, None, theta.copy(), None)
    with pytest.raises(err):
        reset_draw(0, 1, 0, 6)
    with pytest.raises(err):
        reset_draw(0, 1, -1, 1)
    assert not theta.any()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("sdqn_net_set_reset", "sdqn_net_get_reset", "sdqn_net_reset_now", "sdqn_net_reset_last", "sdqn_reset_apply_host", "sdqn_reset_draw")


def test_symbols_in_header_export_map_and_signatures():
    import simple_dqn_amd as sd
    from simple_dqn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    exports = open(os.path.join(ROOT, "simple_dqn_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*sdqn_\*;", exports)                      # the map exports the header's prefix and nothing else
    lib = sd.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype is C.c_int


def test_setters_refuse_a_null_handle():
    import simple_dqn_amd as sd
    lib = sd.load()
    out = (C.c_int64 * 2)()
    assert lib.sdqn_net_set_reset(None, 3, 2, 1.0, 0) != 0 and lib.sdqn_net_reset_now(None) != 0 and lib.sdqn_net_reset_last(None, out) != 0


def test_option_table_still_lists_eleven_names():
    import simple_dqn_amd as sd
    lib = sd.load()
    names = []
    for k in range(64):
        s = lib.sdqn_option_name(k)
        if not s:
            break
        names.append(s.decode())
    assert len(names) == 11 and not any("reset" in n or "shrink" in n for n in names)
