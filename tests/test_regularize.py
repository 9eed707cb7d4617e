"""Decoupled weight decay and L2-init regularisation (--weight_decay, --l2_init) without a device: the library's host
restatement (csrc/regularize.h through sdqn_regularize_apply_host) against tests/regularize_oracle.py, bit for bit; the command line's
ranges and refusals; the C ABI's symbols; the CSV header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dueling_oracle as DU
import regularize_oracle as O
from util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 0.01
COEFFS = [(0.1, 0.0), (0.0, 0.01), (0.1, 0.01)]
SPECIAL = np.array([0.0, -0.0, 1e-38, -1e-42, 1.4e-45, -1.4e-45, 3e38, -3e38, 3.4028235e38, 1.0, -1.0, 2.0 ** -24, 1.17549435e-38], np.float32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def random_buffers(A, seed):
    """theta and anchor: normals of the weights' scale, and at every layer's first entries every pairing of the special values (zeros of both
    signs, denormals, the largest finite values: products that underflow, differences that overflow)"""
    rng = np.random.RandomState(seed)
    n = O.size(A)
    theta = (rng.standard_normal(n) * 0.05).astype(np.float32)
    anchor = (rng.standard_normal(n) * 0.05).astype(np.float32)
    k = SPECIAL.size
    for lo in O.edges(A)[:5]:
        theta[lo:lo + k * k] = np.repeat(SPECIAL, k)          # (169 values: inside the smallest layer, fc5 with one row)
        anchor[lo:lo + k * k] = np.tile(SPECIAL, k)
    return theta, anchor


@pytest.mark.parametrize("A", [1, 4, 18])
@pytest.mark.parametrize("wd,lam", COEFFS)
def test_host_restatement_matches_the_oracle(wd, lam, A):
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    theta, anchor = random_buffers(A, 200 + A)
    got = theta.copy()
    regularize_apply_host(wd, lam, LR, got, anchor if lam > 0 else None)
    want = O.apply(wd, lam, LR, theta, anchor)
    assert np.array_equal(bits(got), bits(want))
    finite = np.isfinite(theta) & (np.abs(theta) > 1e-30) & (np.abs(theta) < 1e30)
    assert (bits(got)[finite] != bits(theta)[finite]).mean() > 0.99       # at this learning rate the rule moves (nearly) every weight's bits


def test_a_single_coefficient_is_the_combined_rule_with_the_other_at_zero():
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    theta, anchor = random_buffers(4, 7)
    a, b = theta.copy(), theta.copy()
    regularize_apply_host(0.1, 0.0, LR, a, None)              # WD alone needs no anchor ...
    regularize_apply_host(0.1, 0.0, LR, b, anchor)            # ... and does not read one
    assert np.array_equal(bits(a), bits(b))
    c = theta.copy()
    regularize_apply_host(0.1, 0.0, LR, c, anchor)
    regularize_apply_host(0.0, 0.01, LR, c, anchor)           # the two lines one behind the other = the combined rule
    d = theta.copy()
    regularize_apply_host(0.1, 0.01, LR, d, anchor)
    assert np.array_equal(bits(c), bits(d))


def test_both_coefficients_zero_leave_every_bit():
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    theta, anchor = random_buffers(4, 8)
    theta[:4] = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
    theta[4:5].view(np.uint32)[0] = 0x7FA00001                # a signalling NaN: multiplying by 1.0f would quiet it
    got = theta.copy()
    regularize_apply_host(0.0, 0.0, LR, got, anchor)
    assert np.array_equal(bits(got), bits(theta))
    got = theta.copy()
    regularize_apply_host(0.0, 0.0, LR, got, None)
    assert np.array_equal(bits(got), bits(theta))


@pytest.mark.parametrize("wd,lam", COEFFS)
def test_dueling_mask_entries_stay_plus_zero(wd, lam):
    """fc5 of a dueling net: +0.0 outside the two blocks, in the weights and in an anchor taken from such weights: +0 kf = +0 and
    +0 + cf (+0 - +0) = +0, so the rule needs no mask launch"""
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    A = 4
    rng = np.random.RandomState(3)
    w5 = DU.masked((rng.standard_normal((A + 1, 512)) * 0.05).astype(np.float32))
    an = DU.masked((rng.standard_normal((A + 1, 512)) * 0.05).astype(np.float32))
    m = DU.mask(A)
    assert not bits(w5)[~m].any() and not bits(an)[~m].any()
    got = w5.copy().reshape(-1)
    for _ in range(3):
        regularize_apply_host(wd, lam, LR, got, an.reshape(-1))
    got = got.reshape(A + 1, 512)
    assert not bits(got)[~m].any()                                        # +0.0, sign bit included
    assert (got[m] != w5[m]).mean() > 0.99


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from simple_dqn_amd.main import build_parser
    return build_parser().parse_args(list(argv))


def test_flags_and_their_ranges():
    from simple_dqn_amd.main import check_regularizer
    a = _parse()
    assert (a.weight_decay, a.l2_init, a.log_weight_norms) == (0.0, 0.0, False)
    assert check_regularizer(a) == (0.0, 0.0, False)
    assert check_regularizer(make_args()) == (0.0, 0.0, False)            # a namespace without the flags: off
    assert check_regularizer(_parse("--weight_decay", "0.1", "--l2_init", "0.01", "--log_weight_norms", "true")) == (0.1, 0.01, True)
    assert check_regularizer(_parse("--l2_init", "4000")) == (0.0, 4000.0, False)      # lr x LAMBDA = 1 exactly (lr 0.00025): allowed
    for argv, word in ((("--weight_decay", "-0.1"), "--weight_decay -0.1"), (("--weight_decay", "nan"), "--weight_decay"),
                       (("--l2_init", "-1"), "--l2_init -1"), (("--l2_init", "nan"), "--l2_init"),
                       (("--weight_decay", "4000"), "--weight_decay 4000"),           # lr x WD = 1: refused
                       (("--weight_decay", "50", "--learning_rate", "0.02"), "--weight_decay 50"),
                       (("--l2_init", "4001"), "--l2_init 4001"), (("--l2_init", "101", "--learning_rate", "0.01"), "--l2_init 101")):
        with pytest.raises(ValueError, match=word):
            check_regularizer(_parse(*argv))


REFUSED = [(("--batch_norm", "true"), "--batch_norm"), (("--noisy_nets", "true"), "--noisy_nets"), (("--datatype", "float64"), "float64"),
           (("--screen_height", "96", "--screen_width", "96"), "84 x 84")]
OURS = [(("--weight_decay", "0.1"), "--weight_decay 0.1"), (("--l2_init", "0.01"), "--l2_init 0.01"), (("--log_weight_norms", "true"), "--log_weight_norms")]


@pytest.mark.parametrize("ours,name", OURS)
@pytest.mark.parametrize("other,word", REFUSED)
def test_refusals_in_both_orders_before_the_device(other, word, ours, name):
    from simple_dqn_amd.main import run
    for argv in (ours + other, other + ours):
        with pytest.raises(ValueError, match=word) as e:                   # (this box has no device: touching one raises something else)
            run(_parse(*argv, "--random_steps", "0", "--train_steps", "0", "--test_steps", "0", "--epochs", "0"))
        assert name in str(e.value)


@pytest.mark.parametrize("argv,word", [(("--weight_decay", "-1"), "--weight_decay -1"), (("--l2_init", "nan"), "--l2_init"),
                                       (("--weight_decay", "4000"), "--weight_decay 4000")])
def test_run_refuses_the_ranges_before_the_device(argv, word):
    from simple_dqn_amd.main import run
    with pytest.raises(ValueError, match=word):
        run(_parse(*argv, "--random_steps", "0", "--train_steps", "0", "--test_steps", "0", "--epochs", "0"))


def test_everything_else_composes_on_the_command_line():
    from simple_dqn_amd.main import check_redo, check_regularizer, check_reset
    for argv in (("--dueling", "true"), ("--prioritized_replay", "true", "--n_step", "3"), ("--double_dqn", "true"), ("--datatype", "float16"),
                 ("--bootstrap_heads", "2"), ("--quantiles", "4"), ("--munchausen", "true"), ("--cql_alpha", "1"), ("--random_shift", "4"),
                 ("--clip_grad_norm", "10"), ("--target_tau", "0.01"), ("--advantage_learning", "0.9"), ("--optimizer", "adam"),
                 ("--redo_interval", "1000"), ("--reset_interval", "1000"), ("--target_steps", "0")):
        a = _parse("--weight_decay", "0.1", "--l2_init", "0.01", *argv)
        assert check_regularizer(a) == (0.1, 0.01, False) and check_redo(a)[0] in (0, 1000) and check_reset(a)[0] in (0, 1000)


def test_library_refuses_bad_arguments_without_a_device():
    import simple_dqn_amd as sd
    from simple_dqn_amd.deepqnetwork import regularize_apply_host
    err = (AssertionError, sd.SdqnError)
    theta = np.ones(64, np.float32)
    for wd, lam, lr, word in ((-0.1, 0.0, LR, "weight_decay"), (float("nan"), 0.0, LR, "weight_decay"), (0.0, -1.0, LR, "l2_init"),
                              (0.0, float("nan"), LR, "l2_init"), (100.0, 0.0, LR, "weight_decay"), (0.0, 100.5, LR, "l2_init"),
                              (0.1, 0.0, float("nan"), "weight_decay")):
        with pytest.raises(err, match=word):
            regularize_apply_host(wd, lam, lr, theta, theta.copy())
    with pytest.raises(err, match="anchor"):
        regularize_apply_host(0.0, 0.01, LR, theta, None)
    regularize_apply_host(0.0, 100.0, LR, theta, np.zeros(64, np.float32))      # lr x LAMBDA = 1: allowed, cf = 1: the anchor itself
    assert not bits(theta).any()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("sdqn_net_set_regularizer", "sdqn_net_get_regularizer", "sdqn_net_regularize_now", "sdqn_net_regularize_with", "sdqn_net_anchor_now",
           "sdqn_net_get_anchor", "sdqn_net_weight_norms", "sdqn_regularize_apply_host")


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


def test_entry_points_refuse_a_null_handle():
    import simple_dqn_amd as sd
    lib = sd.load()
    out = (C.c_double * 10)()
    assert lib.sdqn_net_set_regularizer(None, 0.1, 0.0) != 0 and lib.sdqn_net_regularize_now(None) != 0 and lib.sdqn_net_anchor_now(None) != 0
    assert lib.sdqn_net_weight_norms(None, out) != 0 and lib.sdqn_net_regularize_with(None, 0.1, 0.0) != 0


def test_option_table_still_lists_eleven_names():
    import simple_dqn_amd as sd
    lib = sd.load()
    names = []
    for k in range(64):
        s = lib.sdqn_option_name(k)
        if not s:
            break
        names.append(s.decode())
    assert len(names) == 11 and not any("decay" in n or "l2" in n for n in names)


# ---- the CSV ------------------------------------------------------------------------------------------------------------------------------
def test_csv_header_only_grows_when_asked(tmp_path):
    from simple_dqn_amd.statistics import COLUMNS, DORMANT_COLUMNS, WEIGHT_NORM_COLUMNS, Statistics

    class Stub:
        callback = None
    for kw, want in ((dict(), COLUMNS), (dict(weight_decay=0.1, l2_init=0.01), COLUMNS), (dict(log_weight_norms=False), COLUMNS),
                     (dict(log_weight_norms=True), COLUMNS + WEIGHT_NORM_COLUMNS),
                     (dict(log_weight_norms=True, log_dormant=True), COLUMNS + DORMANT_COLUMNS + WEIGHT_NORM_COLUMNS)):
        path = tmp_path / "s.csv"
        st = Statistics(Stub(), Stub(), None, None, make_args(csv_file=str(path), **kw))
        st.close()
        assert tuple(path.read_text().strip().split(",")) == want
    assert len(COLUMNS) == 16
    assert WEIGHT_NORM_COLUMNS == ("wnorm_1", "wnorm_2", "wnorm_3", "wnorm_4", "wnorm_5", "winit_1", "winit_2", "winit_3", "winit_4", "winit_5")
