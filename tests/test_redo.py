"""Dormant-neuron recycling (--redo_interval) without a device: the library's host restatement (csrc/redo.h through
sdqn_redo_apply_host / sdqn_redo_draw) against tests/redo_oracle.py, which works in the reference's weight layouts; the command line's
ranges and refusals; the C ABI's symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import redo_oracle as O
from util import make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD5678


def _random_net(A, rng):
    ws = [rng.standard_normal(s).astype(np.float32) for s in ((256, 32), (512, 64), (576, 64), (512, 3136), (A, 512))]
    st = [np.abs(rng.standard_normal(w.shape)).astype(np.float32) + np.float32(0.5) for w in ws]
    st2 = [rng.standard_normal(w.shape).astype(np.float32) for w in ws]
    return ws, st, st2


def _random_scores(rng, p=0.2):
    """scores around 1 with a fraction p below 0.1, some exactly 0; the first and last unit of every layer dormant"""
    s = rng.uniform(0.2, 2.0, 672).astype(np.float32)
    low = rng.rand(672) < p
    s[low] = rng.uniform(0.0, 0.1, int(low.sum())).astype(np.float32)
    s[rng.rand(672) < 0.05] = 0.0
    for l in range(4):
        s[O.EDGES[l]] = 0.0
        s[O.EDGES[l + 1] - 1] = 0.05
    return s


def _check_event(A, scores, tau, event, rng):
    from simple_dqn_amd.deepqnetwork import redo_apply_host
    ws, st, st2 = _random_net(A, rng)
    theta, state, state2 = O.to_internal(ws), O.to_internal(st), O.to_internal(st2)
    assert theta.size == O.OFFS[4] + 512 * A
    counts = redo_apply_host(scores, tau, SEED, event, A, theta, state, state2)
    want_w, (want_s, want_s2), masks = O.apply(scores, tau, SEED, event, ws, (st, st2))
    got_w, got_s, got_s2 = O.from_internal(theta, A), O.from_internal(state, A), O.from_internal(state2, A)
    assert [int(c) for c in counts] == [int(d.sum()) for d in O.dormant(scores, tau)]
    for l in range(5):
        red, zer = masks[l]["redrawn"], masks[l]["zeroed"]
        kept = ~(red | zer)
        # the three sets are exact: kept entries keep their bits, zeroed ones are +0.0, redrawn ones are the oracle's draws bit for bit
        assert np.array_equal(got_w[l].view(np.uint32)[kept], ws[l].view(np.uint32)[kept]), l
        assert not got_w[l].view(np.uint32)[zer].any(), l
        assert np.array_equal(got_w[l].view(np.uint32), want_w[l].view(np.uint32)), l
        if red.any():                                         # a draw is never the value it replaced (standard normals) and lies inside (-k, k)
            assert (got_w[l][red] != ws[l][red]).all() and (np.abs(got_w[l][red]) <= O.bound(l + 1)).all(), l
        for g, w, s0 in ((got_s, want_s, st), (got_s2, want_s2, st2)):
            assert np.array_equal(g[l].view(np.uint32), w[l].view(np.uint32)), l
            assert not g[l].view(np.uint32)[~kept].any() and np.array_equal(g[l][kept], s0[l][kept]), l
    return masks


@pytest.mark.parametrize("A", [1, 4, 18])
def test_host_restatement_matches_the_oracle(A):
    rng = np.random.RandomState(100 + A)
    scores = _random_scores(rng)
    masks = _check_event(A, scores, 0.1, 3, rng)
    # units dormant in two consecutive layers: the entry between them is zeroed, not redrawn
    d = O.dormant(scores, 0.1)
    assert d[0][0] and d[1][0] and masks[1]["zeroed"][0, 0] and not masks[1]["redrawn"][0, 0]
    assert d[2][63] and d[3][511] and masks[3]["zeroed"][511, 63 * 49] and not masks[3]["redrawn"][511, 63 * 49]
    assert masks[1]["redrawn"].any() and masks[3]["redrawn"].any() and masks[4]["zeroed"][:, 511].all() and not masks[4]["redrawn"].any()


def test_threshold_zero_selects_silent_units_only():
    rng = np.random.RandomState(7)
    scores = rng.uniform(1e-30, 2.0, 672).astype(np.float32)
    silent = [3, 40, 100, 671]
    scores[silent] = 0.0
    masks = _check_event(4, scores, 0.0, 1, rng)
    d = np.concatenate(O.dormant(scores, 0.0))
    assert sorted(np.nonzero(d)[0]) == silent
    assert masks[0]["redrawn"][:, 3].all() and masks[0]["redrawn"].sum() == 256


def test_layer_with_zero_mean_is_recycled_whole():
    acts = [np.abs(np.random.RandomState(l).standard_normal((40, n))).astype(np.float32) for l, n in enumerate(O.UNITS)]
    acts[1][:] = 0.0
    s = O.scores(acts)
    assert not s[32:96].any() and (s[:32] > 0).all()
    assert abs(float(s[:32].astype(np.float64).mean()) - 1.0) < 1e-6
    rng = np.random.RandomState(9)
    masks = _check_event(4, s, 0.0, 2, rng)
    assert masks[1]["redrawn"].all() and masks[2]["zeroed"].all() and not masks[0]["redrawn"].any() and not masks[3]["zeroed"].any()


def test_draw_bits_against_big_integers():
    from simple_dqn_amd.deepqnetwork import redo_draw
    # splitmix64 itself: the published first outputs of seed 0 (state advanced by G, then mixed)
    assert O.mix(O.G) == 0xE220A8397B1DCDAF and O.mix(2 * O.G) == 0x6E789E6AA1B965F4
    cases = [(0, 0, 0, 1), (SEED, 1, 0, 1), (SEED, 1, 8191, 1), (SEED, 2, 8192, 2), (2 ** 64 - 1, 7, 40960, 3), (SEED, 2 ** 40, 77824, 4),
             (5, 3, 1683455, 4)]
    for seed, event, index, layer in cases:
        w, v = redo_draw(seed, event, index, layer)
        ow, ov = O.draw(seed, event, index, layer)
        assert w == ow, (seed, event, index)
        assert np.float32(v).view(np.uint32) == np.float32(ov).view(np.uint32), (seed, event, index)
        u = ow >> 40
        assert float(ov) == float(np.float32((2.0 * u / 2 ** 24 - 1.0)) * O.bound(layer))
        assert np.array_equal(O.draws(seed, event, [index], layer).view(np.uint32), np.array([ov]).view(np.uint32))
    # the bounds are float32(sqrt(3 / fan_in)) and u = 0 / 2^24 - 1 reach the ends of [-k, k)
    assert [float(O.bound(l)) for l in (1, 2, 3, 4)] == [float(np.float32(np.sqrt(3.0 / f))) for f in (256, 512, 576, 3136)]
    idx = np.arange(200000)
    x = O.draws(SEED, 1, idx, 1)
    assert x.min() >= -O.bound(1) and x.max() < O.bound(1) and abs(float(x.mean())) < 1e-3


def test_host_restatement_refuses_bad_arguments():
    import simple_dqn_amd as sd
    from simple_dqn_amd.deepqnetwork import redo_apply_host, redo_draw
    theta = np.zeros(O.OFFS[4] + 512 * 4, np.float32)
    with pytest.raises((AssertionError, sd.SdqnError)):
        redo_apply_host(np.zeros(672, np.float32), 1.0, 0, 1, 4, theta)
    with pytest.raises((AssertionError, sd.SdqnError)):
        redo_apply_host(np.zeros(672, np.float32), 0.1, 0, 1, 19, np.zeros(O.OFFS[4] + 512 * 19, np.float32))
    with pytest.raises((AssertionError, sd.SdqnError)):
        redo_draw(0, 1, 0, 5)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from simple_dqn_amd.main import build_parser
    return build_parser().parse_args(list(argv))


def test_flags_and_their_ranges():
    from simple_dqn_amd.main import check_redo
    a = _parse()
    assert (a.redo_interval, a.redo_threshold, a.log_dormant) == (0, 0.1, False)
    assert check_redo(a) == (0, 0.1, False)
    assert check_redo(_parse("--redo_interval", "1000", "--redo_threshold", "0", "--log_dormant", "true")) == (1000, 0.0, True)
    assert check_redo(make_args()) == (0, 0.1, False)                     # a namespace without the flags: off
    for argv, word in ((("--redo_interval", "-1"), "--redo_interval -1"), (("--redo_threshold", "1"), "--redo_threshold 1"),
                       (("--redo_threshold", "-0.5"), "--redo_threshold"), (("--redo_threshold", "nan"), "--redo_threshold")):
        with pytest.raises(ValueError, match=word):
            check_redo(_parse(*argv))


REFUSED = [(("--batch_norm", "true"), "--batch_norm"), (("--noisy_nets", "true"), "--noisy_nets"), (("--datatype", "float64"), "float64"),
           (("--screen_height", "42", "--screen_width", "42"), "84 x 84"), (("--history_length", "2"), "84 x 84")]


@pytest.mark.parametrize("ours", [("--redo_interval", "5"), ("--log_dormant", "true")])
@pytest.mark.parametrize("other,word", REFUSED)
def test_refusals_in_both_orders_before_the_device(ours, other, word):
    from simple_dqn_amd.main import run
    for argv in (ours + other, other + ours):
        with pytest.raises(ValueError, match=word) as e:                   # (this box has no device: touching one raises something else)
            run(_parse(*argv, "--random_steps", "0", "--train_steps", "0", "--test_steps", "0", "--epochs", "0"))
        assert ours[0] in str(e.value)


def test_everything_else_composes_on_the_command_line():
    from simple_dqn_amd.main import check_redo
    for argv in (("--dueling", "true"), ("--prioritized_replay", "true", "--n_step", "3"), ("--double_dqn", "true"), ("--datatype", "float16"),
                 ("--bootstrap_heads", "2"), ("--quantiles", "4"), ("--munchausen", "true"), ("--cql_alpha", "1"), ("--random_shift", "4"),
                 ("--clip_grad_norm", "10"), ("--target_tau", "0.01"), ("--advantage_learning", "0.9"), ("--optimizer", "adam")):
        assert check_redo(_parse("--redo_interval", "10", "--log_dormant", "true", *argv))[0] == 10


def test_csv_header_only_grows_when_asked(tmp_path):
    from simple_dqn_amd.statistics import COLUMNS, DORMANT_COLUMNS, Statistics

    class Stub:
        callback = None
    for kw, want in ((dict(), COLUMNS), (dict(redo_interval=0, log_dormant=False), COLUMNS), (dict(redo_interval=10), COLUMNS + DORMANT_COLUMNS),
                     (dict(log_dormant=True), COLUMNS + DORMANT_COLUMNS)):
        path = tmp_path / "s.csv"
        st = Statistics(Stub(), Stub(), None, None, make_args(csv_file=str(path), **kw))
        st.close()
        assert tuple(path.read_text().strip().split(",")) == want
    assert len(COLUMNS) == 16 and DORMANT_COLUMNS == ("dormant_1", "dormant_2", "dormant_3", "dormant_4")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("sdqn_net_set_redo", "sdqn_net_get_redo", "sdqn_net_redo_now", "sdqn_net_redo_scores", "sdqn_net_redo_last", "sdqn_redo_apply_host",
           "sdqn_redo_draw")


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
    out = (C.c_float * 672)()
    assert lib.sdqn_net_set_redo(None, 3, 0.1, 0) != 0 and lib.sdqn_net_redo_now(None) != 0 and lib.sdqn_net_redo_scores(None, out) != 0
