"""--noisy_nets without a device: the noise restated exactly, its distribution, the command line and the weight files."""
import numpy as np
import pytest

import noisy_oracle as N
from simple_dqn_amd import deepqnetwork as D
from simple_dqn_amd.main import build_parser, run

SEED = 123            # make_args' --random_seed: the stream every default test net draws from


def test_words_are_the_integer_mix_exactly():
    for seed, step, slot, layer, side in [(0, 0, 0, 0, 0), (SEED, 1, 1, 0, 1), (2 ** 64 - 1, 2 ** 40 + 3, 0, 1, 0), (7, 5, 1, 1, 1)]:
        got = D.noisy_words(seed, step, slot, layer, side, 300)
        assert got.dtype == np.uint64 and np.array_equal(got, N.words(seed, step, slot, layer, side, 300)), (seed, step, slot, layer, side)


def test_normals_follow_their_words():
    """z against the numpy float32 restatement on the same words: a few ulps of logf / cosf on r <= 6.66 (1e-5 absolute, as on the device)"""
    w = D.noisy_words(SEED, 4, 0, 0, 0, N.IN4)
    z = D.noisy_noise(SEED, 4, 0, 0, 0, N.IN4)
    assert z.dtype == np.float32 and np.isfinite(z).all()
    assert np.abs(z - N.normal(w)).max() < 1e-5
    hi, lo = (w >> np.uint64(32)).astype(np.float64), (w & np.uint64(0xFFFFFFFF)).astype(np.float64)
    z64 = np.sqrt(-2.0 * np.log((hi + 1.0) / 2.0 ** 32)) * np.cos(2.0 * np.pi * lo / 2.0 ** 32)
    assert np.abs(z - z64).max() < 1e-5


def test_distribution_of_the_fc4_vectors_over_64_steps():
    zi = {0: [], 1: []}
    pooled = {0: [], 1: []}
    for step in range(64):
        for slot in (0, 1):
            a, b = D.noisy_noise(SEED, step, slot, 0, 0, N.IN4), D.noisy_noise(SEED, step, slot, 0, 1, N.OUT4)
            zi[slot].append(a)
            pooled[slot] += [a, b]
    for slot in (0, 1):
        z = np.concatenate(pooled[slot]).astype(np.float64)
        assert z.size == 233472
        print("slot %d: mean %.5f var %.5f" % (slot, z.mean(), z.var()))
        assert abs(z.mean()) < 0.01                 # 5 standard errors
        assert abs(z.var() - 1.0) < 0.02            # about 6.8 standard errors
    x, y = np.concatenate(zi[0]).astype(np.float64), np.concatenate(zi[1]).astype(np.float64)
    r = float(np.corrcoef(x, y)[0, 1])
    print("online / target correlation over %d pairs: %.5f" % (x.size, r))
    assert x.size == 200704 and abs(r) < 0.02


def test_no_two_streams_are_equal():
    seen = {}
    for step in range(4):
        for slot in (0, 1):
            for layer in (0, 1):
                for side in (0, 1):
                    w = D.noisy_words(SEED, step, slot, layer, side, 16).tobytes()
                    assert w not in seen, ((step, slot, layer, side), seen.get(w))
                    seen[w] = (step, slot, layer, side)
    assert len(seen) == 32


def test_factor_is_sgn_sqrt_abs():
    z = np.array([-4.0, -0.25, 0.0, 0.25, 9.0], np.float32)
    assert np.array_equal(N.factor(z), np.array([-2.0, -0.5, 0.0, 0.5, 3.0], np.float32))


def test_flags_parse():
    a = build_parser().parse_args([])
    assert a.noisy_nets is False and a.noisy_sigma == 0.5
    a = build_parser().parse_args(["--noisy_nets", "true", "--noisy_sigma", "0.25"])
    assert a.noisy_nets is True and a.noisy_sigma == 0.25


REFUSED = [(["--datatype", "float16"], "--datatype float16"), (["--datatype", "float64"], "--datatype float64"),
           (["--screen_height", "42", "--screen_width", "42"], "--screen_height 42"), (["--history_length", "2"], "--history_length 2"),
           (["--batch_norm", "true"], "--batch_norm"), (["--clip_grad_norm", "10"], "--clip_grad_norm"),
           (["--target_tau", "0.01"], "--target_tau"), (["--munchausen", "true"], "--munchausen"),
           (["--advantage_learning", "0.9"], "--advantage_learning"), (["--bootstrap_heads", "2"], "--bootstrap_heads 2"),
           (["--quantiles", "3"], "--quantiles 3"), (["--dueling", "true"], "--dueling"), (["--noisy_sigma", "-1"], "--noisy_sigma"),
           (["--noisy_sigma", "nan"], "--noisy_sigma")]


@pytest.mark.parametrize("extra,named", REFUSED, ids=[" ".join(e) for e, _ in REFUSED])
def test_run_refuses_by_name_before_touching_a_device(extra, named):
    args = build_parser().parse_args(["--noisy_nets", "true", "--environment", "catch"] + extra)
    with pytest.raises(ValueError) as e:
        run(args)
    assert "--noisy_nets" in str(e.value) or "--noisy_sigma" in str(e.value)
    assert named in str(e.value)


def test_flag_off_refuses_nothing():
    args = build_parser().parse_args(["--noisy_sigma", "-1", "--clip_grad_norm", "10"])
    assert D.check_noisy(args) == (False, -1.0)


class _FileNet(D.DeepQNetwork):
    """save_weights / load_weights over host arrays: what the .npz carries, without a device"""

    def __init__(self, noisy, A=4, fill=0.0):
        self.noisy_nets, self.batch_norm, self.optimizer, self.train_iterations = noisy, False, "rmsprop", 7
        self._h, self._lib = None, None
        self._shapes = D.layer_shapes(A, 4, 84, 84)
        self.layers = dict(((w, i), np.full(s, fill + w + 0.1 * i, np.float32)) for w in (0, 1, 2) for i, s in enumerate(self._shapes))
        self.sig = dict((w, [np.full(self._shapes[3], 0.5 / 56.0, np.float32), np.full(self._shapes[4], 0.5 / np.sqrt(512.0), np.float32)]) for w in (0, 1))

    def get_layer(self, layer, which=0):
        return self.layers[(which, layer)].copy()

    def set_layer(self, layer, w, which=0):
        self.layers[(which, layer)] = np.array(w, np.float32)

    def get_noisy_sigma(self, which=0):
        return [s.copy() for s in self.sig[which]]

    def set_noisy_sigma(self, sigmas, which=0):
        self.sig[which] = [np.array(s, np.float32) for s in sigmas]


def test_npz_round_trip_of_sigma(tmp_path):
    rng = np.random.RandomState(5)
    a = _FileNet(True)
    for w in (0, 1):
        a.sig[w] = [rng.rand(*s.shape).astype(np.float32) for s in a.sig[w]]
    p = str(tmp_path / "noisy.npz")
    a.save_weights(p)
    with np.load(p) as f:
        assert set(("NS3", "NS4", "NSt3", "NSt4", "W3", "Wt4", "S0", "train_iterations")) <= set(f.keys())
    b = _FileNet(True, fill=9.0)
    b.load_weights(p)
    for w in (0, 1):
        for x, y in zip(a.sig[w], b.sig[w]):
            assert np.array_equal(x, y)
        for i in range(5):
            assert np.array_equal(a.layers[(w, i)], b.layers[(w, i)])
    assert b.train_iterations == 7


def test_plain_file_loads_into_a_noisy_net_with_the_init_sigma(tmp_path):
    p = str(tmp_path / "plain.npz")
    _FileNet(False, fill=3.0).save_weights(p)
    with np.load(p) as f:
        assert not any(k.startswith("NS") for k in f.keys())
    b = _FileNet(True)
    init = [s.copy() for s in b.sig[0]]
    b.load_weights(p)
    assert np.array_equal(b.layers[(0, 3)], np.full(b._shapes[3], 3.3, np.float32))
    for w in (0, 1):
        for x, y in zip(init, b.sig[w]):
            assert np.array_equal(x, y)


def test_noisy_file_is_refused_by_a_plain_net_by_name(tmp_path):
    p = str(tmp_path / "noisy.npz")
    _FileNet(True).save_weights(p)
    with pytest.raises(ValueError) as e:
        _FileNet(False).load_weights(p)
    assert "--noisy_nets" in str(e.value) and "NS3" in str(e.value)
