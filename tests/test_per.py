"""--prioritized_replay on the CPU: the command line, the β schedule and the numpy restatement (tests/per_oracle.py)."""
import random

import numpy as np

import per_oracle as P


def test_parser_defaults_and_flags():
    from simple_dqn_amd import main as M
    a = M.build_parser().parse_args([])
    assert a.prioritized_replay is False
    assert (a.priority_alpha, a.priority_beta, a.priority_beta_steps, a.priority_epsilon) == (0.6, 0.4, 1000000, 1e-6)
    b = M.build_parser().parse_args(["--prioritized_replay", "true", "--priority_alpha", "0.5", "--priority_beta", "0.3",
                                     "--priority_beta_steps", "100", "--priority_epsilon", "0.01"])
    assert b.prioritized_replay is True
    assert (b.priority_alpha, b.priority_beta, b.priority_beta_steps, b.priority_epsilon) == (0.5, 0.3, 100, 0.01)


def test_beta_schedule():
    from simple_dqn_amd.agent import priority_beta
    assert priority_beta(0.4, 1000, 0) == 0.4
    assert abs(priority_beta(0.4, 1000, 500) - 0.7) < 1e-15
    assert priority_beta(0.4, 1000, 1000) == 1.0
    assert priority_beta(0.4, 1000, 10 ** 7) == 1.0
    assert priority_beta(0.4, 0, 0) == 1.0


def _ring(rng, size, p_term):
    return rng.rand(size) < p_term


def test_validity_mask_equals_reference_rule():
    rng = np.random.RandomState(0)
    for trial in range(60):
        size = int(rng.randint(8, 200))
        hist = int(rng.randint(1, 5))
        term = _ring(rng, size, [0.0, 0.05, 0.3][trial % 3])
        count = int(rng.randint(hist + 1, size + 1)) if trial % 2 else size      # count < size, and full rings
        current = int(rng.randint(0, size)) if count == size else count % size    # full: wrapped, current anywhere
        m = P.valid_mask(term, count, current, hist, size)
        ref = np.array([P.accepts(i, term, count, current, hist) for i in range(size)])
        assert np.array_equal(m, ref), (trial, size, hist, count, current)


def test_reference_rejection_sampler_only_returns_valid_indexes():
    """the reference's loop (replay_memory.py:54-68) on Python's random: every index it returns is in the mask, and every index of the
    mask is reachable"""
    rng = np.random.RandomState(1)
    size, hist = 120, 4
    term = _ring(rng, size, 0.05)
    count, current = size, 50
    mask = P.valid_mask(term, count, current, hist, size)
    r = random.Random(3)
    seen = set()
    for _ in range(4000):
        while True:
            i = r.randint(hist, count - 1)
            if i >= current and i - hist < current:
                continue
            if term[i - hist:i].any():
                continue
            break
        assert mask[i]
        seen.add(i)
    assert seen == set(np.nonzero(mask)[0])


def _inverse_cdf(leaf, t):
    c = np.cumsum(np.asarray(leaf, dtype=np.float64))
    return np.searchsorted(c, t, side="right")


def test_stratified_sampler_equals_inverse_cdf():
    rng = np.random.RandomState(2)
    for size in (50, 64, 600, 5000, 300000):
        leaf = rng.randint(0, 9, size).astype(np.float32)           # integers: every sum exact in fp32 / fp64
        leaf[rng.rand(size) < 0.2] = 0
        u = rng.rand(32)
        idx = P.sample(leaf, u)
        S = float(leaf.astype(np.float64).sum())
        assert P.SumTree(leaf).total == S
        t = np.array([(n + u[n]) * S / 32 for n in range(32)])
        assert np.array_equal(idx, _inverse_cdf(leaf, t)), size
        assert (leaf[idx] > 0).all()


def test_sampler_never_returns_zero_leaf_at_right_edge():
    leaf = np.zeros(700, np.float32)
    leaf[[3, 100, 640]] = [1.0, 2.0, 0.5]
    tree = P.SumTree(leaf)
    idx = tree.descend(np.array([tree.total, tree.total * 1.0000001, 0.0, 2.999999]))
    assert list(idx) == [640, 640, 3, 100]


def test_tree_levels_are_folds():
    rng = np.random.RandomState(4)
    leaf = rng.rand(64 * 64 * 3 + 17).astype(np.float32)
    tree = P.SumTree(leaf)
    assert [len(x) for x in tree.levels] == [len(leaf), 193, 4]
    assert tree.levels[1][5] == P.fold(leaf[320:384].astype(np.float64))
    assert abs(tree.total - leaf.astype(np.float64).sum()) < 1e-9 * tree.total


def test_weights_and_priorities():
    w = P.weights([4.0, 1.0, 2.0], 0.5)
    assert np.allclose(w, [0.5, 1.0, 2 ** -0.5])
    assert P.weights([4.0, 1.0], 0.0).tolist() == [1.0, 1.0]
    assert P.new_priority([0.0, 3.0], 0.6, 1e-6)[1] == np.float32((3.0 + 1e-6) ** 0.6)
    raw = np.ones(5, np.float32); leaf = raw.copy(); valid = np.array([1, 1, 0, 1, 1], bool)
    P.write_back(raw, leaf, valid, [1, 2, 1], np.float32([5, 6, 7]))
    assert raw.tolist() == [1, 7, 6, 1, 1] and leaf.tolist() == [1, 7, 0, 1, 1]


def test_oracle_weights_the_clipped_delta():
    from oracle.dqn_numpy import OracleDQN, xavier_weights
    A, B = 4, 6
    kw = dict(batch_size=B, history_length=2, screen_height=36, screen_width=36, dtype=np.float64)
    ws = xavier_weights(A, 3, np.float64, 2, 36, 36)
    rng = np.random.RandomState(5)
    mb = (rng.randint(0, 256, (B, 2, 36, 36), dtype=np.uint8), rng.randint(0, A, B).astype(np.uint8),
          rng.randint(-2, 3, B).astype(np.int64), rng.randint(0, 256, (B, 2, 36, 36), dtype=np.uint8), rng.rand(B) < 0.2)
    std = OracleDQN(A, weights=ws, **kw)
    per = P.PEROracle(A, weights=ws, **kw)
    g0, c0, d0, _ = std.gradients(mb)
    g1, c1, d1, _ = per.gradients(mb)                 # no weights: the standard step
    assert abs(c0 - c1) < 1e-12 and np.abs(d0 - d1).max() < 1e-12
    per.weights = np.linspace(0.2, 1.0, B)
    g2, c2, d2, _ = per.gradients(mb)
    assert np.abs(d2 - d0 * per.weights[:, None]).max() < 1e-12
    assert np.abs(g2[4] - (d0 * per.weights[:, None]).T @ np.asarray(per.fprop(per.W, per._normalize(mb[0]), keep=True)[1][3])).max() < 1e-9
    assert c2 < c0
