"""Batch sizes above 256 and the first batch size on the far side of every dispatch edge, on the tuned path (84 x 84 x 4, float32 / float16),
through the interfaces the other GPU files use (train, last_q, get_layer(i, which=3), train_from_memory, getMinibatch, predict).

Above B = 256 the library runs code no other test reaches: the pinned-slot gather (gather_kernel<false>), the second trip of the loops
that stride by 256 (prep_kernel, the prep riding in the update launch, the cost_sh fill), the sample-stationary chain in more than one
round of the chip (float32 train at B = 512; --double_dqn B = 257: 387 workgroups, one with a single odd sample), the float16 chains past
256 workgroups and the larger split-K slab counts.  Below it: B = 33 (prep_inline and conv1's in-kernarg indexes stop, fc4_wgrad moves
into bwd3 with a one-row second chunk), 65 / 97 / 127 (Fc4Wgrad<2> / <4> in the unfused structure, the largest ragged batch of the latency
engine), float16 47 / 48 (the exact-byte conv1 launch of its own starts at 48 where something asks for one).

Three instruments:
  1. one whole step against the float64 oracle (float16: the half oracle) at the bounds the existing one-step tests use;
  2. position invariance — the same minibatch in another order must give the same Q rows and, up to summation round-off, the same
     gradients: a sample handled by its POSITION instead of its content fails it, and Rectlin gate flips (which blunt instrument 1 to
     1e-2 at B >= 128) cancel because the same kernel computes each sample's activations in both runs;
  3. the ring paths (getMinibatch, train_from_memory, --double_dqn, the prioritized-replay refusal) above 256.

CPU-side figures behind the constants below (numpy oracle, this file's seeds):
  * every random_minibatch(B, A, seed, reward_range=(-3, 4)) used holds a terminal (float32 B = 32: 8, 33: 6, 65: 15, 97: 20, 127: 24,
    256: 42, 257: 48, 320: 61, 512: 92; float16 33: 8, 47: 6, 48: 11, 127: 35, 257: 48, 320: 65; --double_dqn 257: 48; asserted again
    in the tests);
  * reorder noise r of the oracle itself — largest per-layer relative Frobenius norm of gradients(mb) - gradients(mb[perm]) over the roll
    and the random permutation.  fp32 oracle: B = 32 2.7e-7, 127 4.9e-7, 256 5.7e-7, 257 5.9e-7 (--double_dqn 6.0e-7), 320 5.0e-7,
    512 6.36e-7.  half oracle: B = 127 4.8e-7, 257 5.06e-7, 320 4.7e-7.  (Its Q rows are bit-identical under both permutations.)
  * the synthetic_fill ring of 5000 slots has 4857 / 4854 indexes the n = 1 / n = 3 sampler accepts; seeds 11, 12, 13 draw 320 indexes
    with 331 / 330 / 328 draws (both n): the rejection sampler is nowhere near exhausting it.
"""
import random

import numpy as np
import pytest

import nstep_oracle as N
from double_dqn_oracle import DoubleDQNOracle
from oracle.dqn_numpy import OracleDQN, xavier_weights
from oracle.replay_numpy import MT19937, ReplayOracle, synthetic_fill
from util import make_args, random_minibatch

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4          # tests/test_gpu_dqn.py
H_TOL = 3e-3          # tests/test_gpu_dqn.py, float16 mode
GAMMA, MINR, MAXR = 0.99, -1.0, 1.0

# name: (datatype, B, A, fused_launches, double_dqn)
CONFIGS = {}
for _B, _A in ((33, 4), (65, 6), (97, 3), (127, 18), (257, 18), (320, 3), (512, 6)):
    CONFIGS["fp32_b%d" % _B] = ("float32", _B, _A, 1, False)
for _B, _A in ((65, 6), (97, 3)):
    CONFIGS["fp32_b%d_unfused" % _B] = ("float32", _B, _A, 0, False)                  # Fc4Wgrad<2> / <4> at a ragged K
for _B, _A in ((33, 6), (47, 3), (48, 4), (127, 18), (257, 4), (320, 18)):
    CONFIGS["fp16_b%d" % _B] = ("float16", _B, _A, 1, False)
PART1 = list(CONFIGS)
CONFIGS["fp32_b32"] = ("float32", 32, 4, 1, False)                                   # controls of the position-invariance check:
CONFIGS["fp32_b256"] = ("float32", 256, 3, 1, False)                                 # sizes the rest of the suite already trusts
CONFIGS["ddqn_b257"] = ("float32", 257, 4, 1, True)                                  # nz = 3: 387 sample-stationary workgroups
PART2 = [n for n in PART1 if CONFIGS[n][1] >= 127] + ["fp32_b256", "fp32_b32", "ddqn_b257"]

# Position invariance bound P = max(32 r, 1e-5), r = the oracle's own reorder noise (module docstring; the factor 32 allows for the
# device's split-K slab order differing from BLAS's).  Ceiling: one sample handled by position moves a layer's gradient by ~1 / sqrt(B)
# of its norm, 4.4e-2 at B = 512 — P is 2 000 x under it.
R_NOISE = {"float32": 6.36e-7, "float16": 5.06e-7}
P_BOUND = {dt: max(32 * r, 1e-5) for dt, r in R_NOISE.items()}                       # 2.04e-5 / 1.62e-5
assert all(p <= 1e-3 for p in P_BOUND.values())
# configurations whose Q rows are NOT bit-identical under a permutation may fall back to the 1e-2 of part 1 (gates may flip between the
# two runs): name -> measured value.  None on MI355X: where the rows are not bit-identical (the sample-stationary chain: fp32_b256,
# fp32_b512, ddqn_b257 — they agree to 1e-6 of max |q|) the gradients still stay within P (at most 4.9e-7).
P_FALLBACK = {}


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _seed(name):
    dt, B, _, _, double = CONFIGS[name]
    return 1000 + B + (50 if dt == "float16" else 0) + (9 if double else 0)


def _minibatch(name):
    _, B, A, _, _ = CONFIGS[name]
    mb = random_minibatch(B, A, _seed(name), reward_range=(-3, 4))
    assert mb[4].any() and not mb[4].all()
    return mb


def _weights(name):
    A, s = CONFIGS[name][2], _seed(name)
    return xavier_weights(A, s), xavier_weights(A, s + 1)


def _net(sd, name):
    dt, B, A, fused, double = CONFIGS[name]
    net = sd.DeepQNetwork(A, make_args(batch_size=B, datatype=dt, double_dqn=double))
    ws, wt = _weights(name)
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    net.set_option("keep_gradients", 1)
    if not fused:
        net.set_option("fused_launches", 0)
    return net


class _Capture:
    """keeps the bootstrap values the step used (last_maxpostq)"""
    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        self.last_maxpostq = np.array(maxpostq)
        return super().td_targets(preq, maxpostq, actions, rewards, terminals)


class _Oracle(_Capture, OracleDQN):
    pass


def _oracle(name):
    """float32 nets: the float64 oracle; float16 nets: the half oracle (fp32 accumulation), as tests/test_gpu_dqn.py.  conv1's input form
    in half mode is OracleDQN's default (exact_conv1_input=None) on BOTH sides of B = 48: conv1 rides in front of the float16 forward chain
    at every batch size (conv_ssh.h), so the exact-byte form applies at 47 as at 48 — what starts at 48 is only the exact-byte conv1 launch
    of its own, which the default options never take."""
    dt, B, A, _, double = CONFIGS[name]
    ws, wt = _weights(name)
    if dt == "float16":
        o = _Oracle(A, batch_size=B, weights=ws, half_activations=True)
        o.Wt = [w.copy() for w in wt]
    else:
        o = (DoubleDQNOracle if double else _Oracle)(A, batch_size=B, dtype=np.float64, weights=[w.astype(np.float64) for w in ws])
        o.Wt = [w.astype(np.float64) for w in wt]
    return o


_steps = {}


def _device_step(sd, name, perm=None, state=False):
    """one train step of a fresh net on the configuration's minibatch (rows reordered by perm): Q, max-Q, cost, the five gradients
    [, weights and RMSProp state].  The unpermuted step is run once and shared by parts 1 and 2."""
    if perm is None and name in _steps:
        return _steps[name]
    mb = _minibatch(name)
    if perm is not None:
        mb = tuple(np.ascontiguousarray(x[perm]) for x in mb)
    net = _net(sd, name)
    costs = []
    net.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
    net.train(mb)
    q, mq = net.last_q()
    out = dict(q=q, mq=mq, cost=costs[0], g=[np.array(net.get_layer(i, which=3)) for i in range(5)])
    if state:
        out["W"] = [np.array(net.get_layer(i, 0)) for i in range(5)]
        out["S"] = [np.array(net.get_layer(i, 2)) for i in range(5)]
    assert net.train_iterations == 1
    if perm is None:
        _steps[name] = out
    return out


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(1e-12, np.linalg.norm(b)))


def _check_step(name, dev, o, g, cost, preq):
    """the comparisons of part 1, at the bounds the existing one-step tests hold their regimes to"""
    dt, B, A, _, _ = CONFIGS[name]
    half = dt == "float16"
    qtol = H_TOL if half else Q_TOL
    assert dev["q"].shape == (B, A)
    eq, em = np.abs(dev["q"] - preq).max(), np.abs(dev["mq"] - o.last_maxpostq).max()
    ec = abs(dev["cost"] - float(cost)) / max(1.0, float(cost))
    print("%s: Q max abs err %.3e, max-Q %.3e, cost rel err %.3e" % (name, eq, em, ec))
    assert eq < qtol and em < qtol
    assert ec < (5e-3 if half else 1e-5)
    for i in range(5):
        mx, fro = np.abs(dev["g"][i] - g[i]).max(), _rel(dev["g"][i], g[i])
        print("%s layer %d: grad max abs err %.3e (max |g| %.3e), rel norm %.3e" % (name, i, mx, np.abs(g[i]).max(), fro))
        if half:
            assert fro < 5e-2, i                                       # test_fp16_one_step_gradients
        elif B >= 128:
            assert fro < 1e-2, i                                       # _check_grads of tests/test_gpu_nstep.py
        else:
            assert mx < 1e-4 * max(1e-3, np.abs(g[i]).max()), i        # test_one_step_gradients_and_update


@pytest.mark.parametrize("name", PART1)
def test_one_step_against_the_oracle(sd, name):
    """Part 1.  Q and max-Q of every row, the cost, the five gradients and — float32 below B = 128, where the element bounds of
    test_one_step_gradients_and_update apply — the weights and the RMSProp state after the update."""
    dt, B, A, _, _ = CONFIGS[name]
    small32 = dt == "float32" and B < 128
    o = _oracle(name)
    g, cost, _, preq = o.gradients(_minibatch(name))
    dev = _device_step(sd, name, state=small32)
    _check_step(name, dev, o, g, cost, preq)
    if small32:
        o.rmsprop(g, B)
        for i in range(5):
            big = np.abs(g[i]) / B > 1e-6
            assert np.abs(dev["W"][i] - o.W[i])[big].max() < 2e-5, "weights layer %d" % i
            assert np.abs(dev["S"][i] - o.S[i]).max() < 1e-6 + 1e-3 * np.abs(o.S[i]).max(), "state layer %d" % i


@pytest.mark.parametrize("name", ["fp32_b257", "fp32_b512"])
def test_predict_rows_of_zeros(sd, name):
    """The padding property of test_predict_parity above 256: rows of zeros come back exactly 0 (no biases), row 0 within 1e-4 of the
    oracle.  predict at B = 512 is nz = 1 on the sample-stationary chain in exactly one round (256 two-sample workgroups)."""
    _, B, A, _, _ = CONFIGS[name]
    net = _net(sd, name)
    st = _minibatch(name)[0].copy()
    st[1:] = 0
    q = net.predict(st)
    o1 = OracleDQN(A, batch_size=1, dtype=np.float64, weights=[w.astype(np.float64) for w in _weights(name)[0]])
    assert q.shape == (B, A) and np.all(q[1:] == 0)
    assert np.abs(q[0] - o1.predict(st[:1])[0]).max() < Q_TOL


def _perms(name):
    """roll by one; a fixed random permutation, repaired so that every sample with index >= 256 lands below 256"""
    B, p = CONFIGS[name][1], np.random.RandomState(_seed(name)).permutation(CONFIGS[name][1])
    if B > 256:
        lo = [k for k in range(256) if p[k] < 256]
        for k, j in zip([k for k in range(256, B) if p[k] >= 256], lo):
            p[k], p[j] = p[j], p[k]
        assert (p[256:] < 256).all()
    assert sorted(p) == list(range(B))
    return {"roll": np.roll(np.arange(B), 1), "perm": p}


def _invariance(sd, name, which):
    """(bit-identical Q rows?, largest per-layer relative norm of the gradient difference) of the step on mb[perm] against the step on mb"""
    perm = _perms(name)[which]
    base, twin = _device_step(sd, name), _device_step(sd, name, perm=perm)
    q, qp = base["q"], twin["q"]
    assert np.abs(qp - q[perm]).max() <= 1e-6 * max(1.0, float(np.abs(q).max()))
    assert np.abs(twin["mq"] - base["mq"][perm]).max() <= 1e-6 * max(1.0, float(np.abs(base["mq"]).max()))
    bits = bool(np.array_equal(qp, q[perm]) and np.array_equal(twin["mq"], base["mq"][perm]))
    rels = [_rel(twin["g"][i], base["g"][i]) for i in range(5)]
    print("%s %s: Q rows bit-identical: %s; gradient rel norm of the difference per layer %s (P = %.3e)" % (
        name, which, bits, " ".join("%.3e" % r for r in rels), P_BOUND[CONFIGS[name][0]]))
    return bits, rels


@pytest.mark.parametrize("which", ["roll", "perm"])
@pytest.mark.parametrize("name", PART2)
def test_position_invariance(sd, name, which):
    """Part 2.  A twin net trained on the minibatch permuted along the batch axis: Q rows equal q[perm] (1e-6 of max |q|; whether they
    are bit-identical is printed), every layer's gradient within P = max(32 r, 1e-5) in relative Frobenius norm — r = 6.36e-7 (fp32
    oracle) / 5.06e-7 (half oracle) is the reference's own reorder noise, so P = 2.04e-5 / 1.62e-5; handling one sample by position would
    move a gradient by ~1 / sqrt(B) >= 4.4e-2.  Measured on MI355X, largest layer over both permutations: float32 B = 32 1.9e-7, 127
    2.3e-7, 256 4.3e-7, 257 3.8e-7, 320 3.7e-7, 512 4.9e-7, --double_dqn 257 4.6e-7; float16 127 1.6e-7, 257 1.8e-7, 320 2.1e-7 — the
    device reorders no more noisily than numpy.  Q rows are bit-identical except on the sample-stationary chain (float32 B = 256, 512,
    --double_dqn 257), where they agree to 1e-6 of max |q|; no configuration needed the fallback (P_FALLBACK is empty)."""
    bits, rels = _invariance(sd, name, which)
    bound = P_BOUND[CONFIGS[name][0]]
    if not bits and name in P_FALLBACK:
        bound = 1e-2
    for i in range(5):
        assert rels[i] < bound, (i, rels[i])


# ---- part 3: the ring paths above 256 ----------------------------------------------------------------------------------------------------
SIZE = 5000


def _mems(sd, dt, B, n, A=4, seed=3):
    mem = sd.ReplayMemory(SIZE, make_args(batch_size=B, datatype=dt, n_step=n))
    om = ReplayOracle(SIZE, batch_size=B)
    synthetic_fill(mem, seed, num_actions=A)
    synthetic_fill(om, seed, num_actions=A)
    mem.sync_mirror()
    return mem, om


def _expected_gather(om, idx, n):
    if n == 1:
        return om.gather(idx)
    return N.gather(om, idx, n, GAMMA, MINR, MAXR)


def _compare_gather(mb, exp, n):
    pre, act, rew, post, term = mb
    assert np.array_equal(np.asarray(pre), exp[0]) and np.array_equal(np.asarray(post), exp[3])
    assert np.array_equal(act, exp[1]) and act.dtype == exp[1].dtype
    assert np.array_equal(term, exp[4]) and term.dtype == np.bool_
    if n == 1:
        assert np.array_equal(rew, exp[2]) and rew.dtype == exp[2].dtype
    else:
        assert rew.dtype == np.float64 and np.array_equal(rew.view(np.int64), exp[2].view(np.int64))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("B", [257, 320])
@pytest.mark.parametrize("dt", ["float32", "float16"])
def test_ring_gather_through_the_pinned_slot(sd, dt, B, n):
    """getMinibatch() above 256 (replay_push_idx -> gather_kernel<false> -> replay_release_idx) against ReplayOracle's gather of the same
    indexes, byte for byte, all five arrays; Python's random stream consumed as the oracle's MT19937 consumes it; three gathers in a row
    (the pinned slot pushed and released each time) with an add() between the second and the third; n_step 1 and 3."""
    mem, om = _mems(sd, dt, B, n)
    scr = np.random.RandomState(9).randint(0, 256, (84, 84), dtype=np.uint8)
    for k, seed in enumerate((11, 12, 13)):
        if k == 2:
            mem.add(2, 1, scr, True)
            om.add(2, 1, scr, True)
        random.seed(seed)
        rng = MT19937()
        rng.setstate(random.getstate()[1])
        mb = mem.getMinibatch()
        oidx, _ = N.sample_indexes(rng, om.terminals, om.count, om.current, om.history_length, n, B)
        if n == 1:
            rng1 = MT19937(seed)
            assert np.array_equal(oidx, om.sample_indexes(rng1))               # (the n = 1 rule is the reference sampler's)
        assert np.array_equal(mem.last_indexes, oidx), k
        assert random.getstate()[1] == rng.getstate(), k
        _compare_gather(mb, _expected_gather(om, oidx, n), n)
        idx2 = oidx[::-1].copy()                                               # gather() by index: same branch, another order
        _compare_gather(mem.gather(idx2), _expected_gather(om, idx2, n), n)


@pytest.mark.parametrize("B", [257, 320])
@pytest.mark.parametrize("dt", ["float32", "float16"])
def test_train_from_ring_equals_tuple_api(sd, dt, B):
    """train_from_memory(mem, 3) — standalone prep for step 0, the prep riding in the update launch after it, both past their first 256
    samples, and the cost mean over more than 256 terms — against three train(getMinibatch()) calls of a twin from the same random state:
    weights and RMSProp state bit-identical (test_train_replay_equals_train_host), mean cost equal to the mean of the three to 1e-6."""
    A = 4
    mem, _ = _mems(sd, dt, B, 1, A=A)
    nets = []
    for _ in range(2):
        net = sd.DeepQNetwork(A, make_args(batch_size=B, datatype=dt))
        net.set_weights(xavier_weights(A, 32), 1)
        net.set_weights(xavier_weights(A, 31), 0)
        nets.append(net)
    n1, n2 = nets
    random.seed(5)
    st = random.getstate()
    mean = n1.train_from_memory(mem, 3, want_cost=True)
    after = random.getstate()
    random.setstate(st)
    costs = []
    n2.callback = type("CB", (), {"on_train": lambda self, c: costs.append(c)})()
    for _ in range(3):
        n2.train(mem.getMinibatch())
    assert random.getstate() == after
    for i in range(5):
        assert np.array_equal(n1.get_layer(i, 0), n2.get_layer(i, 0)), i
        assert np.array_equal(n1.get_layer(i, 2), n2.get_layer(i, 2)), i
    print("%s B=%d: mean cost %r, the twin's costs %r" % (dt, B, mean, costs))
    assert len(costs) == 3 and np.isfinite(mean) and mean > 0
    assert abs(mean - np.mean(costs)) < 1e-6 * max(1.0, abs(np.mean(costs)))


def test_double_dqn_b257_one_step(sd):
    """--double_dqn, float32, B = 257: the third net slot rides in the sample-stationary chain (nz = 3: 387 workgroups of two samples, the
    last of each slot with one) — one step against tests/double_dqn_oracle.py in float64 at the B >= 128 bounds of part 1.  The weights
    are draws whose online top-2 gap on the poststates is clear of the Q tolerance on every sample (so the step's action choice is not
    decided by round-off) and whose online / target argmaxes differ somewhere (so a library ignoring the option fails)."""
    name = "ddqn_b257"
    o = _oracle(name)
    g, cost, _, preq = o.gradients(_minibatch(name))
    top = np.sort(o.last_online_postq, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 3 * Q_TOL
    differ = o.last_online_postq.argmax(1) != o.last_target_postq.argmax(1)
    print("%s: online / target argmax differ on %d of %d samples" % (name, int(differ.sum()), len(differ)))
    assert differ.any() and np.abs(o.last_maxpostq - o.last_target_postq.max(1)).max() > Q_TOL
    _check_step(name, _device_step(sd, name), o, g, cost, preq)


def test_prioritized_replay_refuses_batch_257(sd):
    """PER_MAX_B = 256 (sdqn_per.h): the sampling launch carries its uniform draws in the kernel arguments"""
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6)
    with pytest.raises(Exception, match=r"batch sizes up to 256 \(got 257\)"):
        sd.ReplayMemory(600, make_args(batch_size=257, **kw))
    mem = sd.ReplayMemory(600, make_args(batch_size=256, **kw))                # the limit itself is accepted
    assert mem.prioritized
