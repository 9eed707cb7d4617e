"""--bootstrap_heads without a device: the oracle's gradients against torch autograd of the stated loss, K = 1 against the
parent oracle bit for bit, the two hashes of the C ABI against their Python restatement, the vote rule, the command line and its refusals,
the C ABI symbols, and the compiler's resource report of the bootstrap head kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
import bootstrap_oracle as BO  # noqa: E402
from oracle.dqn_numpy import OracleDQN, xavier_weights  # noqa: E402
from test_oracle_dqn import _neon_grads, _torch_fwd, _torch_weights  # noqa: E402
from util import make_args, random_minibatch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdqn_net_set_bootstrap", "sdqn_net_get_bootstrap", "sdqn_net_bootstrap_acting", "sdqn_bootstrap_mask", "sdqn_bootstrap_head_of",
         "sdqn_bootstrap_act")


@pytest.mark.parametrize("K,P", [(1, 1.0), (2, 1.0), (6, 1.0), (6, 0.5)])
def test_gradients_match_torch_autograd_of_the_stated_loss(K, P):
    """L = sum_n (1/K) sum_k m_k huber_1(Q_k(s_n)[a_n] - y_k), y_k detached: d huber_1 / d delta = clip(delta, -1, 1)"""
    torch.set_num_threads(4)
    A, B, dt = 3, 6, np.float64
    o = BO.BootstrapOracle(A, K, batch_size=B, dtype=dt, weights=xavier_weights(K * A, 1, dt), mask_probability=P, mask_seed=5)
    o.Wt = [w.copy() for w in xavier_weights(K * A, 2, dt)]
    pre, act, rew, post, term = random_minibatch(B, A, 3)
    o.indexes = np.arange(40, 40 + B)
    g, cost, deltas, preq = o.gradients((pre, act, rew, post, term))
    m = torch.tensor(np.stack([BO.mask(5, P, K, i) for i in o.indexes]).astype(np.float64))
    assert P == 1.0 or (0 < float(m.sum()) < m.numel())
    w, wt = _torch_weights(o.W, torch.float64), _torch_weights(o.Wt, torch.float64)
    with torch.no_grad():
        mq = _torch_fwd(wt, post, torch.float64).reshape(B, K, A).max(2).values
    q = _torch_fwd(w, pre, torch.float64)
    r = torch.tensor(np.clip(rew, -1, 1)).to(torch.float64)[:, None]
    y = torch.where(torch.tensor(term)[:, None], r.expand(B, K), r + 0.99 * mq)
    qa = q.reshape(B, K, A)[torch.arange(B), :, torch.tensor(act.astype(np.int64))]
    loss = (m * F.huber_loss(qa, y, reduction="none", delta=1.0)).sum() / K
    loss.backward()
    assert np.abs(q.detach().numpy() - preq).max() < 1e-11
    d = (qa - y).detach()
    assert abs(float((m * 0.5 * d * d).sum(1).mean() / K) - float(cost)) < 1e-10
    assert np.abs(o.last_maxq - mq.mean(1).numpy()).max() < 1e-12
    for a, b in zip(_neon_grads(w), g):
        assert np.abs(a - b).max() < 1e-11 * max(1.0, np.abs(b).max())
    assert (deltas.reshape(B, K, A)[m.numpy() == 0] == 0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_head_is_the_parent_oracle_bit_for_bit(dt):
    A, B = 4, 5
    ws, wt = xavier_weights(A, 7, dt), xavier_weights(A, 8, dt)
    a, b = BO.BootstrapOracle(A, 1, batch_size=B, dtype=dt, weights=ws), OracleDQN(A, batch_size=B, dtype=dt, weights=ws)
    a.Wt, b.Wt = [w.copy() for w in wt], [w.copy() for w in wt]
    for s in range(2):
        mb = random_minibatch(B, A, 20 + s)
        ga, gb = a.gradients(mb), b.gradients(mb)
        for x, y in zip(ga[0], gb[0]):
            assert np.array_equal(x, y)
        assert ga[1] == gb[1] and np.array_equal(ga[2], gb[2]) and np.array_equal(ga[3], gb[3])
        assert a.train(mb) == b.train(mb)
    for x, y in zip(a.W + a.S, b.W + b.S):
        assert np.array_equal(x, y)


def test_hashes_of_the_c_abi_equal_the_restatement():
    lib = sd.load()
    out, k = (C.c_uint8 * 18)(), C.c_int()
    rng = np.random.RandomState(0)
    idx = [0, 1, 2, 31, 32, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 3] + [int(x) for x in rng.randint(0, 1 << 40, 600)]
    live = 0
    for seed, P, K in ((0, 0.5, 6), (1234567, 0.25, 2), (2 ** 63 + 5, 1.0, 6), (9, 0.01, 3), (3, 1e-300, 18)):
        for i in idx:
            _lib.check(lib.sdqn_bootstrap_mask(seed, P, K, i, out))
            got, ref = np.array(out[:K], np.uint8), BO.mask(seed, P, K, i)
            assert np.array_equal(got, ref), (seed, P, K, i)
            live += int(got.sum())
            if P == 1.0:
                assert got.all()
    assert live > 0
    # the rate of ones is P: 6 x 608 draws at P = 0.5
    ones = sum(int(BO.mask(0, 0.5, 6, i).sum()) for i in idx)
    assert abs(ones / (6.0 * len(idx)) - 0.5) < 0.05
    seen = set()
    for seed, K in ((0, 6), (77, 2), (2 ** 64 - 1, 18), (5, 1)):
        for copy in range(40):
            for ep in list(range(30)) + [2 ** 33, 2 ** 62]:
                _lib.check(lib.sdqn_bootstrap_head_of(seed, K, copy, ep, C.byref(k)))
                assert k.value == BO.head_of(seed, K, copy, ep) and 0 <= k.value < K
                if K == 6 and seed == 0:
                    seen.add(k.value)
    assert seen == set(range(6))
    assert lib.sdqn_bootstrap_mask(0, 0.0, 2, 0, out) != 0 and lib.sdqn_bootstrap_mask(0, 1.5, 2, 0, out) != 0


def test_a_small_probability_leaves_some_slot_without_a_head():
    """the (seed, slot) the GPU mask test uses: P = 0.5, K = 6, a slot whose six masks are all zero — found, not assumed"""
    seed, slot = BO.empty_mask_case()
    om = BO.ReplayOracle(BO.RING_SIZE, 84, 84, 4, 32)
    BO.fill_ring(om, 3)
    assert slot in BO.valid_slots(om) and not BO.mask(seed, 0.5, 6, slot).any()
    lib, out = sd.load(), (C.c_uint8 * 6)()
    _lib.check(lib.sdqn_bootstrap_mask(seed, 0.5, 6, slot, out))
    assert not any(out[:6])


def test_vote_rule_with_ties():
    lib, a = sd.load(), C.c_int()
    rows = {  # K = 3, A = 3
        "majority": ([0, 1, 0, 0, 2, 1, 5, 9, 1], 1),                 # greedy actions 1, 1, 1
        "two_one": ([3, 1, 0, 0, 0, 4, 0, 0, 5], 2),                  # 0, 2, 2
        "three_way_tie": ([0, 0, 1, 0, 1, 0, 1, 0, 0], 0),            # 2, 1, 0: one vote each -> the lowest action
        "tie_inside_a_head": ([1, 1, 0, 0, 2, 2, 0, 0, 0], 0),        # first maxima 0, 1, 0
        "nan_counts_as_max": ([0, float("nan"), 5, 0, 3, 0, 0, 0, 1], 1),   # 1, 1, 2
    }
    for name, (row, want) in rows.items():
        assert BO.vote(row, 3, 3)[0] == want, name
        q = np.array(row, np.float32)
        _lib.check(lib.sdqn_bootstrap_act(_lib.ptr(q, C.c_float), 3, 3, 1, 0, 0, 0, C.byref(a)))
        assert a.value == want, name
    q = np.array([0, 1, 2, 1, 0, 2, 1, 2, 0, 2, 1, 0], np.float32)     # K = 4, A = 3: 2, 2, 1, 0 -> 2; K = 2 of the same row x 2: exact tie
    assert BO.vote(q, 4, 3)[0] == 2
    tie = np.array([0, 1, 1, 0], np.float32)                          # K = 2, A = 2: head 0 picks 1, head 1 picks 0 -> 0
    assert BO.vote(tie, 2, 2)[0] == 0
    _lib.check(lib.sdqn_bootstrap_act(_lib.ptr(tie, C.c_float), 2, 2, 1, 0, 0, 0, C.byref(a)))
    assert a.value == 0
    # collecting: the greedy action of the episode's head
    for ep in range(12):
        k = BO.head_of(11, 2, 0, ep)
        _lib.check(lib.sdqn_bootstrap_act(_lib.ptr(tie, C.c_float), 2, 2, 0, 11, 0, ep, C.byref(a)))
        assert a.value == int(np.argmax(BO.head_slice(tie, 2, 2, k))) == 1 - k


def test_parser_defaults_and_refusals_before_any_device_call():
    from simple_dqn_amd import main
    from simple_dqn_amd.deepqnetwork import check_bootstrap
    d = main.build_parser().parse_args([])
    assert d.bootstrap_heads == 1 and d.bootstrap_mask_probability == 1.0
    assert main.check_bootstrap(d) == (1, 1.0)
    on = main.build_parser().parse_args(["--bootstrap_heads", "6", "--bootstrap_mask_probability", "0.5"])
    assert main.check_bootstrap(on) == (6, 0.5) and check_bootstrap(on, 3) == (6, 0.5)
    with pytest.raises(ValueError) as ei:
        check_bootstrap(on, 4)
    assert "24" in str(ei.value) and "18" in str(ei.value)
    with pytest.raises(ValueError) as ei:                           # the constructor refuses before it loads the library or binds a device
        sd.DeepQNetwork(4, make_args(bootstrap_heads=5))
    assert "20" in str(ei.value) and "18" in str(ei.value)
    base = ["--bootstrap_heads", "2", "--random_steps", "0", "--epochs", "0"]
    for extra, words in ((["--double_dqn", "true"], ("--bootstrap_heads", "--double_dqn")),
                         (["--prioritized_replay", "true"], ("--bootstrap_heads", "--prioritized_replay")),
                         (["--munchausen", "true"], ("--bootstrap_heads", "--munchausen")),
                         (["--batch_norm", "true"], ("--bootstrap_heads", "--batch_norm")),
                         (["--bootstrap_mask_probability", "0"], ("--bootstrap_mask_probability",)),
                         (["--bootstrap_mask_probability", "1.5"], ("--bootstrap_mask_probability",)),
                         (["--bootstrap_mask_probability", "nan"], ("--bootstrap_mask_probability",)),
                         (["--bootstrap_heads", "0"], ("--bootstrap_heads",))):
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
    # with one head the four options are not refused by this check
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true"])
    assert main.check_bootstrap(off) == (1, 1.0)


def test_symbols_in_signatures_and_library():
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name in hdr, name


def test_isa_census_of_the_bootstrap_heads():
    """every bootstrap head: no scratch, LDS no larger than head_kernel's for the same action bucket, two workgroups per CU"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_bootstrap.hip")
    mine = [r for r in rows if "bootstrap_head_kernel" in r["name"]]
    std = isa_census.census_rows("sdqn_kernels.hip")
    assert len(mine) == 6, [r["name"] for r in mine]               # 3 buckets x {one-step, n-step}
    for bucket in (4, 8, 18):
        ref = [r for r in std if "head_kernelILi%dELb0ELb0ELb0ELb0ELb0E" % bucket in r["name"]]
        assert len(ref) == 1, bucket
        for r in [r for r in mine if "bootstrap_head_kernelILi%dE" % bucket in r["name"]]:
            print("%s: vgpr %d lds %d scratch %d (head_kernel: lds %d)" % (r["name"][:60], r["vgpr"], r["lds"], r["scratch"], ref[0]["lds"]))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] <= ref[0]["lds"], (r["name"], r["lds"], ref[0]["lds"])
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])
    for r in [r for r in rows if "bootstrap_select_kernel" in r["name"]]:
        assert r["scratch"] == 0 and r["lds"] == 0, r
