"""--quantiles without a device: the oracle's gradients and cost against torch autograd of the quantile Huber loss, the
edge inputs |delta| = kappa and delta = 0, the C ABI's host restatement against the oracle to the last bit, the row layout and the
mean-acting rule, the command line and its refusals, the compiler's resource report of the new kernels, and the existing route and
step-trace goldens regenerated (with the new head's line read from the trace tool's own quantile grid)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_dqn_amd as sd  # noqa: E402
from simple_dqn_amd import _lib  # noqa: E402
import quantile_oracle as QO  # noqa: E402
from nstep_oracle import gamma_n  # noqa: E402
from oracle.dqn_numpy import xavier_weights  # noqa: E402
from test_oracle_dqn import _neon_grads, _torch_fwd, _torch_weights  # noqa: E402
from util import make_args, random_minibatch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdqn_net_set_quantiles", "sdqn_net_get_quantiles", "sdqn_net_last_quantile_step", "sdqn_quantile_loss", "sdqn_quantile_act")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402


def _torch_loss(theta, T, N, kappa):
    """mean over the N^2 pairs of |tau_j - 1[delta > 0]| huber_kappa(delta) / kappa; theta [N] with grad, T [N] detached"""
    taus = torch.tensor([(2 * j + 1) / (2.0 * N) for j in range(N)], dtype=torch.float64)[:, None]
    d = theta[:, None] - T[None, :]
    w = torch.abs(taus - (d.detach() > 0).to(torch.float64))
    return (w * F.huber_loss(d, torch.zeros_like(d), reduction="none", delta=kappa) / kappa).mean()


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("A,N", [(2, 2), (3, 6), (2, 9), (1, 5)])
def test_oracle_matches_torch_autograd_of_the_quantile_huber_loss(A, N, n_step):
    torch.set_num_threads(4)
    B, dt, kappa = 6, np.float64, 1.0
    o = QO.QuantileOracle(A, N, batch_size=B, dtype=dt, weights=xavier_weights(N * A, 1, dt), n_step=n_step)
    o.Wt = [w.copy() for w in xavier_weights(N * A, 2, dt)]
    pre, act, rew, post, term = random_minibatch(B, A, 3)
    term = np.array([True, False, False, True, False, False])                 # terminal and non-terminal samples
    if n_step > 1:
        rew, gam = np.random.RandomState(4).uniform(-2.5, 2.5, B), gamma_n(n_step, 0.99)     # the returns R as the n-step gather hands them over
        r = torch.tensor(rew)
    else:
        gam, r = 0.99, torch.tensor(np.clip(rew, -1, 1)).to(torch.float64)
    g, cost, deltas, preq = o.gradients((pre, act, rew, post, term))
    w, wt = _torch_weights(o.W, torch.float64), _torch_weights(o.Wt, torch.float64)
    with torch.no_grad():
        qp = _torch_fwd(wt, post, torch.float64).reshape(B, N, A)
        astar = qp.mean(1).argmax(1)
        nxt = qp[torch.arange(B), :, astar]                                    # [B][N]
        T = torch.where(torch.tensor(term)[:, None], r[:, None].expand(B, N), r[:, None] + gam * nxt)
    q = _torch_fwd(w, pre, torch.float64)
    theta = q.reshape(B, N, A)[torch.arange(B), :, torch.tensor(act.astype(np.int64))]
    losses = torch.stack([_torch_loss(theta[n], T[n], N, kappa) for n in range(B)])
    losses.sum().backward()
    assert (o.last_gaps > QO.GAP).all()
    assert np.abs(q.detach().numpy() - preq).max() < 1e-11
    assert np.abs(o.last_targets - T.numpy()).max() < 1e-12
    assert np.abs(o.last_maxq - qp.mean(1).max(1).values.numpy()).max() < 1e-12
    assert abs(float(losses.mean().detach()) - float(cost)) < 1e-12
    for a, b in zip(_neon_grads(w), g):
        assert np.abs(a - b).max() < 1e-11 * max(1.0, np.abs(b).max())
    live = np.zeros((B, N, A), bool)
    live[np.arange(B), :, act.astype(np.int64)] = True
    assert (deltas.reshape(B, N, A)[~live] == 0).all() and (deltas != 0).sum() > B


def _c_loss(N, A, kappa, q_pre, q_post, action, r, terminal, gam):
    lib = sd.load()
    q_pre, q_post = np.ascontiguousarray(q_pre, np.float32), np.ascontiguousarray(q_post, np.float32)
    dq, cost = np.full(N * A, 7.0, np.float32), C.c_float()
    _lib.check(lib.sdqn_quantile_loss(N, A, float(kappa), _lib.ptr(q_pre, C.c_float), _lib.ptr(q_post, C.c_float), int(action), float(r),
                                      int(terminal), float(gam), _lib.ptr(dq, C.c_float), C.byref(cost)))
    return dq, np.float32(cost.value)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_edge_inputs_delta_equal_kappa_and_delta_zero():
    """terminal sample, r = 0: every target is 0, so delta_jj' = theta_j.  theta = (kappa, 0): quantile 0's pairs sit on the Huber knee,
    quantile 1's on the indicator's step (strict: delta = 0 counts as not above)"""
    N, A, kappa = 2, 2, 0.5
    q_pre = np.array([0.5, 9.0, 0.0, 9.0], np.float32)                       # rows j A + a: action 0 holds (kappa, 0)
    q_post = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    o = QO.sample(q_pre, q_post, N, A, 0, 0.0, True, 0.99, kappa)
    # quantile 0: delta = kappa > 0 -> w = 1 - 1/4, clip = kappa, L = 0.5 kappa^2 from both branches; two pairs, over N^2 = 4
    assert o["dq"][0] == np.float32(2 * 0.75 * 0.5 / 0.5 / 4) and o["dq"][2] == 0.0 and o["dq"][1] == 0.0 and o["dq"][3] == 0.0
    assert o["cost"] == np.float32(2 * 0.75 * 0.5 * 0.25 / 0.5 / 4)
    g, rho = QO.pair(np.float32(0.0), QO.tau(1, 2), np.float32(kappa), np.float32)
    assert g == 0.0 and rho == 0.0
    g_in, _ = QO.pair(np.float32(np.nextafter(np.float32(0.5), np.float32(0))), QO.tau(0, 2), np.float32(kappa), np.float32)
    g_out, _ = QO.pair(np.float32(np.nextafter(np.float32(0.5), np.float32(1))), QO.tau(0, 2), np.float32(kappa), np.float32)
    assert g_in < g_out == np.float32(0.75)                                   # the knee: linear inside, flat outside
    gm, _ = QO.pair(np.float32(-1e-30), QO.tau(1, 2), np.float32(kappa), np.float32)
    gp, _ = QO.pair(np.float32(1e-30), QO.tau(1, 2), np.float32(kappa), np.float32)
    assert gm < 0 < gp and abs(gm / gp) == pytest.approx(3.0)                 # the step: tau on and below zero, 1 - tau above
    dq, cost = _c_loss(N, A, kappa, q_pre, q_post, 0, 0.0, True, 0.99)
    assert np.array_equal(_bits(dq), _bits(o["dq"])) and _bits(cost) == _bits(o["cost"])
    # the same through autograd: the subgradient torch takes at both points is the stated one
    theta = torch.tensor([0.5, 0.0], dtype=torch.float64, requires_grad=True)
    _torch_loss(theta, torch.zeros(2, dtype=torch.float64), N, kappa).backward()
    assert np.allclose(theta.grad.numpy(), o["dq"].reshape(N, A)[:, 0], atol=1e-7)


@pytest.mark.parametrize("A,N", [(2, 2), (3, 6), (2, 9), (1, 5), (1, 18), (9, 2)])
def test_c_abi_loss_equals_the_oracle_to_the_last_bit(A, N):
    rng = np.random.RandomState(100 * A + N)
    n = 0
    for kappa in (1.0, 0.5, 3.0):
        for s in range(40):
            q_pre = (rng.randn(N * A) * (0.3 if s % 2 else 2.0)).astype(np.float32)
            q_post = (rng.randn(N * A) * 1.5).astype(np.float32)
            action, terminal = int(rng.randint(A)), bool(s % 5 == 0)
            r, gam = (float(rng.randint(-1, 2)), 0.99) if s % 3 else (float(rng.uniform(-2.9, 2.9)), gamma_n(3, 0.99))
            if s % 7 == 0:
                q_pre[action] = np.float32(r) + np.float32(kappa) if terminal else q_pre[action]      # a pair exactly on the knee
            o = QO.sample(q_pre, q_post, N, A, action, r, terminal, gam, kappa)
            dq, cost = _c_loss(N, A, kappa, q_pre, q_post, action, r, terminal, gam)
            assert np.array_equal(_bits(dq), _bits(o["dq"])), (kappa, s)
            assert _bits(cost) == _bits(o["cost"]), (kappa, s)
            n += int((dq != 0).sum())
    assert n > 100
    lib, out, c = sd.load(), np.zeros(N * A, np.float32), C.c_float()
    assert lib.sdqn_quantile_loss(N, A, 0.0, _lib.ptr(out, C.c_float), _lib.ptr(out, C.c_float), 0, 0.0, 0, 0.99, _lib.ptr(out, C.c_float), C.byref(c)) != 0
    assert lib.sdqn_quantile_loss(N, A, 1.0, _lib.ptr(out, C.c_float), _lib.ptr(out, C.c_float), A, 0.0, 0, 0.99, _lib.ptr(out, C.c_float), C.byref(c)) != 0


def test_row_layout_and_the_greedy_poststate_action():
    """row j A + a is quantile j of action a: dq is non-zero on rows j A + a_n only, the targets read the rows j' A + a*"""
    N, A = 3, 2
    q_post = np.array([0.0, 1.0, 5.0, 1.0, 0.0, 2.0], np.float32)            # m = (5/3, 4/3): a* = 0 although action 1 wins two quantiles
    q_pre = np.arange(6, dtype=np.float32)
    o = QO.sample(q_pre, q_post, N, A, 1, 1.0, False, 0.5, 1.0)
    assert o["astar"] == 0 and o["maxq"] == np.float32(5.0 / 3.0) and np.array_equal(o["targets"], np.array([1.0, 3.5, 1.0], np.float32))
    assert np.array_equal(o["dq"] != 0, np.array([0, 1, 0, 1, 0, 1], bool))
    dq, _ = _c_loss(N, A, 1.0, q_pre, q_post, 1, 1.0, False, 0.5)
    assert np.array_equal(_bits(dq), _bits(o["dq"]))
    # the first maximum wins; a NaN m(a) is never chosen over a number, a NaN m(0) stays (head_kernel's Double DQN argmax)
    nan = float("nan")
    assert QO.greedy([1.0, 1.0]) == 0 and QO.greedy([0.0, 2.0, 2.0]) == 1 and QO.greedy([0.0, nan, -1.0]) == 0 and QO.greedy([nan, 5.0]) == 0
    tie = np.array([1.0, 3.0, 3.0, 1.0], np.float32)                          # N = 2, A = 2: m = (2, 2)
    assert QO.sample(np.zeros(4, np.float32), tie, 2, 2, 0, 0.0, False, 1.0, 1.0)["astar"] == 0
    dq_nan, _ = _c_loss(2, 2, 1.0, np.zeros(4, np.float32), np.array([0.0, nan, 0.0, 9.0], np.float32), 0, 0.0, False, 1.0)
    assert np.array_equal(_bits(dq_nan), _bits(QO.sample(np.zeros(4, np.float32), np.array([0.0, nan, 0.0, 9.0], np.float32), 2, 2, 0, 0.0, False, 1.0, 1.0)["dq"]))
    assert not np.isnan(dq_nan).any()


def test_mean_acting_rule_with_a_tie_and_a_nan_row():
    lib, a = sd.load(), C.c_int()
    nan = float("nan")
    rows = {  # N = 2, A = 3
        "mean_not_vote": ([0, 1, 0, 7, 1, 0], 0),                              # action 1 wins no quantile alone: means (3.5, 1, 0)
        "tied_maximum": ([1, 3, 0, 3, 1, 0], 0),                               # means (2, 2, 0): the first
        "tie_later": ([0, 3, 1, 0, 1, 3], 1),                                  # means (0, 2, 2)
        "nan_counts_as_max": ([0, nan, 5, 0, 3, 9], 1),
        "nan_first": ([nan, 1, 5, 0, 3, 9], 0),
        "nan_row": ([nan] * 6, 0),
    }
    for name, (row, want) in rows.items():
        q = np.array(row, np.float32)
        assert QO.act(q, 2, 3) == want, name
        _lib.check(lib.sdqn_quantile_act(_lib.ptr(q, C.c_float), 2, 3, C.byref(a)))
        assert a.value == want, name
    rng = np.random.RandomState(2)
    for N, A in ((6, 3), (9, 2), (2, 2), (1, 4), (18, 1)):
        for _ in range(50):
            q = rng.randn(N * A).astype(np.float32)
            _lib.check(lib.sdqn_quantile_act(_lib.ptr(q, C.c_float), N, A, C.byref(a)))
            assert a.value == QO.act(q, N, A)
    v = QO.action_values(np.array([1, 2, 3, 4, 5, 6], np.float32), 3, 2)
    assert np.array_equal(v, np.array([(np.float32(1) + np.float32(3) + np.float32(5)) / np.float32(3), np.float32(12) / np.float32(3)], np.float32))


def test_parser_defaults_and_refusals_before_any_device_call(monkeypatch):
    from simple_dqn_amd import main
    from simple_dqn_amd.deepqnetwork import check_quantiles
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded before the refusal")))
    monkeypatch.setattr(_lib, "bind_device", lambda args: (_ for _ in ()).throw(AssertionError("a device was bound before the refusal")))
    d = main.build_parser().parse_args([])
    assert d.quantiles == 1 and main.check_quantiles(d) == 1
    on = main.build_parser().parse_args(["--quantiles", "6"])
    assert main.check_quantiles(on) == 6 and check_quantiles(on, 3) == 6 and check_quantiles(main.build_parser().parse_args(["--quantiles", "9"]), 2) == 9
    with pytest.raises(ValueError) as ei:
        check_quantiles(main.build_parser().parse_args(["--quantiles", "19"]), 1)
    assert "19" in str(ei.value) and "18" in str(ei.value)
    with pytest.raises(ValueError) as ei:                           # the constructor refuses before it loads the library or binds a device
        sd.DeepQNetwork(4, make_args(quantiles=5))
    assert "--quantiles 5" in str(ei.value) and "4" in str(ei.value) and "20" in str(ei.value) and "18" in str(ei.value)
    base = ["--quantiles", "2", "--random_steps", "0", "--epochs", "0"]
    cases = ((["--double_dqn", "true"], ("--quantiles", "--double_dqn")),
             (["--prioritized_replay", "true"], ("--quantiles", "--prioritized_replay")),
             (["--munchausen", "true"], ("--quantiles", "--munchausen")),
             (["--advantage_learning", "0.5"], ("--quantiles", "--advantage_learning")),
             (["--bootstrap_heads", "2"], ("--quantiles", "--bootstrap_heads")),
             (["--batch_norm", "true"], ("--quantiles", "--batch_norm")),
             (["--clip_error", "0"], ("--quantiles", "--clip_error")),
             (["--clip_error", "-1"], ("--quantiles", "--clip_error")),
             (["--quantiles", "0"], ("--quantiles",)))
    for extra, words in cases:
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
        kw = {k: getattr(args, k) for k in ("quantiles", "double_dqn", "prioritized_replay", "munchausen", "advantage_learning", "bootstrap_heads",
                                            "batch_norm", "clip_error")}
        with pytest.raises(ValueError) as ei:
            sd.DeepQNetwork(3, make_args(**kw))
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
    # with one quantile none of them is refused by this check, and clip_error 0 keeps its meaning
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true", "--clip_error", "0"])
    assert main.check_quantiles(off) == 1
    # what it composes with parses and passes the check
    ok = main.build_parser().parse_args(["--quantiles", "6", "--n_step", "3", "--target_tau", "0.01", "--clip_grad_norm", "10", "--train_envs", "32",
                                         "--eval_envs", "32", "--environment", "catch"])
    assert main.check_quantiles(ok, 3) == 6


def test_symbols_in_signatures_header_and_library():
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name in hdr, name


needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_census.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_isa_census_of_the_quantile_kernels():
    """every quantile head: no scratch, at most 128 registers, LDS no larger than head_kernel's for the same action bucket"""
    rows = isa_census.census_rows("sdqn_quantile.hip")
    mine = [r for r in rows if "quantile_head_kernel" in r["name"]]
    std = isa_census.census_rows("sdqn_kernels.hip")
    assert len(mine) == 6, [r["name"] for r in mine]               # 3 buckets x {one-step, n-step}
    for bucket in (4, 8, 18):
        ref = [r for r in std if "head_kernelILi%dELb0ELb0ELb0ELb0ELb0E" % bucket in r["name"]]
        assert len(ref) == 1, bucket
        sel = [r for r in mine if "quantile_head_kernelILi%dE" % bucket in r["name"]]
        assert len(sel) == 2
        for r in sel:
            print("%s: vgpr %d lds %d scratch %d (head_kernel: lds %d)" % (r["name"][:60], r["vgpr"], r["lds"], r["scratch"], ref[0]["lds"]))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] <= ref[0]["lds"], (r["name"], r["lds"], ref[0]["lds"])
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])
    mean = [r for r in rows if "quantile_mean_kernel" in r["name"]]
    assert len(mean) == 2
    for r in mean:
        assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 128, r


def test_route_golden_regenerates_identically():
    import route_emul as R
    assert list(R.table_lines()) == open(os.path.join(ROOT, "tests", "golden", "launch_routes.txt")).read().splitlines()


@needs_hipcc
def test_step_trace_goldens_regenerate_and_the_quantile_step_ends_its_forward_with_head_6(tmp_path):
    from step_trace_golden import GOLDEN
    env = dict(os.environ, HIPCC=isa_census.HIPCC)
    thin = subprocess.run(["sh", os.path.join(ROOT, "tools", "step_trace.sh"), str(tmp_path)], env=env, capture_output=True, text=True)
    assert thin.returncode == 0, thin.stderr[-2000:]
    assert thin.stdout == open(GOLDEN).read()
    assert " train=6 " not in thin.stdout
    q = subprocess.run([os.path.join(str(tmp_path), "step_trace"), "--quantiles"], capture_output=True, text=True)
    assert q.returncode == 0 and "ERROR" not in q.stdout
    blocks = [b.splitlines() for b in q.stdout.split("train B=")[1:]]
    assert len(blocks) == 9
    for b in blocks:
        heads = [l for l in b if " head " in l]
        assert len(heads) == 1 and " train=6 " in heads[0] and " nz=2 " in heads[0], b[0]        # one forward, two net slots, the quantile head
        assert b[-1].startswith("  -> rc=0 ") and " blend " in b[-2], b[0]
    # the launches around the head are those of a standard step of the same cell: only the head's `train` differs
    std = subprocess.run([os.path.join(str(tmp_path), "step_trace"), "--full"], capture_output=True, text=True).stdout
    first = "train B=32 float32 fused=1 dp=none clip=0 target=standard next=0 opt=rmsprop keep_grads=0\n"
    want = std.split(first)[1].split("train B=")[0].replace(" train=1 ", " train=6 ")
    assert want == q.stdout.split(first)[1].split("train B=")[0]
