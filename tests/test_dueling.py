"""--dueling without a device: the oracle against torch autograd of a masked two-stream net, the function class (the
streams do not see each other's hidden units), the C ABI's host restatements against the oracle to the last bit, the command line and its
refusals, the step trace of a dueling step, the compiler's resource report of the new kernels, and the existing route and step-trace
goldens regenerated."""
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
import dueling_oracle as DO  # noqa: E402
from nstep_oracle import gamma_n  # noqa: E402
from oracle.dqn_numpy import xavier_weights  # noqa: E402
from test_oracle_dqn import _neon_grads, _torch_fwd, _torch_weights  # noqa: E402
from util import make_args, random_minibatch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdqn_net_set_dueling", "sdqn_net_get_dueling", "sdqn_net_last_dueling_step", "sdqn_dueling_loss", "sdqn_dueling_act")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402


def _torch_streams(w, x, A):
    """(V [B], Adv [B][A]) of the masked two-stream net: the torso of tests/test_oracle_dqn.py, fc5 multiplied by the block mask"""
    w5 = w[4] * torch.tensor(DO.mask(A, dtype=np.float64))
    raw = _torch_fwd(w[:4] + [w5], x, torch.float64)
    return raw[:, 0], raw[:, 1:]


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("A", [1, 3, 4, 17])
def test_oracle_matches_torch_autograd_of_a_masked_two_stream_net(A, n_step):
    torch.set_num_threads(4)
    B, dt = 6, np.float64
    # dense Xavier draws: the oracle masks them itself, torch multiplies by the mask
    ws, wt = xavier_weights(A + 1, 1, dt), xavier_weights(A + 1, 2, dt)
    o = DO.DuelingOracle(A, batch_size=B, dtype=dt, weights=ws, n_step=n_step)
    o.set_target(wt)
    pre, act, rew, post, term = random_minibatch(B, A, 3)
    term = np.array([True, False, False, True, False, False])
    if n_step > 1:
        rew, gam = np.random.RandomState(4).uniform(-2.5, 2.5, B), gamma_n(n_step, 0.99)
        r = torch.tensor(rew)
    else:
        gam, r = 0.99, torch.tensor(np.clip(rew, -1, 1)).to(torch.float64)
    g, cost, deltas, preq = o.gradients((pre, act, rew, post, term))
    assert (o.last["gaps"] > DO.GAP).all() and (o.last["edges"] > DO.GAP).all()
    w, wtt = _torch_weights(ws, torch.float64), _torch_weights(wt, torch.float64)
    with torch.no_grad():
        vp, ap = _torch_streams(wtt, post, A)
        mq = (vp[:, None] + ap - ap.mean(1, keepdim=True)).max(1).values
        y = torch.where(torch.tensor(term), r, r + gam * mq)
    v, adv = _torch_streams(w, pre, A)
    q = v[:, None] + adv - adv.mean(1, keepdim=True)
    qa = q.gather(1, torch.tensor(act.astype(np.int64))[:, None])[:, 0]
    F.huber_loss(qa, y, reduction="sum", delta=1.0).backward()              # d huber / d delta = clip(delta, -1, 1): the reference's clipped error
    assert np.abs(q.detach().numpy() - o.predict_q(pre)).max() < 1e-12
    assert np.abs(o.last["y"] - y.numpy()).max() < 1e-12
    assert np.abs(o.last["maxq"] - mq.numpy()).max() < 1e-12
    assert abs(float((0.5 * (qa - y) ** 2).mean().detach()) - float(cost)) < 1e-12
    for i, (a, b) in enumerate(zip(_neon_grads(w), g)):
        assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(b).max()), i
    assert (g[4][~DO.mask(A)] == 0).all() and (np.signbit(g[4][~DO.mask(A)]) == 0).all()
    # the rows' gradient: c on V, c (1[b = a_n] - 1 / A) on the advantages
    c = deltas[:, 0]
    want = np.concatenate([c[:, None], c[:, None] * ((np.arange(A)[None, :] == act[:, None]) - 1.0 / A)], axis=1)
    assert np.abs(deltas - want).max() < 1e-15
    if A == 1:
        assert (deltas[:, 1] == 0).all()


def test_function_class_the_streams_do_not_see_each_others_hidden_units():
    """a re-parametrised linear fc5 over the shared 512 units would fail both halves of this"""
    A, B, dt = 4, 6, np.float64
    o = DO.DuelingOracle(A, batch_size=B, dtype=dt, weights=xavier_weights(A + 1, 5, dt))
    x = random_minibatch(B, A, 7)[0]
    v0, a0 = o.streams(x)
    q0 = o.predict_q(x)
    w4 = o.W[3].copy()
    o.W[3] = w4.copy(); o.W[3][:256] += 0.003                                # every value-stream unit's incoming weights
    v1, a1 = o.streams(x)
    q1 = o.predict_q(x)
    assert np.array_equal(a1, a0)                                            # Adv untouched, to the bit
    assert np.abs(v1 - v0).min() > 1e-6
    assert np.abs((q1 - q0) - (v1 - v0)[:, None]).max() < 1e-12             # every Q(s, .) moves by the same amount
    o.W[3] = w4.copy(); o.W[3][256:] += 0.003                                # every advantage-stream unit's
    v2, a2 = o.streams(x)
    assert np.array_equal(v2, v0)                                            # V untouched, to the bit
    assert np.abs(a2 - a0).max() > 1e-6
    # one unit of each stream
    j = 3
    o.W[3] = w4.copy(); o.W[3][j] += 0.01
    assert np.array_equal(o.streams(x)[1], a0)
    o.W[3] = w4.copy(); o.W[3][256 + j] += 0.01
    assert np.array_equal(o.streams(x)[0], v0)


def _c_loss(A, clip, q_pre, q_post, action, r, terminal, gam, weight=None, alpha=0.6, eps=1e-6):
    lib = sd.load()
    q_pre, q_post = np.ascontiguousarray(q_pre, np.float32), np.ascontiguousarray(q_post, np.float32)
    dq = np.full(A + 1, 7.0, np.float32)
    cost, y, d, mq, p = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
    _lib.check(lib.sdqn_dueling_loss(A, float(clip), _lib.ptr(q_pre, C.c_float), _lib.ptr(q_post, C.c_float), int(action), float(r), int(terminal),
                                     float(gam), int(weight is not None), float(weight or 0.0), float(alpha), float(eps), _lib.ptr(dq, C.c_float),
                                     C.byref(cost), C.byref(y), C.byref(d), C.byref(mq), C.byref(p)))
    return dict(dq=dq, cost=np.float32(cost.value), y=np.float32(y.value), delta=np.float32(d.value), maxq=np.float32(mq.value),
                priority=np.float32(p.value))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("A", [1, 2, 3, 4, 7, 17])
def test_c_abi_loss_equals_the_oracle_to_the_last_bit(A):
    rng = np.random.RandomState(100 + A)
    n = 0
    for clip in (1.0, 0.0, 0.5):
        for s in range(40):
            q_pre = (rng.randn(A + 1) * (0.3 if s % 2 else 2.0)).astype(np.float32)
            q_post = (rng.randn(A + 1) * 1.5).astype(np.float32)
            action, terminal = int(rng.randint(A)), bool(s % 5 == 0)
            r, gam = (float(rng.randint(-1, 2)), 0.99) if s % 3 else (float(rng.uniform(-2.9, 2.9)), gamma_n(3, 0.99))
            weight = float(rng.uniform(0.1, 1.0)) if s % 4 == 0 else None
            o = DO.sample(q_pre, q_post, A, action, r, terminal, gam, clip, np.float32, weight, 0.6, 1e-6)
            c = _c_loss(A, clip, q_pre, q_post, action, r, terminal, gam, weight)
            for k in ("dq", "cost", "y", "delta", "maxq"):
                assert np.array_equal(_bits(c[k]), _bits(o[k])), (clip, s, k)
            if weight is not None:
                assert abs(float(c["priority"]) - float(o["priority"])) <= 2e-7 * float(o["priority"]), (clip, s)     # pow: one ulp between libms
            n += int((c["dq"] != 0).sum())
    assert n > 100
    if A == 1:                                                               # Adv - mean(Adv) is 0: Q = V, and the advantage row gets c x 0
        q_pre, q_post = np.array([0.5, 9.0], np.float32), np.array([0.25, -3.0], np.float32)
        c = _c_loss(1, 1.0, q_pre, q_post, 0, 0.0, False, 0.5)
        assert c["maxq"] == np.float32(0.25) and c["y"] == np.float32(0.125) and c["delta"] == np.float32(0.375)
        assert c["dq"][0] == np.float32(0.375) and c["dq"][1] == 0.0
    lib, out, cc = sd.load(), np.zeros(A + 1, np.float32), C.c_float()
    assert lib.sdqn_dueling_loss(A, 1.0, _lib.ptr(out, C.c_float), _lib.ptr(out, C.c_float), A, 0.0, 0, 0.99, 0, 0.0, 0.0, 0.0, _lib.ptr(out, C.c_float),
                                 C.byref(cc), None, None, None, None) != 0
    assert lib.sdqn_dueling_loss(18, 1.0, _lib.ptr(out, C.c_float), _lib.ptr(out, C.c_float), 0, 0.0, 0, 0.99, 0, 0.0, 0.0, 0.0, _lib.ptr(out, C.c_float),
                                 C.byref(cc), None, None, None, None) != 0


def test_acting_rule_with_ties_a_nan_row_and_one_action():
    lib, a = sd.load(), C.c_int()
    nan = float("nan")
    rows = {  # A = 3: (V, Adv_0, Adv_1, Adv_2)
        "plain": ([1, 0, 2, 1], 1),
        "v_does_not_matter": ([-50, 0, 2, 1], 1),
        "tied_maximum": ([0, 3, 3, 1], 0),
        "tie_later": ([0, 1, 3, 3], 1),
        "all_tied": ([2, 5, 5, 5], 0),
        "nan_v": ([nan, 0, 2, 1], 0),
        "nan_adv": ([0, 1, nan, 5], 0),
        "nan_row": ([nan] * 4, 0),
    }
    for name, (row, want) in rows.items():
        q = np.array(row, np.float32)
        assert DO.act(q, 3) == want, name
        qo = np.zeros(3, np.float32)
        _lib.check(lib.sdqn_dueling_act(_lib.ptr(q, C.c_float), 3, C.byref(a), _lib.ptr(qo, C.c_float)))
        assert a.value == want, name
        assert np.array_equal(_bits(qo), _bits(DO.q_values(q, 3))), name
    # a NaN Q(a) is never chosen over a number, a NaN Q(0) stays (the rule on the Q values themselves)
    assert DO.greedy([0.0, nan, -1.0]) == 0 and DO.greedy([nan, 5.0]) == 0 and DO.greedy([1.0, 1.0]) == 0 and DO.greedy([0.0, 2.0, 2.0]) == 1
    q1 = np.array([0.7, -4.0], np.float32)                                   # A = 1: the one action, Q = V
    _lib.check(lib.sdqn_dueling_act(_lib.ptr(q1, C.c_float), 1, C.byref(a), None))
    assert a.value == 0 and DO.q_values(q1, 1)[0] == np.float32(0.7)
    rng = np.random.RandomState(2)
    for A in (1, 2, 3, 4, 9, 17):
        for _ in range(50):
            q = rng.randn(A + 1).astype(np.float32)
            _lib.check(lib.sdqn_dueling_act(_lib.ptr(q, C.c_float), A, C.byref(a), None))
            assert a.value == DO.act(q, A)
    # the same through the loss: exact ties in the target row take the first maximum's value, a NaN row gives a NaN y and a finite nothing
    tie = np.array([0.0, 2.0, 2.0, -1.0], np.float32)
    c, o = _c_loss(3, 1.0, np.zeros(4, np.float32), tie, 0, 0.0, False, 1.0), DO.sample(np.zeros(4, np.float32), tie, 3, 0, 0.0, False, 1.0, 1.0)
    assert np.array_equal(_bits(c["dq"]), _bits(o["dq"])) and c["maxq"] == o["maxq"] == np.float32(1.0)
    bad = np.array([0.0, nan, 1.0, 2.0], np.float32)
    c, o = _c_loss(3, 1.0, np.zeros(4, np.float32), bad, 1, 0.0, False, 1.0), DO.sample(np.zeros(4, np.float32), bad, 3, 1, 0.0, False, 1.0, 1.0)
    assert np.isnan(c["maxq"]) and np.isnan(o["maxq"]) and np.array_equal(_bits(c["dq"]), _bits(o["dq"]))


def test_mask_layout():
    m = DO.mask(3)
    assert m.shape == (4, 512) and m[0, :256].all() and not m[0, 256:].any() and m[1:, 256:].all() and not m[1:, :256].any()
    w = DO.masked(np.full((4, 512), -2.0, np.float32))
    assert (w[~m] == 0).all() and not np.signbit(w[~m]).any() and (w[m] == -2.0).all()


def test_parser_defaults_and_refusals_before_any_device_call(monkeypatch):
    from simple_dqn_amd import main
    from simple_dqn_amd.deepqnetwork import check_dueling
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded before the refusal")))
    monkeypatch.setattr(_lib, "bind_device", lambda args: (_ for _ in ()).throw(AssertionError("a device was bound before the refusal")))
    d = main.build_parser().parse_args([])
    assert d.dueling is False and main.check_dueling(d) is False
    on = main.build_parser().parse_args(["--dueling", "true"])
    assert main.check_dueling(on) is True and check_dueling(on, 3) is True and check_dueling(on, 17) is True
    with pytest.raises(ValueError) as ei:
        check_dueling(on, 18)
    assert "18" in str(ei.value) and "19" in str(ei.value)
    with pytest.raises(ValueError) as ei:                           # the constructor refuses before it loads the library or binds a device
        sd.DeepQNetwork(18, make_args(dueling=True))
    assert "--dueling" in str(ei.value) and "19" in str(ei.value) and "18" in str(ei.value)
    base = ["--dueling", "true", "--random_steps", "0", "--epochs", "0"]
    cases = ((["--double_dqn", "true"], ("--dueling", "--double_dqn")),
             (["--munchausen", "true"], ("--dueling", "--munchausen")),
             (["--advantage_learning", "0.5"], ("--dueling", "--advantage_learning")),
             (["--bootstrap_heads", "2"], ("--dueling", "--bootstrap_heads")),
             (["--quantiles", "2"], ("--dueling", "--quantiles")),
             (["--batch_norm", "true"], ("--dueling", "--batch_norm")))
    for extra, words in cases:
        args = main.build_parser().parse_args(base + extra)
        with pytest.raises(ValueError) as ei:
            main.run(args)
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
        kw = {k: getattr(args, k) for k in ("dueling", "double_dqn", "munchausen", "advantage_learning", "bootstrap_heads", "quantiles", "batch_norm")}
        with pytest.raises(ValueError) as ei:
            sd.DeepQNetwork(3, make_args(**kw))
        assert all(w in str(ei.value) for w in words), (extra, str(ei.value))
    # with the flag off none of them is refused by this check
    off = main.build_parser().parse_args(["--double_dqn", "true", "--batch_norm", "true", "--quantiles", "2"])
    assert main.check_dueling(off) is False
    # what it composes with parses and passes the check
    ok = main.build_parser().parse_args(["--dueling", "true", "--prioritized_replay", "true", "--n_step", "3", "--target_tau", "0.01", "--clip_grad_norm", "10",
                                         "--train_envs", "32", "--eval_envs", "32", "--environment", "catch", "--optimizer", "adam"])
    assert main.check_dueling(ok, 3) is True


def test_symbols_in_signatures_header_and_library():
    hdr = open(os.path.join(ROOT, "include", "sdqn.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(sd.load(), name) and name in hdr, name


needs_hipcc = pytest.mark.skipif(not os.path.exists(isa_census.HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_isa_census_of_the_dueling_kernels():
    """every dueling head: no scratch, at most 128 registers, LDS no larger than head_kernel's for the same bucket"""
    rows = isa_census.census_rows("sdqn_dueling.hip")
    mine = [r for r in rows if "dueling_head_kernel" in r["name"]]
    std = isa_census.census_rows("sdqn_kernels.hip")
    assert len(mine) == 12, [r["name"] for r in mine]              # 3 buckets x {one-step, n-step} x {uniform, prioritized}
    for bucket in (4, 8, 18):
        ref = [r for r in std if "head_kernelILi%dELb0ELb0ELb0ELb0ELb0E" % bucket in r["name"]]
        assert len(ref) == 1, bucket
        sel = [r for r in mine if "dueling_head_kernelILi%dE" % bucket in r["name"]]
        assert len(sel) == 4
        for r in sel:
            print("%s: vgpr %d lds %d scratch %d (head_kernel: lds %d)" % (r["name"][:64], r["vgpr"], r["lds"], r["scratch"], ref[0]["lds"]))
            assert r["scratch"] == 0, (r["name"], r["scratch"])
            assert r["lds"] <= ref[0]["lds"], (r["name"], r["lds"], ref[0]["lds"])
            assert r["vgpr"] + r["agpr"] <= 128, (r["name"], r["vgpr"])
    small = [r for r in rows if "dueling_mask_kernel" in r["name"] or "dueling_q_kernel" in r["name"]]
    assert len(small) == 4
    for r in small:
        assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 128, r


def test_route_golden_regenerates_identically():
    import route_emul as R
    assert list(R.table_lines()) == open(os.path.join(ROOT, "tests", "golden", "launch_routes.txt")).read().splitlines()


def _blocks(text):
    return {b.split("\n", 1)[0]: b.split("\n", 1)[1].splitlines() for b in ("B=" + x for x in text.split("train B=")[1:])}


@needs_hipcc
def test_step_trace_goldens_regenerate_and_the_dueling_step_adds_its_head_and_one_mask_launch(tmp_path):
    from step_trace_golden import GOLDEN
    env = dict(os.environ, HIPCC=isa_census.HIPCC)
    thin = subprocess.run(["sh", os.path.join(ROOT, "tools", "step_trace.sh"), str(tmp_path)], env=env, capture_output=True, text=True)
    assert thin.returncode == 0, thin.stderr[-2000:]
    assert thin.stdout == open(GOLDEN).read()
    assert " train=7 " not in thin.stdout and "duel_mask" not in thin.stdout
    exe = os.path.join(str(tmp_path), "step_trace")
    d = subprocess.run([exe, "--dueling"], capture_output=True, text=True)
    assert d.returncode == 0 and "ERROR" not in d.stdout
    full = subprocess.run([exe, "--full"], capture_output=True, text=True).stdout
    duel, std = _blocks(d.stdout.split("apply_update")[0]), _blocks(full.split("\npredict")[0])
    assert len(duel) == 12
    MASK = "  main 12 duel_mask   w5=g+6733824 f64=0 rows=4 H=512"          # (fc5's offset in the flat vector: OFF5 floats)
    for head, lines in duel.items():
        heads = [l for l in lines if " head " in l]
        assert len(heads) == 1 and " train=7 " in heads[0] and " nz=2 " in heads[0], head
        masks = [i for i, l in enumerate(lines) if "duel_mask" in l]
        if "dp=grad_only" in head:                                           # nothing applied, nothing masked: sdqn_net_apply_update does both
            assert not masks
            want = std[head]
        else:
            # a standard step of the same cell under --clip_grad_norm runs the same split tail: the dueling step is that step with the
            # dueling head, the mask launch behind the sums / exchange and — without the flag — not the two clip launches
            assert len(masks) == 1 and lines[masks[0]] == MASK, head
            nxt = lines[masks[0] + 1]
            assert ("clip_sqnorm" in nxt) if "clip=1" in head else (" update " in nxt and "mode=2" in nxt), head
            prev = lines[masks[0] - 1]
            assert ("mode=1" in prev and " update " in prev) or "allreduce" in prev or "from_half" in prev or "group_end" in prev, (head, prev)
            ref = std[head.replace("clip=0", "clip=1")]
            want = [l for l in ref if "clip=1" in head or "clip_s" not in l]
            if "clip=0" in head and "dp=overlap" not in head:
                want[-1] = want[-1].replace("clip_ran=1", "clip_ran=0")
            lines = [l for l in lines if "duel_mask" not in l]
        if "dp=overlap" in head and "clip=0" in head:
            continue                                                         # (a clipped step leaves the overlapped form; a dueling step keeps it: no twin to compare with)
        assert [l.replace(" train=7 ", " train=1 ") for l in lines] == want, head
    # sdqn_net_apply_update: the mask in front of the clip / the apply launch
    for b in d.stdout.split("apply_update")[1:]:
        ls = b.splitlines()[1:]
        assert ls[0] == MASK and ("clip_sqnorm" in ls[1] if "clip=1" in b.splitlines()[0] else "mode=2" in ls[1]), b
