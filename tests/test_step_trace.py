"""What the host orchestration of a step sends outward — every launch, event and all-reduce of run_train, predict_forward_tuned and
sdqn_net_apply_update, with the arguments the orchestration patches — is pinned in tests/golden/step_trace.txt.  tools/step_trace.sh builds
the recording program (host code only, no device) against this tree; its output has to equal the golden byte for byte, and the whole cross
product (--full, 12 MB) has to hash to the pinned checksum.  Both were generated from the tree BEFORE run_train was rewritten around one
StepPlan (tools/step_trace.sh BUILD_DIR PARENT_CHECKOUT [--full]), so a change that moves, drops or re-patches any launch of any
configuration shows up here as a diff of readable lines.  The golden names every distinct line once, numbered, and writes each step as
the numbers of its lines (tests/step_trace_golden.py reads it back).

What FOLLOWS an applied step — the regulariser, the blend of --target_tau, the ReDo and reset events with the derived copies each rebuilds —
and every refusal of those three features, in both directions, is pinned the same way in tests/golden/step_trace_events.txt (--events, written
out in full).  It was generated from the tree BEFORE those launches moved behind one hook (step_applied) and one refresh (refresh_derived)."""
import hashlib
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402  (HIPCC: where the compiler-driven CPU tests find the compiler)

from step_trace_golden import GOLDEN, golden_blocks  # noqa: E402

FULL_SHA256 = os.path.join(HERE, "golden", "step_trace_full.sha256")
EVENTS = os.path.join(HERE, "golden", "step_trace_events.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(isa_census.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("step_trace"))
    env = dict(os.environ, HIPCC=isa_census.HIPCC)
    thin = subprocess.run(["sh", os.path.join(ROOT, "tools", "step_trace.sh"), out], env=env, capture_output=True, text=True)
    assert thin.returncode == 0, thin.stderr[-2000:]
    return os.path.join(out, "step_trace"), thin.stdout


def test_trace_equals_the_golden(tool):
    got, want = tool[1].splitlines(), open(GOLDEN).read().splitlines()
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, "%d lines against %d; first difference at line %d:\n- %s\n+ %s" % (
        len(got), len(want), diff[0][0] + 1 if diff else 0, diff[0][2] if diff else "", diff[0][1] if diff else "")
    assert tool[1] == open(GOLDEN).read()


def test_full_grid_hashes_to_the_pinned_checksum(tool):
    full = subprocess.run([tool[0], "--full"], capture_output=True)
    assert full.returncode == 0
    assert hashlib.sha256(full.stdout).hexdigest() == open(FULL_SHA256).read().split()[0]


def test_events_trace_equals_the_golden(tool):
    run = subprocess.run([tool[0], "--events"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got, want = run.stdout.splitlines(), open(EVENTS).read().splitlines()
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, "%d lines against %d; first difference at line %d:\n- %s\n+ %s" % (
        len(got), len(want), diff[0][0] + 1 if diff else 0, diff[0][2] if diff else "", diff[0][1] if diff else "")
    assert run.stdout == open(EVENTS).read()


def test_events_golden_covers_every_event_and_refusal():
    """the events golden reaches every launch that follows a step, each derived copy, the three shapes of a reset's range, and all refusals"""
    text = open(EVENTS).read()
    assert " ? " not in text and "=? " not in text
    for needle in (" regularize ", " blend ", " redo_scores ", " redo_apply ", " reset_apply ", " refresh16 ", " w1_planes ", " duel_mask   w5=theta+", " duel_mask   w5=theta_t+",
                   " malloc ", " memset ", "tau=0.01 wh_t=wh[1]", "theta_t=0 tau=0 ", "main    wait        ev_w4\n  main 12 regularize", "main    wait        ev_w4\n  -       malloc      alloc1 bytes=15616\n", "main    wait        ev_w4\n  -       malloc      alloc1 bytes=16\n",
                   "reset_layers=1 shrink_perturb=1 ", "reset_layers=4 ", "reset_layers=5 ", "dp=grad_only", "apply_update B=32 float16"):
        assert needle in text, needle
    for feature in ("redo_interval", "redo_now", "redo_scores", "reset_interval", "reset_now", "weight_decay", "l2_init", "regularize_now", "anchor_now", "get_anchor", "weight_norms"):
        for reason in ("is implemented for the 84x84x4", "cannot be combined with batch_norm: ", "cannot be combined with noisy_nets: ", "cannot be combined with data parallel on 2 ranks: "):
            assert "  ERROR %s %s" % (feature, reason) in text, (feature, reason)
    for on in ("redo_interval 5", "reset_interval 5", "weight_decay 0.1 / l2_init 0", "weight_decay 0 / l2_init 0.01"):
        assert "  ERROR noisy_nets cannot be combined with %s: " % on in text and "  ERROR data parallel with 2 ranks cannot be combined with %s: " % on in text, on


def test_golden_covers_every_structure_and_tail():
    """the thinned grid reaches every launch structure, every exchange and both entry points besides run_train; no step reports an error"""
    blocks = golden_blocks()
    text = open(GOLDEN).read()
    assert "ERROR" not in text and " ? " not in text and "=? " not in text
    assert all(lines[-1].startswith("  -> rc=0 ") for lines in blocks.values())
    for needle in (" 24 wgrads ", " 16 bwd3 ", " 6 fc4_wgrad ", "comm 12 update ", "group_start", " to_half ", "dtype=6", "clip_scale", "bn_update", "mode=0", "mode=1", "mode=2", "nz=3",
                   "train=3", "train=2", "v=48", "f4w=940+470"):
        assert needle in text, needle
    assert any(h.startswith("predict_one ") for h in blocks) and any(h.startswith("apply_update(half payload) ") for h in blocks)
    # a grad_only step applies nothing and does not blend; every other step ends with the blend of --target_tau
    for header, lines in blocks.items():
        if header.startswith("train "):
            assert (" blend " in lines[-2]) == ("dp=grad_only" not in header), header
