"""One profiled ring step from a 64-slot memory per case: the launches per profiler id — the update slot, the all-reduces, the BatchNorm
passes and the soft target update included, which test_gpu_launch_route.py leaves out — are what the recorded orchestration of that
configuration holds in tests/golden/step_trace.txt (written from the tree before run_train was rewritten around one StepPlan).  A traced
launch of a routed stage counts when resolve_route (tests/route_emul.py) gives it a kernel of its own; a stage that rides in a sibling's
launch leaves no sample.  Shapes: the smallest at which each optimizer tail and each launch structure runs."""
import random
import re

import pytest

import route_emul as R
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from step_trace_golden import golden_blocks
from util import make_args

pytestmark = pytest.mark.gpu

PREP = 15
# (datatype, batch_norm, B, data-parallel form, clip)
CASES = [("float32", False, 32, "none", 0), ("float32", False, 32, "none", 1), ("float32", False, 32, "grad_only", 0), ("float32", False, 32, "serial", 0),
         ("float32", False, 32, "overlap", 0), ("float32", True, 32, "none", 0), ("float32", True, 32, "none", 1),
         ("float16", False, 128, "none", 0), ("float16", False, 128, "serial", 0)]


@pytest.fixture(scope="module")
def blocks():
    return golden_blocks()


def expected_counts(lines, h16):
    """profiler id -> samples of one traced step: every line that names a kernel id, minus the routed stages that ride in another launch"""
    want = {}
    for line in lines:
        m = re.match(r"  (?:main|comm) +(\d+) (\S+)", line)
        if not m:
            continue
        kid = int(m.group(1))
        if m.group(2) in ("to_half", "from_half"):             # launched, but their launchers (sdqn_kernels.hip) are plain launches that do not
            continue                                           # take the profiler's event pair: bracketed in the update slot, no sample
        if kid in R.IDS and kid not in (4, 12):               # a GEMM-shaped stage: launch_kernel resolves its route
            f = dict(kv.split("=") for kv in line.split() if "=" in kv)
            unit = R.route(kid, int(f["B"]), int(f["nz"]), h16, int(f["bn"]), f4w=int(f["f4w"].split("+")[1] != "0"), ring=int(f["ring"]),
                           hidx=int(f["hidx"]), variant=int(f["v"]))[0]
            if unit == "none":
                continue
        want[kid] = want.get(kid, 0) + 1
    return want


@pytest.mark.parametrize("datatype,bn,B,dp,clip", CASES)
def test_profiled_step_launches_what_the_trace_recorded(blocks, datatype, bn, B, dp, clip):
    import simple_dqn_amd as sd
    from simple_dqn_amd.deepqnetwork import dp_unique_id
    header = "train B=%d %s fused=1 dp=%s clip=%d target=standard next=0 opt=rmsprop keep_grads=0" % (B, datatype + ("+bn" if bn else ""), dp, clip)
    want = expected_counts(blocks[header], 2 if datatype == "float16" else 0)
    want[PREP] = 1                                             # (the ring path's own prep launch in front of run_train)
    A = 4
    args = make_args(batch_size=B, datatype=datatype, batch_norm=bn, replay_size=64)
    mem = sd.ReplayMemory(64, args)
    synthetic_fill(mem, 5, num_actions=A)
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    net.set_weights(xavier_weights(A, 12), 1)
    net.set_weights(xavier_weights(A, 11), 0)
    net.set_target_tau(0.01)                                   # as in the trace: every applied step ends with its blend
    if clip:
        net.set_clip_grad_norm(10.0)
    if dp == "grad_only":
        net.set_option("grad_only", 1)
    if dp in ("serial", "overlap"):
        net.set_option("dp_overlap", 1 if dp == "overlap" else 0)
        net.dp_init(dp_unique_id(), 0, 1)                      # a one-rank communicator
    net.profile(True, -1); net.profile_reset()
    random.seed(3)
    net.train_from_memory(mem, 1)
    got = {p["id"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    if dp in ("serial", "overlap"):
        net.dp_shutdown()
    print("launches:", got)
    assert got == want
