"""Cost of the regulariser launches (--weight_decay / --l2_init): per datatype (float32, float16), at B = 32 on one
synthetic-filled ring in one process, four nets alternated: the default step, the step with the regulariser (WD 0.1, LAMBDA 0.01), the step
with --target_tau 0.05 (the existing blend launch) and the step with both (the fused launch).  A launch's time is the difference of the
profiled time per step of its slot (the dispatch's own begin / end stamps) between two nets: the regulariser launch and the fused launch
ride in the update slot, the blend has the target slot to itself.  The weight_norms read-out is not a profiled launch: its figure is the host's
wall time per call (two launches, an 80-byte copy and the wait), an upper bound of the kernels' time.  Prints microseconds (median of the
alternated rounds), the bytes each pass moves and their share of the HBM peak named below; --out writes the lines as a JSON list."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

HBM_SPEC_GBPS = 8000.0             # the peak the README's "43 % of HBM peak" of the replay gather is taken against
UPDATE = 12                        # the profiler's update slot: the optimizer launch, and the regulariser / fused launch behind it
OFF5, W1 = 1683456, 8192
WD, LAMBDA, TAU, A = 0.1, 0.01, 0.05, 4


def derived_bytes(dt):
    """bytes of one net's derived copies a launch writes: conv1's three bf16 planes (float32) or wh and wht (float16)"""
    return 3 * W1 * 2 if dt == "float32" else 2 * OFF5 * 2


def pass_bytes(kind, dt):
    n = OFF5 + 512 * A
    if kind == "regularize":        # theta read and written, the anchor read, the online net's derived copies
        return 12 * n + derived_bytes(dt)
    if kind == "blend":             # theta read, theta- read and written, the target's derived copies
        return 12 * n + derived_bytes(dt)
    if kind == "fused":             # theta and theta- read and written, the anchor read, both nets' derived copies
        return 20 * n + 2 * derived_bytes(dt)
    return 8 * n                    # weight_norms with an anchor: theta and the anchor read


def rate(nbytes, us):
    return {"bytes": nbytes, "GBps": round(nbytes / us / 1e3, 1) if us > 0 else None,
            "fraction_of_hbm_spec_8000_GBps": round(nbytes / us / 1e3 / HBM_SPEC_GBPS, 3) if us > 0 else None}


ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=5, help="alternated rounds")
ap.add_argument("--size", type=int, default=20000, help="replay slots")
ap.add_argument("--out", help="write the result lines here as a JSON list")
a = ap.parse_args()
lines = []
for dt in ("float32", "float16"):
    args = make_args(batch_size=32, datatype=dt)
    mem = sd.ReplayMemory(a.size, args)
    synthetic_fill(mem, 1, num_actions=A)
    mem.sync_mirror()
    on = dict(weight_decay=WD, l2_init=LAMBDA)
    nets = {"default": sd.DeepQNetwork(A, args), "regularize": sd.DeepQNetwork(A, make_args(batch_size=32, datatype=dt, **on)),
            "blend": sd.DeepQNetwork(A, make_args(batch_size=32, datatype=dt, target_tau=TAU)),
            "fused": sd.DeepQNetwork(A, make_args(batch_size=32, datatype=dt, target_tau=TAU, **on))}
    target = [p["id"] for p in nets["default"].profile_read() if "target_blend" in p["name"]][0]
    us = {k: [] for k in nets}
    upd = {k: [] for k in nets}
    tgt = {k: [] for k in nets}
    norms = []
    random.seed(1)
    for r in range(a.rounds + 1):
        for k, net in nets.items():
            net.train_from_memory(mem, 10); net.sync()
            t0 = time.perf_counter()
            net.train_from_memory(mem, a.steps)                # one call, no wait between the steps
            net.sync()
            if r:                                              # (round 0 warms the code objects and the caches up)
                us[k].append(1e6 * (time.perf_counter() - t0) / a.steps)
            net.profile(True, -1); net.profile_reset()
            net.train_from_memory(mem, 50); net.sync()
            p = net.profile_read()
            net.profile(False)
            if r:
                upd[k].append(1e3 * p[UPDATE]["total_ms"] / 50)
                tgt[k].append(1e3 * p[target]["total_ms"] / 50)
        net = nets["regularize"]
        net.sync()
        t0 = time.perf_counter()
        for _ in range(20):
            net.weight_norms()
        if r:
            norms.append(1e6 * (time.perf_counter() - t0) / 20)
    m = {k: float(np.median(v)) for k, v in us.items()}
    mu = {k: float(np.median(v)) for k, v in upd.items()}
    mt = {k: float(np.median(v)) for k, v in tgt.items()}
    reg_us, blend_us, fused_us, norms_us = mu["regularize"] - mu["default"], mt["blend"], mu["fused"] - mu["default"], float(np.median(norms))
    line = {"datatype": dt, "batch_size": 32, "weight_decay": WD, "l2_init": LAMBDA, "target_tau": TAU, "rounds": a.rounds, "steps": a.steps,
            "step_us": {k: round(v, 2) for k, v in m.items()}, "update_slot_us": {k: round(v, 2) for k, v in mu.items()},
            "target_slot_us": {k: round(v, 2) for k, v in mt.items()},
            "regularize_launch_us": round(reg_us, 2), "regularize_launch": rate(pass_bytes("regularize", dt), reg_us),
            "blend_launch_us": round(blend_us, 2), "blend_launch": rate(pass_bytes("blend", dt), blend_us),
            "fused_launch_us": round(fused_us, 2), "fused_launch": rate(pass_bytes("fused", dt), fused_us),
            "two_launches_us": round(reg_us + blend_us, 2), "fused_saves_us": round(reg_us + blend_us - fused_us, 2),
            "weight_norms_call_us": round(norms_us, 2), "weight_norms_call": rate(pass_bytes("norms", dt), norms_us)}
    lines.append(line)
    print(json.dumps(line), flush=True)
    del nets
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
