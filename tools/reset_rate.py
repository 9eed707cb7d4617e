"""Cost of one reset event (--reset_interval): per datatype (float32, float16) and --reset_layers (2 with --shrink_perturb 1:
fc4 and fc5 redrawn; 5: everything redrawn; and 2 with --shrink_perturb 0.5: fc4 and fc5 redrawn, the torso shrunk and perturbed), at
B = 32 on one synthetic-filled ring in one process, alternated: the default step and the same step with reset_interval 1 (an event behind
every step: the difference is one event with its derived-copy launches).  The kernel alone is the difference of the update slot's profiled
time per step (the dispatch's own begin / end stamps) between the two nets.  Prints microseconds (median of the alternated rounds), the bytes
the pass moves and what they would cost at the HBM rates named below; --out writes the lines as a JSON list."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

HBM_SPEC_GBPS = 8000.0             # the peak the README's "43 % of HBM peak" of the replay gather is taken against
D2D_COPY_GBPS = 4789.0             # the box's measured device-to-device copy rate (profiles/r01_box.json)
UPDATE = 12                        # the profiler's update slot: the optimizer launch, and the reset launch behind it
OFFS = (0, 8192, 40960, 77824, 1683456)


def pass_bytes(layers, alpha, A, state2):
    """(read, written) bytes of reset_apply_kernel on a net with a target net: redrawn entries write theta, theta_t, state (, state2) and read
    nothing; shrunk ones read theta and theta_t as well"""
    n = OFFS[4] + 512 * A
    redrawn = n - OFFS[5 - layers] if alpha > 0.0 else n
    shrunk = (n - redrawn) if alpha < 1.0 else 0
    return 8 * shrunk, (12 + (4 if state2 else 0)) * (redrawn + shrunk)


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
    synthetic_fill(mem, 1, num_actions=4)
    mem.sync_mirror()
    for layers, alpha in ((2, 1.0), (5, 1.0), (2, 0.5)):
        nets = {"default": sd.DeepQNetwork(4, args),
                "event": sd.DeepQNetwork(4, make_args(batch_size=32, datatype=dt, reset_interval=1, reset_layers=layers, shrink_perturb=alpha))}
        us = {k: [] for k in nets}
        kern = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k, net in nets.items():
                net.train_from_memory(mem, 10); net.sync()
                t0 = time.perf_counter()
                net.train_from_memory(mem, a.steps)            # one call, no wait between the steps
                net.sync()
                if r:                                          # (round 0 warms the code objects and the caches up)
                    us[k].append(1e6 * (time.perf_counter() - t0) / a.steps)
                net.profile(True, UPDATE); net.profile_reset()
                net.train_from_memory(mem, 50); net.sync()
                p = net.profile_read()[UPDATE]
                net.profile(False)
                if r:
                    kern[k].append(1e3 * p["total_ms"] / 50)
        m = {k: float(np.median(v)) for k, v in us.items()}
        mk = {k: float(np.median(v)) for k, v in kern.items()}
        rd, wr = pass_bytes(layers, alpha, 4, False)
        kernel_us = mk["event"] - mk["default"]
        line = {"datatype": dt, "batch_size": 32, "reset_layers": layers, "shrink_perturb": alpha, "rounds": a.rounds, "steps": a.steps,
                "default_us": round(m["default"], 2), "step_plus_event_us": round(m["event"], 2), "event_us": round(m["event"] - m["default"], 2),
                "update_slot_us": round(mk["default"], 2), "update_slot_with_reset_us": round(mk["event"], 2), "reset_kernel_us": round(kernel_us, 2),
                "bytes_read": rd, "bytes_written": wr, "floor_us_at_hbm_spec_8000_GBps": round((rd + wr) / HBM_SPEC_GBPS / 1e3, 2),
                "floor_us_at_d2d_copy_4789_GBps": round((rd + wr) / D2D_COPY_GBPS / 1e3, 2),
                "kernel_GBps": round((rd + wr) / kernel_us / 1e3, 1) if kernel_us > 0 else None,
                "kernel_fraction_of_hbm_spec": round((rd + wr) / kernel_us / 1e3 / HBM_SPEC_GBPS, 3) if kernel_us > 0 else None,
                "last_event": list(nets["event"].last_reset())}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del nets
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
