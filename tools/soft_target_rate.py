"""Cost of --target_tau: a standard net and a net with target_tau = 0.005 trained alternately in one process with train_from_memory (the
fused replay loop of the Agent path) on a synthetic-filled ring, at B = 32 and B = 256 in float32 and float16.  Prints us per step of
both, their difference and their ratio per configuration (median of the alternated rounds), and the blend launch's own device time from
the library's profile row."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated (standard, soft target) rounds")
ap.add_argument("--tau", type=float, default=0.005)
ap.add_argument("--datatype", choices=["float32", "float16"], help="one datatype only")
ap.add_argument("--batch", type=int, help="one batch size only")
ap.add_argument("--net", choices=["both", "standard", "soft"], default="both", help="one net only (a kernel trace of each form)")
a = ap.parse_args()
for dt in ([a.datatype] if a.datatype else ["float32", "float16"]):
    for B in ([a.batch] if a.batch else [32, 256]):
        args = make_args(batch_size=B, datatype=dt)
        mem = sd.ReplayMemory(20000, args)
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        nets = {k: sd.DeepQNetwork(4, make_args(batch_size=B, datatype=dt, target_tau=a.tau if k == "soft" else 0.0)) for k in ("standard", "soft")
                if a.net in ("both", k)}
        rate = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k, net in nets.items():
                net.train_from_memory(mem, 10); net.sync()
                t0 = time.perf_counter()
                net.train_from_memory(mem, a.steps); net.sync()
                if r:                                        # (round 0 warms the code objects and the caches up)
                    rate[k].append(a.steps / (time.perf_counter() - t0))
        if a.net != "both":
            print(json.dumps({"datatype": dt, "batch_size": B, a.net + "_steps_per_s": round(float(np.median(rate[a.net])), 1)}), flush=True)
            continue
        # the blend launch alone, from its dispatch packets' timestamps (outside the timed rounds)
        soft = nets["soft"]
        soft.profile(True, 27); soft.profile_reset()
        soft.train_from_memory(mem, 50); soft.sync()
        row = [p for p in soft.profile_read() if p["id"] == 27][0]
        soft.profile(False)
        s, d = float(np.median(rate["standard"])), float(np.median(rate["soft"]))
        print(json.dumps({"datatype": dt, "batch_size": B, "tau": a.tau, "standard_steps_per_s": round(s, 1), "soft_target_steps_per_s": round(d, 1),
                          "ratio": round(d / s, 4), "standard_us": round(1e6 / s, 2), "soft_target_us": round(1e6 / d, 2),
                          "added_us": round(1e6 / d - 1e6 / s, 2),
                          "blend_kernel_us": round(1e3 * row["total_ms"] / max(1, row["launches"]), 2), "blend_launches": row["launches"]}), flush=True)
