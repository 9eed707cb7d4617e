"""Cost of --clip_grad_norm: a default net and a clipped net (G = 10) trained alternately in one process with train_from_memory (the fused
replay loop of the Agent path) on one synthetic-filled ring, at B = 32 and B = 256 in float32 and float16.  Prints steps/s of both (median and
min..max of the alternated rounds), their ratio and the microseconds per step the option adds, one JSON line per configuration."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated (default, clipped) rounds")
ap.add_argument("--datatype", choices=["float32", "float16"], help="one datatype only")
ap.add_argument("--batch", type=int, help="one batch size only")
ap.add_argument("--size", type=int, default=20000, help="replay slots")
ap.add_argument("--clip_grad_norm", type=float, default=10.0)
ap.add_argument("--net", choices=["both", "default", "clip"], default="both", help="one net only (a kernel trace of each form)")
a = ap.parse_args()
for dt in ([a.datatype] if a.datatype else ["float32", "float16"]):
    for B in ([a.batch] if a.batch else [32, 256]):
        args = make_args(batch_size=B, datatype=dt)
        mem = sd.ReplayMemory(a.size, args)
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        nets = {}
        for k in ("default", "clip"):
            if a.net in ("both", k):
                nets[k] = sd.DeepQNetwork(4, args)
        if "clip" in nets:
            nets["clip"].set_clip_grad_norm(a.clip_grad_norm)
        rate = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k, net in nets.items():
                net.train_from_memory(mem, 10); net.sync()
                t0 = time.perf_counter()
                net.train_from_memory(mem, a.steps); net.sync()
                if r:                                        # (round 0 warms the code objects and the caches up)
                    rate[k].append(a.steps / (time.perf_counter() - t0))
        row = {"datatype": dt, "batch_size": B}
        for k, v in rate.items():
            row[k + "_steps_per_s"] = round(float(np.median(v)), 1)
            row[k + "_range"] = [round(float(min(v)), 1), round(float(max(v)), 1)]
            row[k + "_us"] = round(1e6 / float(np.median(v)), 2)
        if len(rate) == 2:
            row["ratio"] = round(row["clip_steps_per_s"] / row["default_steps_per_s"], 4)
            row["added_us"] = round(row["clip_us"] - row["default_us"], 2)
            row["last_norm_scale"] = [round(x, 6) for x in nets["clip"].last_grad_norm()]
        print(json.dumps(row), flush=True)
