"""Cost of --munchausen: a standard net and a Munchausen net trained alternately in one process with train_from_memory
(the fused replay loop of the Agent path) on a synthetic-filled ring, at B = 32 and B = 256 in float32 and float16.  Prints steps/s of
both and their ratio per configuration (median of the alternated rounds)."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated (standard, Munchausen) rounds")
ap.add_argument("--datatype", choices=["float32", "float16"], help="one datatype only")
ap.add_argument("--batch", type=int, help="one batch size only")
ap.add_argument("--net", choices=["both", "standard", "munchausen"], default="both", help="one net only (a kernel trace of each form)")
a = ap.parse_args()
for dt in ([a.datatype] if a.datatype else ["float32", "float16"]):
    for B in ([a.batch] if a.batch else [32, 256]):
        args = make_args(batch_size=B, datatype=dt)
        mem = sd.ReplayMemory(20000, args)
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        nets = {k: sd.DeepQNetwork(4, make_args(batch_size=B, datatype=dt, munchausen=k == "munchausen")) for k in ("standard", "munchausen")
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
        s, d = float(np.median(rate["standard"])), float(np.median(rate["munchausen"]))
        print(json.dumps({"datatype": dt, "batch_size": B, "standard_steps_per_s": round(s, 1), "munchausen_steps_per_s": round(d, 1),
                          "ratio": round(d / s, 4), "standard_us": round(1e6 / s, 2), "munchausen_us": round(1e6 / d, 2),
                          "standard_all": [round(x, 1) for x in rate["standard"]], "munchausen_all": [round(x, 1) for x in rate["munchausen"]]}), flush=True)
