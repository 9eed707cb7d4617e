"""Cost of --n_step: a standard net on a standard memory and an n = 3 net on an n = 3 memory trained alternately in one process with
train_from_memory (the fused replay loop of the Agent path) on a synthetic-filled ring, at B = 32 and B = 256 in float32 and float16, plus
one row with both memories prioritized (float32, B = 32).  Prints steps/s of both and their ratio per configuration (median of the
alternated rounds)."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated (standard, n-step) rounds")
ap.add_argument("--n", type=int, default=3, help="n_step of the second net")
a = ap.parse_args()
PER = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6)
rows = [("float32", 32, {}), ("float32", 256, {}), ("float16", 32, {}), ("float16", 256, {}), ("float32", 32, PER)]
for dt, B, extra in rows:
    mems, nets = {}, {}
    for k, n in (("standard", 1), ("nstep", a.n)):
        args = make_args(batch_size=B, datatype=dt, n_step=n, **extra)
        mems[k] = sd.ReplayMemory(20000, args)
        synthetic_fill(mems[k], 1, num_actions=4)
        mems[k].sync_mirror()
        nets[k] = sd.DeepQNetwork(4, args)
    rate = {k: [] for k in nets}
    random.seed(1)
    for r in range(a.rounds + 1):
        for k, net in nets.items():
            net.train_from_memory(mems[k], 10); net.sync()
            t0 = time.perf_counter()
            net.train_from_memory(mems[k], a.steps); net.sync()
            if r:                                        # (round 0 warms the code objects and the caches up)
                rate[k].append(a.steps / (time.perf_counter() - t0))
    s, d = float(np.median(rate["standard"])), float(np.median(rate["nstep"]))
    print(json.dumps({"datatype": dt, "batch_size": B, "prioritized": bool(extra), "n_step": a.n, "standard_steps_per_s": round(s, 1),
                      "nstep_steps_per_s": round(d, 1), "ratio": round(d / s, 4), "standard_us": round(1e6 / s, 2),
                      "nstep_us": round(1e6 / d, 2)}), flush=True)
