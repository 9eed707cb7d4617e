"""Cost of dormant-neuron recycling (--redo_interval): per datatype (float32, float16) and batch size (32, 256), on one
synthetic-filled ring in one process, alternated: the default step, the same step with redo_interval 1 (an event behind every step: the
difference is one event), and a default step followed by dormant_scores() (the read-out: two launches, a 2.7 KB copy and a wait).  Prints
microseconds per step of each and the differences (median of the alternated rounds); --out writes the lines as a JSON list."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=5, help="alternated rounds")
ap.add_argument("--size", type=int, default=20000, help="replay slots")
ap.add_argument("--out", help="write the result lines here as a JSON list")
a = ap.parse_args()
lines = []
for dt in ("float32", "float16"):
    for B in (32, 256):
        args = make_args(batch_size=B, datatype=dt)
        mem = sd.ReplayMemory(a.size, args)
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        nets = {"default": sd.DeepQNetwork(4, args), "event": sd.DeepQNetwork(4, make_args(batch_size=B, datatype=dt, redo_interval=1)),
                "default1": sd.DeepQNetwork(4, args), "scores": sd.DeepQNetwork(4, args)}

        def run(k, n):
            if k in ("default", "event"):
                nets[k].train_from_memory(mem, n)              # one call, no wait between the steps
            else:
                for _ in range(n):                             # step by step, each waited for: the read-out's own baseline
                    nets[k].train_from_memory(mem, 1)
                    if k == "scores":
                        nets[k].dormant_scores()
            nets[k].sync()
        us = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k in nets:
                run(k, 10)
                t0 = time.perf_counter()
                run(k, a.steps)
                if r:                                          # (round 0 warms the code objects and the caches up)
                    us[k].append(1e6 * (time.perf_counter() - t0) / a.steps)
        m = {k: float(np.median(v)) for k, v in us.items()}
        line = {"datatype": dt, "batch_size": B, "rounds": a.rounds, "steps": a.steps, "default_us": round(m["default"], 2),
                "step_plus_event_us": round(m["event"], 2), "event_us": round(m["event"] - m["default"], 2),
                "waited_step_us": round(m["default1"], 2), "waited_step_plus_scores_us": round(m["scores"], 2),
                "scores_us": round(m["scores"] - m["default1"], 2), "last_event": nets["event"].last_redo()}
        lines.append(line)
        print(json.dumps(line), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
