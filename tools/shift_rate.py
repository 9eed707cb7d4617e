"""Cost of --random_shift: a default net, a net with random_shift 4 and (for scale) the tuple path net.train(mem.getMinibatch()) reading the
device minibatch in place, trained alternately in one process on one synthetic-filled ring, float32 at B = 32 and B = 256.  The first two go
through train_from_memory (the fused replay loop of the Agent path).  Prints steps/s of each and the ratios per configuration (median of
the alternated rounds); --out writes the lines as a JSON list."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated rounds")
ap.add_argument("--shift", type=int, default=4, help="the P of the shifted net")
ap.add_argument("--batch", type=int, help="one batch size only")
ap.add_argument("--size", type=int, default=20000, help="replay slots")
ap.add_argument("--out", help="write the result lines here as a JSON list")
a = ap.parse_args()
lines = []
for B in ([a.batch] if a.batch else [32, 256]):
    args = make_args(batch_size=B)
    mem = sd.ReplayMemory(a.size, args)
    synthetic_fill(mem, 1, num_actions=4)
    mem.sync_mirror()
    nets = {"default": sd.DeepQNetwork(4, args), "shift": sd.DeepQNetwork(4, make_args(batch_size=B, random_shift=a.shift)),
            "tuple": sd.DeepQNetwork(4, args)}

    def run(k, n):
        if k == "tuple":
            for _ in range(n):
                nets[k].train(mem.getMinibatch())
        else:
            nets[k].train_from_memory(mem, n)
        nets[k].sync()
    rate = {k: [] for k in nets}
    random.seed(1)
    for r in range(a.rounds + 1):
        for k in nets:
            run(k, 10)
            t0 = time.perf_counter()
            run(k, a.steps)
            if r:                                            # (round 0 warms the code objects and the caches up)
                rate[k].append(a.steps / (time.perf_counter() - t0))
    m = {k: float(np.median(v)) for k, v in rate.items()}
    line = {"datatype": "float32", "batch_size": B, "random_shift": a.shift, "rounds": a.rounds, "steps": a.steps,
            "default_steps_per_s": round(m["default"], 1), "shift_steps_per_s": round(m["shift"], 1), "tuple_steps_per_s": round(m["tuple"], 1),
            "shift_over_default": round(m["shift"] / m["default"], 4), "shift_over_tuple": round(m["shift"] / m["tuple"], 4),
            "default_us": round(1e6 / m["default"], 2), "shift_us": round(1e6 / m["shift"], 2), "tuple_us": round(1e6 / m["tuple"], 2)}
    lines.append(line)
    print(json.dumps(line), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
