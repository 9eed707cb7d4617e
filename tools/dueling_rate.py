"""Cost of --dueling: a standard 4-action net and a dueling net over 3 actions (4 outputs) — the same forward and backward
launches; the head and the optimizer tail differ — trained alternately in one process with train_from_memory on a synthetic-filled ring,
float32 at B = 32 and B = 256.  Prints steps/s of both and their ratio per batch size (median of the alternated rounds) and, with
--clipped, of a standard net under --clip_grad_norm 10 as well: the same split tail with two clip launches where dueling has one mask
launch.  --out appends the lines to a file."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
    ap.add_argument("--rounds", type=int, default=7, help="alternated (standard, dueling) rounds")
    ap.add_argument("--batch", type=int, help="one batch size only")
    ap.add_argument("--clipped", action="store_true", help="a third net: standard under --clip_grad_norm 10")
    ap.add_argument("--net", choices=["all", "standard", "dueling"], default="all", help="one net only (a kernel trace of each form)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for B in ([a.batch] if a.batch else [32, 256]):
        mem = sd.ReplayMemory(20000, make_args(batch_size=B))
        synthetic_fill(mem, 1, num_actions=3)                    # actions < 3: valid for every net
        mem.sync_mirror()
        make = {"standard": lambda: sd.DeepQNetwork(4, make_args(batch_size=B)),
                "dueling": lambda: sd.DeepQNetwork(3, make_args(batch_size=B, dueling=True))}
        if a.clipped:
            make["clipped"] = lambda: sd.DeepQNetwork(4, make_args(batch_size=B, clip_grad_norm=10.0))
        nets = {k: make[k]() for k in make if a.net in ("all", k)}
        rate = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k, net in nets.items():
                net.train_from_memory(mem, 10); net.sync()
                t0 = time.perf_counter()
                net.train_from_memory(mem, a.steps); net.sync()
                if r:                                            # (round 0 warms the code objects and the caches up)
                    rate[k].append(a.steps / (time.perf_counter() - t0))
        out = {"batch_size": B, "rounds": a.rounds}
        for k in nets:
            out[k + "_steps_per_s"] = round(float(np.median(rate[k])), 1); out[k + "_us"] = round(1e6 / float(np.median(rate[k])), 2)
            out[k + "_all"] = [round(x, 1) for x in rate[k]]
        if "standard" in nets and "dueling" in nets:
            out["ratio"] = round(out["dueling_steps_per_s"] / out["standard_steps_per_s"], 4)
        if "clipped" in nets and "dueling" in nets:
            out["ratio_to_clipped"] = round(out["dueling_steps_per_s"] / out["clipped_steps_per_s"], 4)
        print(json.dumps(out), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
