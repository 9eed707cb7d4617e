"""Cost of --noisy_nets: a plain 4-action net and a noisy one — the same forward, backward and head launches; the noisy step
runs the split optimizer tail plus its compose, sigma and compose launches — trained alternately in one process with train_from_memory
on a synthetic-filled ring, float32 at B = 32 and B = 256.  Prints steps/s of both per batch size (median, min .. max of the alternated
rounds) and their ratio and, with --clipped, of a plain net under --clip_grad_norm 10 as well: the same split tail with two clip launches
where the noisy step has three of its own.  --net noisy runs that net alone (a kernel trace).  --out appends the lines to a file."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
    ap.add_argument("--rounds", type=int, default=7, help="alternated (plain, noisy) rounds")
    ap.add_argument("--batch", type=int, help="one batch size only")
    ap.add_argument("--clipped", action="store_true", help="a third net: plain under --clip_grad_norm 10")
    ap.add_argument("--net", choices=["all", "plain", "noisy"], default="all", help="one net only (a kernel trace of each form)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for B in ([a.batch] if a.batch else [32, 256]):
        mem = sd.ReplayMemory(20000, make_args(batch_size=B))
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        make = {"plain": lambda: sd.DeepQNetwork(4, make_args(batch_size=B)),
                "noisy": lambda: sd.DeepQNetwork(4, make_args(batch_size=B, noisy_nets=True, noisy_sigma=0.5))}
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
            out[k + "_min_max"] = [round(min(rate[k]), 1), round(max(rate[k]), 1)]
        if "plain" in nets and "noisy" in nets:
            out["ratio"] = round(out["noisy_steps_per_s"] / out["plain_steps_per_s"], 4)
            out["added_us"] = round(out["noisy_us"] - out["plain_us"], 2)
        if "clipped" in nets and "noisy" in nets:
            out["added_us_over_clipped"] = round(out["noisy_us"] - out["clipped_us"], 2)
        print(json.dumps(out), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
