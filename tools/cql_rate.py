"""Cost of --cql_alpha: a standard net and a CQL net (alpha 1) trained alternately in one process with train_from_memory
(the fused replay loop of the Agent path) on a synthetic-filled ring, at B = 32 and B = 256 in float32 and float16.  The CQL step launches
what the standard step launches; the difference is the head's softmax.  Prints steps/s of the two and the ratio CQL / standard per
configuration (median of the alternated rounds); --out collects the records into a JSON file (profiles/cql_rate.json)."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200, help="train steps per timed call")
ap.add_argument("--rounds", type=int, default=7, help="alternated (standard, CQL) rounds")
ap.add_argument("--datatype", choices=["float32", "float16"], help="one datatype only")
ap.add_argument("--batch", type=int, help="one batch size only")
ap.add_argument("--net", choices=["all", "standard", "cql"], default="all", help="one net only (a kernel trace of each form)")
ap.add_argument("--out", help="write the records to this JSON file")
a = ap.parse_args()
KW = {"standard": {}, "cql": dict(cql_alpha=1.0)}
records = []
for dt in ([a.datatype] if a.datatype else ["float32", "float16"]):
    for B in ([a.batch] if a.batch else [32, 256]):
        args = make_args(batch_size=B, datatype=dt)
        mem = sd.ReplayMemory(20000, args)
        synthetic_fill(mem, 1, num_actions=4)
        mem.sync_mirror()
        nets = {k: sd.DeepQNetwork(4, make_args(batch_size=B, datatype=dt, **kw)) for k, kw in KW.items() if a.net in ("all", k)}
        rate = {k: [] for k in nets}
        random.seed(1)
        for r in range(a.rounds + 1):
            for k, net in nets.items():
                net.train_from_memory(mem, 10); net.sync()
                t0 = time.perf_counter()
                net.train_from_memory(mem, a.steps); net.sync()
                if r:                                        # (round 0 warms the code objects and the caches up)
                    rate[k].append(a.steps / (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in rate.items()}
        rec = {"datatype": dt, "batch_size": B, "steps": a.steps, "rounds": a.rounds}
        for k, v in med.items():
            rec[k + "_steps_per_s"], rec[k + "_us"], rec[k + "_all"] = round(v, 1), round(1e6 / v, 2), [round(x, 1) for x in rate[k]]
        if a.net == "all":
            rec["ratio_to_standard"] = round(med["cql"] / med["standard"], 4)
        print(json.dumps(rec), flush=True)
        records.append(rec)
if a.out:
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)
