"""Rate of Agent.train_offline: learns per second at offline_chunk 64 and 1, with --cql_alpha 0 and 1, float32 B = 32, on a
synthetic-filled 20 000-slot ring with no callback installed (a callback makes train_from_memory report every step's cost one by one).
5 rounds of 3 200 learns after 640 of warm-up, median; --out writes profiles/offline_rate.json."""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import simple_dqn_amd as sd
from oracle.replay_numpy import synthetic_fill
from util import make_args

ap = argparse.ArgumentParser()
ap.add_argument("--learns", type=int, default=3200, help="learns per timed call")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", help="write the record to this JSON file")
a = ap.parse_args()


class Env:
    def numActions(self):
        return 4


cells = {}
for alpha in (0.0, 1.0):
    for chunk in (64, 1):
        args = make_args(batch_size=32, cql_alpha=alpha, target_steps=10000)
        mem = sd.ReplayMemory(20000, args); synthetic_fill(mem, 1, num_actions=4); mem.sync_mirror()
        net = sd.DeepQNetwork(4, args)
        agent = sd.Agent(Env(), mem, net, args, offline_chunk=chunk)
        random.seed(1)
        agent.train_offline(640); net.sync()
        rates = []
        for r in range(a.rounds):
            t0 = time.perf_counter(); agent.train_offline(a.learns); net.sync()
            rates.append(a.learns / (time.perf_counter() - t0))
        key = "alpha%g_chunk%d" % (alpha, chunk)
        cells[key] = {"median_learns_per_s": round(sorted(rates)[len(rates) // 2], 1), "all": [round(x, 1) for x in rates]}
        print(json.dumps({key: cells[key]}), flush=True)
if a.out:
    rec = {"what": "learns per second of Agent.train_offline (no callback installed), float32 B = 32, synthetic-filled 20 000-slot ring, "
                   "%d rounds of %d learns (tools/offline_rate.py)" % (a.rounds, a.learns), "cells": cells}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
