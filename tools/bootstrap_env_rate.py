"""Price of the select launch of --bootstrap_heads: train-phase env-steps/s of Agent.train_vectorised at --train_envs 32 on a
library game, K = 6 against K = 1, float32, B = 32, alternated in one process, median of the rounds (the method of tools/env_rate.py
--train_envs).  The K = 6 phase differs in two places: one more launch per lockstep (bootstrap_select_kernel) and the bootstrap head in
its train steps.
    python tools/bootstrap_env_rate.py [--environment catch] [--heads 1 6] [--rounds 7] [--train_steps 16384] [--json out.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(game, heads):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", game])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_seed = 20000, 10000, 500, 1
    a.train_envs, a.batch_size, a.bootstrap_heads = 32, 32, heads
    return a


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--environment", default="catch", choices=["catch", "freeway"])
    p.add_argument("--heads", type=int, nargs="+", default=[1, 6])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--train_steps", type=int, default=16384)
    p.add_argument("--json", default=None)
    o = p.parse_args()
    import simple_dqn_amd as sd
    from simple_dqn_amd.environment import LIBRARY_GAMES
    agents = {}
    for K in o.heads:
        a = _args(o.environment, K)
        random.seed(1)
        env = LIBRARY_GAMES[o.environment](a, seed=1)
        mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
        ag = sd.Agent(env, mem, net, a)
        ag.play_random_vectorised(2000); ag.train_vectorised(1024)
        net.sync()
        agents[K] = (ag, net)
    rates = dict((K, []) for K in o.heads)
    for _ in range(o.rounds):
        for K, (ag, net) in agents.items():
            t0 = time.perf_counter()
            ag.train_vectorised(o.train_steps)
            net.sync()
            rates[K].append(o.train_steps / (time.perf_counter() - t0))
    out = {"environment": o.environment, "train_envs": 32, "rounds": o.rounds, "train_steps": o.train_steps}
    for K, r in rates.items():
        out["heads_%d" % K] = dict(env_steps_per_s=round(statistics.median(r), 1), min=round(min(r), 1), max=round(max(r), 1))
    base = out["heads_%d" % o.heads[0]]["env_steps_per_s"]
    for K in o.heads[1:]:
        out["heads_%d" % K]["ratio"] = round(out["heads_%d" % K]["env_steps_per_s"] / base, 4)
    print(json.dumps(out), flush=True)
    if o.json:
        with open(o.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
