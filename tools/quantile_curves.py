"""Learning curves of --quantiles on catch: what tests/test_gpu_quantile_learning.py's budget is set from.  That test's
loop and hyper-parameters (tests/test_gpu_catch.py: LEARN, with --train_envs 32 --eval_envs 32), seeds 1, 2, 3, N in {1, 6}, evaluated by
its criterion every 5 000 of 60 000 env-steps; `first_crossing` is the first evaluation at or above the midpoint between the random
policy's reward per ball and +1 (null: none within the horizon).
    python tools/quantile_curves.py [--quantiles 1 6] [--seeds 1 2 3] [--steps 60000] [--every 5000] [--out curves.json]
One JSON line per finished run is appended to --out as it completes; the table is printed at the end."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def crossing(N, seed, steps, every):
    """the learning test's loop (tests/test_gpu_catch.py: learning_run) with an evaluation after every epoch"""
    import simple_dqn_amd as sd
    from test_gpu_catch import LEARN, _args as targs, _midpoint, per_ball
    a = targs(random_seed=seed, epochs=steps // every, train_steps=every, train_envs=32, eval_envs=32, quantiles=N, **LEARN)
    random.seed(seed)
    env = sd.CatchEnvironment(a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(3, a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(game="catch", quantiles=N, seed=seed, midpoint=_midpoint(), untrained=per_ball(net, env, 1000 + seed), curve=[])
    agent.play_random_vectorised(a.random_steps)
    for epoch in range(a.epochs):
        agent.train_vectorised(every, epoch)
        rec["curve"].append(((epoch + 1) * every, per_ball(net, env, 2000 + seed + epoch)))
    rec["first_crossing"] = next((s for s, v in rec["curve"] if v >= rec["midpoint"]), None)
    rec["seconds"] = time.time() - t0
    return rec


def table(recs):
    by, lines = {}, []
    for r in recs:
        by.setdefault(r["quantiles"], []).append(r)
    for N, rs in sorted(by.items()):
        rs.sort(key=lambda r: r["seed"])
        lines.append("catch N=%d seeds %s  midpoint %.3f  first crossing %s  last %s" % (N, [r["seed"] for r in rs], rs[0]["midpoint"],
                                                                                   [r["first_crossing"] for r in rs], ["%.2f" % r["curve"][-1][1] for r in rs]))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--quantiles", type=int, nargs="+", default=[1, 6])
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--steps", type=int, default=60000)
    p.add_argument("--every", type=int, default=5000)
    p.add_argument("--out", default=None)
    o = p.parse_args()
    recs = []
    for N in o.quantiles:
        for seed in o.seeds:
            rec = crossing(N, seed, o.steps, o.every)
            recs.append(rec)
            print("catch N=%d seed %d: untrained %.2f curve %s (%.0f s)" % (N, seed, rec["untrained"], " ".join("%.2f" % v for _, v in rec["curve"]), rec["seconds"]), flush=True)
            if o.out:
                with open(o.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
