"""Learning curves of --bootstrap_heads on the library's games freeway and catch: --train_envs 32, seeds 1, 2, 3, float32,
B = 32, K in {1, 6}, evaluated every 10 000 env-steps with DeepQNetwork.evaluate on 32 copies (1 000 agent steps each, epsilon 0.05; the
K = 6 net acts by its heads' vote there).  The figure is the game's `caught` tally per 500 agent steps (freeway: crossings; catch: balls
caught), next to the uniformly random policy's on the same seeds.
    python tools/bootstrap_curves.py [--games freeway catch] [--heads 1 6] [--steps 300000] [--every 10000] [--seeds 1 2 3]
        [--mask_probability 1.0] [--out curves.json]
One JSON line per finished run is appended to --out as it completes; the table is printed at the end.  Hyper-parameters as
tools/freeway_curves.py: --replay_size 51200, --exploration_decay_steps 50000, --target_steps 1000, --random_steps 3200."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EVAL_COPIES, EVAL_STEPS = 32, 1000


def _args(game, seed, heads, P):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", game])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_steps, a.random_seed = 51200, 50000, 1000, 3200, seed
    a.batch_size, a.datatype, a.train_envs, a.bootstrap_heads, a.bootstrap_mask_probability = 32, "float32", 32, heads, P
    return a


def score(net, env, seed, epsilon=0.05):
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    return 500.0 * float(out["caught"].sum()) / float(EVAL_COPIES * EVAL_STEPS)


def run(game, heads, seed, steps, every, P):
    import simple_dqn_amd as sd
    a = _args(game, seed, heads, P)
    random.seed(seed)
    env = {"freeway": sd.FreewayEnvironment, "catch": sd.CatchEnvironment}[game](a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(game=game, heads=heads, mask_probability=P, seed=seed, random=score(net, env, seed, 1.0), curve=[])
    agent.play_random_vectorised(a.random_steps)
    for epoch in range(steps // every):
        agent.train_vectorised(every, epoch)
        rec["curve"].append(((epoch + 1) * every, score(net, env, 2000 + seed + epoch)))
    rec["seconds"] = time.time() - t0
    return rec


def table(recs):
    by, lines = {}, []
    for r in recs:
        by.setdefault((r["game"], r["heads"]), []).append(r)
    for (game, heads), rs in sorted(by.items()):
        rs.sort(key=lambda r: r["seed"])
        last = [statistics.mean(v for _, v in r["curve"][-3:]) for r in rs]      # the plateau: mean of the last three evaluations
        lines.append("%-8s K=%d seeds %s  random %.2f  last-3 mean %s  (mean %.2f, spread %.2f)"
                     % (game, heads, [r["seed"] for r in rs], statistics.mean(r["random"] for r in rs), ["%.2f" % v for v in last],
                        statistics.mean(last), max(last) - min(last)))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--games", nargs="+", default=["freeway", "catch"], choices=["freeway", "catch"])
    p.add_argument("--heads", type=int, nargs="+", default=[1, 6])
    p.add_argument("--steps", type=int, default=300000)
    p.add_argument("--every", type=int, default=10000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--mask_probability", type=float, default=1.0)
    p.add_argument("--out", default=None)
    o = p.parse_args()
    recs = []
    for game in o.games:
        for heads in o.heads:
            for seed in o.seeds:
                rec = run(game, heads, seed, o.steps, o.every, o.mask_probability)
                recs.append(rec)
                print("%s K=%d seed %d: random %.3f curve %s (%.0f s)" % (game, heads, seed, rec["random"], " ".join("%.1f" % v for _, v in rec["curve"]),
                                                                          rec["seconds"]), flush=True)
                if o.out:
                    with open(o.out, "a") as f:
                        f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
