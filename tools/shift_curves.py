"""Learning curves with --random_shift on the library's game "breakout" (DESIGN.md §34): summed reward per finished episode, evaluated every
10 000 env-steps of a run, seeds 1, 2, 3, float32, B = 32, --train_envs 32, for --random_shift 0, 2 and 4, next to the same figure of the
uniformly random policy and of the untrained network.  Every evaluation is DeepQNetwork.evaluate on 32 copies, 1 000 agent steps each,
epsilon 0.05 (never shifted: the option acts on train steps only).
    python tools/shift_curves.py [--steps 300000] [--every 10000] [--seeds 1 2 3] [--shifts 0 2 4] [--environment breakout] [--out curves.json]
One JSON line per finished run is appended to --out as it completes, the table is printed at the end.  Hyper-parameters besides the
option: --replay_size 51200, --exploration_decay_steps 50000 (1 -> 0.1), --target_steps 1000, --random_steps 3200, everything else at the
command line's defaults (tools/freeway_curves.py's)."""
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


def _args(game, seed, shift):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", game])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_steps, a.random_seed = 51200, 50000, 1000, 3200, seed
    a.batch_size, a.datatype, a.train_envs, a.random_shift = 32, "float32", 32, shift
    return a


def per_episode(net, env, seed, epsilon=0.05):
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    return float(out["reward"].sum()) / max(1.0, float(out["episodes"].sum()))


def run(game, shift, seed, steps, every):
    import simple_dqn_amd as sd
    from simple_dqn_amd.environment import LIBRARY_GAMES
    a = _args(game, seed, shift)
    random.seed(seed)
    env = LIBRARY_GAMES[game](a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(environment=game, random_shift=shift, seed=seed, random=per_episode(net, env, seed, 1.0), untrained=per_episode(net, env, 1000 + seed), curve=[])
    agent.play_random_vectorised(a.random_steps)
    for epoch in range(steps // every):
        agent.train_vectorised(every, epoch)
        rec["curve"].append(((epoch + 1) * every, per_episode(net, env, 2000 + seed + epoch)))
    rec["shifted_steps"], rec["seconds"] = net.random_shift_steps(), time.time() - t0
    return rec


def table(recs):
    by = {}
    for r in recs:
        by.setdefault(r["random_shift"], []).append(r)
    lines = []
    for shift, rs in sorted(by.items()):
        rs.sort(key=lambda r: r["seed"])
        last = [statistics.mean(v for _, v in r["curve"][-3:]) for r in rs]      # the plateau: mean of the last three evaluations
        lines.append("random_shift %d  seeds %s  last-3 mean %s  (mean %.2f, spread %.2f)  best %s"
                     % (shift, [r["seed"] for r in rs], ["%.2f" % v for v in last], statistics.mean(last), max(last) - min(last),
                        ["%.2f" % max(v for _, v in r["curve"]) for r in rs]))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300000)
    p.add_argument("--every", type=int, default=10000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--shifts", type=int, nargs="+", default=[0, 2, 4])
    p.add_argument("--environment", default="breakout", choices=["catch", "breakout", "freeway"])
    p.add_argument("--out", default=None)
    o = p.parse_args()
    recs = []
    for shift in o.shifts:
        for seed in o.seeds:
            rec = run(o.environment, shift, seed, o.steps, o.every)
            recs.append(rec)
            print("random_shift %d seed %d: random %.3f untrained %.3f curve %s (%.0f s)" % (shift, seed, rec["random"], rec["untrained"],
                                                                                            " ".join("%.2f" % v for _, v in rec["curve"]), rec["seconds"]), flush=True)
            if o.out:
                with open(o.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
