"""Learning curves on the library's game "freeway" (DESIGN.md §25): crossings per 500 game ticks, evaluated every 10 000 env-steps of a
run, seeds 1, 2, 3, float32, B = 32, --train_envs 32, for
  envs32               the default step
  envs32_nstep3        ... --n_step 3
  envs32_double        ... --double_dqn true
  envs32_munchausen    ... --munchausen true
next to the same figure of the uniformly random policy (evaluate(..., epsilon=1.0), same seeds) and of the untrained network: the
baselines the curves are read against.  Every evaluation is DeepQNetwork.evaluate on 32 copies, 1 000 agent steps each (64 episodes
of 500 ticks at --frame_skip 1), epsilon 0.05; `hits` is the chicken's hits per 500 ticks in the same evaluation.
    python tools/freeway_curves.py [--steps 300000] [--every 10000] [--seeds 1 2 3] [--configs envs32 ...] [--out curves.json]
        [--frame_skip K] [--repeat_action_probability P]     the game's dynamics, passed through to every run and evaluation
One JSON line per finished run is appended to --out as it completes (a run cut short leaves what was finished), the table is printed at the end.
Hyper-parameters besides the options above: --replay_size 51200, --exploration_decay_steps 50000 (1 -> 0.1), --target_steps 1000,
--random_steps 3200, --freeway_ticks 500, everything else at the command line's defaults."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "envs32": dict(train_envs=32),
    "envs32_nstep3": dict(train_envs=32, n_step=3),
    "envs32_double": dict(train_envs=32, double_dqn=True),
    "envs32_munchausen": dict(train_envs=32, munchausen=True),
}
EVAL_COPIES, EVAL_STEPS = 32, 1000


def _args(seed, **kw):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", "freeway"])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_steps, a.random_seed = 51200, 50000, 1000, 3200, seed
    a.batch_size, a.datatype = 32, "float32"
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def per_500_ticks(net, env, seed, epsilon=0.05):
    """(crossings, hits) per 500 game ticks; the ticks played are counted from the tallies: an episode is `balls_per_episode` ticks"""
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    ticks = float(EVAL_COPIES * EVAL_STEPS * env.frame_skip)          # (an upper bound when a terminal cuts an agent step short)
    return 500.0 * float(out["caught"].sum()) / ticks, 500.0 * float(out["missed"].sum()) / ticks


def run(name, seed, steps, every, **dynamics):
    import simple_dqn_amd as sd
    a = _args(seed, **dict(CONFIGS[name], **dynamics))
    random.seed(seed)
    env = sd.FreewayEnvironment(a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(config=name, seed=seed, frame_skip=a.frame_skip, repeat_action_probability=a.repeat_action_probability,
               random=per_500_ticks(net, env, seed, 1.0)[0], untrained=per_500_ticks(net, env, 1000 + seed)[0], curve=[], hits=[])
    agent.play_random_vectorised(a.random_steps)
    for epoch in range(steps // every):
        agent.train_vectorised(every, epoch)
        c, h = per_500_ticks(net, env, 2000 + seed + epoch)
        rec["curve"].append(((epoch + 1) * every, c)); rec["hits"].append(h)
    rec["seconds"] = time.time() - t0
    return rec


def table(recs):
    by = {}
    for r in recs:
        by.setdefault(r["config"], []).append(r)
    lines = []
    rnd = [r["random"] for r in recs]
    if rnd:
        lines.append("random policy: crossings per 500 ticks %.3f (min %.3f, max %.3f over %d runs)" % (statistics.mean(rnd), min(rnd), max(rnd), len(rnd)))
    for name, rs in by.items():
        rs.sort(key=lambda r: r["seed"])
        last = [statistics.mean(v for _, v in r["curve"][-3:]) for r in rs]      # the plateau: mean of the last three evaluations
        best = [max(v for _, v in r["curve"]) for r in rs]
        lines.append("%-20s seeds %s  last-3 mean %s  (mean %.2f, spread %.2f)  best %s"
                     % (name, [r["seed"] for r in rs], ["%.2f" % v for v in last], statistics.mean(last), max(last) - min(last),
                        ["%.2f" % v for v in best]))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300000)
    p.add_argument("--every", type=int, default=10000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument("--out", default=None)
    p.add_argument("--frame_skip", type=int, default=1)
    p.add_argument("--repeat_action_probability", type=float, default=0.0)
    o = p.parse_args()
    from simple_dqn_amd.main import check_dynamics
    check_dynamics(argparse.Namespace(environment="freeway", frame_skip=o.frame_skip, repeat_action_probability=o.repeat_action_probability))
    recs = []
    for name in o.configs:
        for seed in o.seeds:
            rec = run(name, seed, o.steps, o.every, frame_skip=o.frame_skip, repeat_action_probability=o.repeat_action_probability)
            recs.append(rec)
            print("%s seed %d: random %.3f untrained %.3f curve %s (%.0f s)" % (name, seed, rec["random"], rec["untrained"],
                                                                               " ".join("%.1f" % v for _, v in rec["curve"]), rec["seconds"]), flush=True)
            if o.out:
                with open(o.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
