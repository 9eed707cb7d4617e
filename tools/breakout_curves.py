"""Learning curves on the library's game "breakout" (DESIGN.md §20): bricks broken per lost ball, evaluated every 10 000 env-steps of a
200 000-step run, seeds 1, 2, 3, float32, B = 32, for
  envs32               --train_envs 32 (default step)
  envs32_double        ... --double_dqn true
  envs32_nstep3        ... --n_step 3
  envs32_double_nstep3 ... --double_dqn true --n_step 3
  single               one environment (Agent.train, the fused act step)
  single_per           ... --prioritized_replay true (prioritized replay cannot be laned)
next to the same figure of the uniformly random policy (evaluate(..., epsilon=1.0), 24 000 steps, same seeds): the baseline the curves
are read against.  Every evaluation is DeepQNetwork.evaluate on 32 copies, 750 steps each, epsilon 0.05.
    python tools/breakout_curves.py [--steps 200000] [--every 10000] [--seeds 1 2 3] [--configs envs32 single ...] [--out curves.json]
        [--frame_skip K] [--repeat_action_probability P]     the game's dynamics, passed through to every run and evaluation
One JSON line per finished run is appended to --out as it completes (a run cut short leaves what was finished), the table is printed at the end.
Hyper-parameters besides the options above: --replay_size 51200, --exploration_decay_steps 50000 (1 -> 0.1), --target_steps 1000,
--random_steps 3200, --breakout_balls 3, everything else at the command line's defaults."""
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
    "envs32_double": dict(train_envs=32, double_dqn=True),
    "envs32_nstep3": dict(train_envs=32, n_step=3),
    "envs32_double_nstep3": dict(train_envs=32, double_dqn=True, n_step=3),
    "single": dict(train_envs=0),
    "single_per": dict(train_envs=0, prioritized_replay=True),
}
EVAL_COPIES, EVAL_STEPS = 32, 750                                     # 24 000 steps per evaluation


def _args(seed, **kw):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", "breakout"])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_steps, a.random_seed = 51200, 50000, 1000, 3200, seed
    a.batch_size, a.datatype = 32, "float32"
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def bricks_per_ball(net, env, seed, epsilon=0.05):
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    return float(out["caught"].sum()) / max(int(out["missed"].sum()), 1)


def run(name, seed, steps, every, **dynamics):
    import simple_dqn_amd as sd
    a = _args(seed, **dict(CONFIGS[name], **dynamics))
    random.seed(seed)
    env = sd.BreakoutEnvironment(a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(config=name, seed=seed, frame_skip=a.frame_skip, repeat_action_probability=a.repeat_action_probability, random=bricks_per_ball(net, env, seed, 1.0), untrained=bricks_per_ball(net, env, 1000 + seed), curve=[])
    if a.train_envs:
        agent.play_random_vectorised(a.random_steps)
    else:
        agent.play_random(a.random_steps)
    for epoch in range(steps // every):
        if a.train_envs:
            agent.train_vectorised(every, epoch)
        else:
            agent.train(every, epoch)
        rec["curve"].append(((epoch + 1) * every, bricks_per_ball(net, env, 2000 + seed + epoch)))
    rec["seconds"] = time.time() - t0
    return rec


def table(recs):
    by = {}
    for r in recs:
        by.setdefault(r["config"], []).append(r)
    lines = []
    rnd = [r["random"] for r in recs]
    if rnd:
        lines.append("random policy: bricks per lost ball %.3f (min %.3f, max %.3f over %d runs)" % (statistics.mean(rnd), min(rnd), max(rnd), len(rnd)))
    for name, rs in by.items():
        rs.sort(key=lambda r: r["seed"])
        last = [r["curve"][-1][1] for r in rs]
        best = [max(v for _, v in r["curve"]) for r in rs]
        first2x = []
        for r in rs:                                                  # first evaluation at twice the random policy's figure
            hit = [s for s, v in r["curve"] if v >= 2.0 * r["random"]]
            first2x.append(hit[0] if hit else None)
        lines.append("%-22s seeds %s  final %s  (mean %.3f, spread %.3f)  best %s  first >= 2x random at %s"
                     % (name, [r["seed"] for r in rs], ["%.3f" % v for v in last], statistics.mean(last), max(last) - min(last),
                        ["%.3f" % v for v in best], first2x))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=200000)
    p.add_argument("--every", type=int, default=10000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument("--out", default=None)
    p.add_argument("--frame_skip", type=int, default=1)
    p.add_argument("--repeat_action_probability", type=float, default=0.0)
    o = p.parse_args()
    from simple_dqn_amd.main import check_dynamics
    check_dynamics(argparse.Namespace(environment="breakout", frame_skip=o.frame_skip, repeat_action_probability=o.repeat_action_probability))
    recs = []
    for name in o.configs:
        for seed in o.seeds:
            rec = run(name, seed, o.steps, o.every, frame_skip=o.frame_skip, repeat_action_probability=o.repeat_action_probability)
            recs.append(rec)
            print("%s seed %d: random %.3f untrained %.3f final %.3f (%.0f s)" % (name, seed, rec["random"], rec["untrained"],
                                                                                rec["curve"][-1][1], rec["seconds"]), flush=True)
            if o.out:
                with open(o.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
