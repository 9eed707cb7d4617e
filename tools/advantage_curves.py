"""Learning curves of --advantage_learning / --persistent_advantage on the library's games catch, breakout and freeway:
--train_envs 32, seeds 1, 2, 3, float32, B = 32, the standard step (alpha 0) against AL and PAL at alpha 0.9, evaluated as
tools/bootstrap_curves.py evaluates: every 10 000 env-steps with DeepQNetwork.evaluate on 32 copies (1 000 agent steps each, epsilon 0.05);
the figure is the game's `caught` tally per 500 agent steps, next to the uniformly random policy's on the same seeds.
    python tools/advantage_curves.py [--games catch breakout freeway] [--forms std al pal] [--alpha 0.9] [--steps 300000] [--every 10000]
        [--seeds 1 2 3] [--out curves.json]
    python tools/advantage_curves.py --crossing [--forms al] [--seeds 1 2 3] [--out crossings.json]
--crossing measures what tests/test_gpu_advantage_learning_curve.py's budget is set from: that test's loop and hyper-parameters on catch
(tests/test_gpu_catch.py: LEARN, --train_envs 32), evaluated by its criterion every 5 000 of 60 000 env-steps; `first_crossing` is the first
evaluation at or above the midpoint between the random policy's reward per ball and +1 (null: none).
One JSON line per finished run is appended to --out as it completes; the table is printed at the end.  Hyper-parameters of the curves as
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
EVAL_COPIES, EVAL_STEPS = 32, 1000
FORMS = {"std": (0.0, False), "al": (None, False), "pal": (None, True)}      # (alpha; None: --alpha, persistent)


def _form(form, alpha):
    a, pal = FORMS[form]
    return (alpha if a is None else a), pal


def _args(game, seed, alpha, pal):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", game])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_steps, a.random_seed = 51200, 50000, 1000, 3200, seed
    a.batch_size, a.datatype, a.train_envs, a.advantage_learning, a.persistent_advantage = 32, "float32", 32, alpha, pal
    return a


def score(net, env, seed, epsilon=0.05):
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    return 500.0 * float(out["caught"].sum()) / float(EVAL_COPIES * EVAL_STEPS)


def run(game, form, alpha, seed, steps, every):
    import simple_dqn_amd as sd
    al, pal = _form(form, alpha)
    a = _args(game, seed, al, pal)
    random.seed(seed)
    env = {"freeway": sd.FreewayEnvironment, "catch": sd.CatchEnvironment, "breakout": sd.BreakoutEnvironment}[game](a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(game=game, form=form, alpha=al, persistent=pal, seed=seed, random=score(net, env, seed, 1.0), curve=[])
    agent.play_random_vectorised(a.random_steps)
    for epoch in range(steps // every):
        agent.train_vectorised(every, epoch)
        rec["curve"].append(((epoch + 1) * every, score(net, env, 2000 + seed + epoch)))
    rec["seconds"] = time.time() - t0
    return rec


def crossing(form, alpha, seed, steps=60000, every=5000):
    """the learning test's loop (tests/test_gpu_catch.py: learning_run with --train_envs 32) with an evaluation after every epoch"""
    import simple_dqn_amd as sd
    from test_gpu_catch import LEARN, _args as targs, _midpoint, per_ball
    al, pal = _form(form, alpha)
    a = targs(random_seed=seed, epochs=steps // every, train_steps=every, train_envs=32, advantage_learning=al, persistent_advantage=pal, **LEARN)
    random.seed(seed)
    env = sd.CatchEnvironment(a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(3, a)
    agent = sd.Agent(env, mem, net, a)
    t0 = time.time()
    rec = dict(game="catch", form=form, alpha=al, persistent=pal, seed=seed, midpoint=_midpoint(), untrained=per_ball(net, env, 1000 + seed), curve=[])
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
        by.setdefault((r["game"], r["form"]), []).append(r)
    for (game, form), rs in sorted(by.items()):
        rs.sort(key=lambda r: r["seed"])
        if "first_crossing" in rs[0]:
            lines.append("%-8s %-3s seeds %s  midpoint %.3f  first crossing %s" % (game, form, [r["seed"] for r in rs], rs[0]["midpoint"],
                                                                                 [r["first_crossing"] for r in rs]))
            continue
        last = [statistics.mean(v for _, v in r["curve"][-3:]) for r in rs]      # the plateau: mean of the last three evaluations
        lines.append("%-8s %-3s seeds %s  random %.2f  last-3 mean %s  (mean %.2f, spread %.2f)  best %s"
                     % (game, form, [r["seed"] for r in rs], statistics.mean(r["random"] for r in rs), ["%.2f" % v for v in last],
                        statistics.mean(last), max(last) - min(last), ["%.2f" % max(v for _, v in r["curve"]) for r in rs]))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--games", nargs="+", default=["catch", "breakout", "freeway"], choices=["catch", "breakout", "freeway"])
    p.add_argument("--forms", nargs="+", default=None, choices=list(FORMS))
    p.add_argument("--alpha", type=float, default=0.9)
    p.add_argument("--steps", type=int, default=300000)
    p.add_argument("--every", type=int, default=10000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--crossing", action="store_true")
    p.add_argument("--out", default=None)
    o = p.parse_args()
    forms = o.forms or (["al"] if o.crossing else ["std", "al", "pal"])
    recs = []
    for game in (["catch"] if o.crossing else o.games):
        for form in forms:
            for seed in o.seeds:
                rec = crossing(form, o.alpha, seed) if o.crossing else run(game, form, o.alpha, seed, o.steps, o.every)
                recs.append(rec)
                print("%s %s seed %d: curve %s (%.0f s)" % (game, form, seed, " ".join("%.2f" % v for _, v in rec["curve"]), rec["seconds"]), flush=True)
                if o.out:
                    with open(o.out, "a") as f:
                        f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
