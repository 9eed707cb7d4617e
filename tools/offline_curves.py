"""Offline training curves, --offline_replay with --cql_alpha 0 and 1, on the library's games catch and freeway.  A dataset
is a replay memory of 20 000 transitions written by main.run's single-environment Agent loop with --save_replay: `random` is random play
only (--random_steps 20000), `online` the replay of a short online run (--random_steps 1000, one epoch of 19 000 training steps; the
hyper-parameters of tests/test_gpu_catch.py's learning test).  One dataset per (game, kind, seed).  Each run then loads its dataset,
collects nothing and trains with Agent.train_offline, float32, B = 32, the target net refreshed every 500 learns, evaluated every --every
learns with DeepQNetwork.evaluate on 32 copies (1 000 agent steps each, epsilon 0.05); the figure is the game's `caught` tally per 500
agent steps, next to the uniformly random policy's on the same seed.
    python tools/offline_curves.py [--games catch freeway] [--datasets random online] [--alphas 0 1] [--learns 40000] [--every 4000]
        [--seeds 1 2 3] [--out curves.json]
    python tools/offline_curves.py --crossing [--alphas 1 0] [--seeds 1 2 3] [--out crossings.json]
--crossing measures what tests/test_gpu_offline_learning.py's budget is set from: catch, the random-play dataset, evaluated by
tests/test_gpu_catch.py's criterion every 2 000 of 40 000 learns; `first_crossing` is the first evaluation at or above the midpoint
between the random policy's reward per ball and +1 (null: none).
One JSON line per finished run is appended to --out as it completes; the table is printed at the end."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
EVAL_COPIES, EVAL_STEPS, SIZE = 32, 1000, 20000
_DATASETS = {}


def _base(game, seed, **kw):
    """the learning test's hyper-parameters (tests/test_gpu_catch.py: LEARN) on `game`"""
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", game])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_seed, a.test_steps = SIZE, 10000, 500, seed, 0
    a.batch_size, a.datatype, a.log_level = 32, "float32", "WARNING"
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def dataset(game, kind, seed, folder):
    """the file of (game, kind, seed), written once per process by main.run --save_replay"""
    from simple_dqn_amd import main
    key = (game, kind, seed)
    if key not in _DATASETS:
        path = os.path.join(folder, "%s_%s_%d.ring" % key)
        if kind == "random":
            a = _base(game, seed, random_steps=SIZE, epochs=0, train_steps=0, save_replay=path)
        else:
            a = _base(game, seed, random_steps=1000, epochs=1, train_steps=SIZE - 1000, save_replay=path)
        main.run(a)
        _DATASETS[key] = path
    return _DATASETS[key]


def score(net, env, seed, epsilon=0.05):
    out = net.evaluate(env, EVAL_COPIES, EVAL_STEPS, epsilon, seed)
    return 500.0 * float(out["caught"].sum()) / float(EVAL_COPIES * EVAL_STEPS)


def _offline(game, path, alpha, seed):
    import simple_dqn_amd as sd
    from simple_dqn_amd.main import check_offline_file
    a = _base(game, seed, offline_replay=path, cql_alpha=alpha, random_steps=0)
    check_offline_file(a, path)
    random.seed(seed)
    env = {"freeway": sd.FreewayEnvironment, "catch": sd.CatchEnvironment}[game](a, seed=seed)
    mem, net = sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(env.numActions(), a)
    mem.load(path)
    return env, mem, net, sd.Agent(env, mem, net, a)


def run(game, kind, alpha, seed, learns, every, folder):
    path = dataset(game, kind, seed, folder)
    env, mem, net, agent = _offline(game, path, alpha, seed)
    t0 = time.time()
    rec = dict(game=game, dataset=kind, alpha=alpha, seed=seed, transitions=mem.count, random=score(net, env, seed, 1.0), curve=[])
    for epoch in range(learns // every):
        agent.train_offline(every, epoch)
        rec["curve"].append(((epoch + 1) * every, score(net, env, 2000 + seed + epoch)))
    rec["seconds"] = time.time() - t0
    return rec


def crossing(alpha, seed, folder, learns=40000, every=2000):
    """the offline learning test's loop (tests/test_gpu_offline_learning.py) with an evaluation after every epoch"""
    from test_gpu_catch import _midpoint, per_ball
    path = dataset("catch", "random", seed, folder)
    env, mem, net, agent = _offline("catch", path, alpha, seed)
    t0 = time.time()
    rec = dict(game="catch", dataset="random", alpha=alpha, seed=seed, transitions=mem.count, midpoint=_midpoint(),
               untrained=per_ball(net, env, 1000 + seed), curve=[])
    for epoch in range(learns // every):
        agent.train_offline(every, epoch)
        rec["curve"].append(((epoch + 1) * every, per_ball(net, env, 2000 + seed + epoch)))
    rec["first_crossing"] = next((s for s, v in rec["curve"] if v >= rec["midpoint"]), None)
    rec["seconds"] = time.time() - t0
    return rec


def table(recs):
    by, lines = {}, []
    for r in recs:
        by.setdefault((r["game"], r["dataset"], r["alpha"]), []).append(r)
    for (game, kind, alpha), rs in sorted(by.items()):
        rs.sort(key=lambda r: r["seed"])
        if "first_crossing" in rs[0]:
            lines.append("%-8s %-6s alpha %g seeds %s  midpoint %.3f  first crossing %s  last %s" % (
                game, kind, alpha, [r["seed"] for r in rs], rs[0]["midpoint"], [r["first_crossing"] for r in rs],
                ["%.3f" % r["curve"][-1][1] for r in rs]))
            continue
        last = [statistics.mean(v for _, v in r["curve"][-3:]) for r in rs]      # the plateau: mean of the last three evaluations
        lines.append("%-8s %-6s alpha %g seeds %s  random %.2f  last-3 mean %s  (mean %.2f)  best %s"
                     % (game, kind, alpha, [r["seed"] for r in rs], statistics.mean(r["random"] for r in rs), ["%.2f" % v for v in last],
                        statistics.mean(last), ["%.2f" % max(v for _, v in r["curve"]) for r in rs]))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--games", nargs="+", default=["catch", "freeway"], choices=["catch", "freeway"])
    p.add_argument("--datasets", nargs="+", default=["random", "online"], choices=["random", "online"])
    p.add_argument("--alphas", type=float, nargs="+", default=[0.0, 1.0])
    p.add_argument("--learns", type=int, default=40000)
    p.add_argument("--every", type=int, default=4000)
    p.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    p.add_argument("--crossing", action="store_true")
    p.add_argument("--out", default=None)
    o = p.parse_args()
    recs = []
    with tempfile.TemporaryDirectory() as folder:
        cells = [("catch", "random")] if o.crossing else [(g, k) for g in o.games for k in o.datasets]
        for game, kind in cells:
            for seed in o.seeds:
                for alpha in o.alphas:
                    rec = crossing(alpha, seed, folder) if o.crossing else run(game, kind, alpha, seed, o.learns, o.every, folder)
                    recs.append(rec)
                    print("%s %s alpha %g seed %d: curve %s (%.0f s)" % (game, kind, alpha, seed, " ".join("%.2f" % v for _, v in rec["curve"]),
                                                                       rec["seconds"]), flush=True)
                    if o.out:
                        with open(o.out, "a") as f:
                            f.write(json.dumps(rec) + "\n")
    print(table(recs))


if __name__ == "__main__":
    main()
