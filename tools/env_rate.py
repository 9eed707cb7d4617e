"""Rates of the catch environment paths, one process, forms alternated, median of 7 rounds:
  train   Agent.train env-steps/s on catch, fused act step (game stepped and rendered inside the library) vs host-driven (env.act + act_step
          with the screen), same build, same seeds
  eval    DeepQNetwork.evaluate env-steps/s at N = 32 and N = 256 (float32, float16) vs Agent.test on the same float32 net
    python tools/env_rate.py [--rounds 7] [--train_steps 4000] [--eval_steps 400] [--json out.json]
  --environment catch|breakout|freeway   the library game the rates are taken on (default catch); `--environment both`
          instead alternates catch and breakout in one process, `--environment all` (§25) all three games: DeepQNetwork.evaluate at
          N = 32 and the --train_envs 32 train phase, float32
  --train_envs    instead: train-phase env-steps/s of Agent.train_vectorised — 32 copies (float32, float16), 8 copies, 256
          copies at batch_size 256 — against the fused single-environment Agent.train, all alternated in the same process"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


GAME = "catch"                             # --environment


def _env(sd, a, seed=1, game=None):
    from simple_dqn_amd.environment import LIBRARY_GAMES
    return LIBRARY_GAMES[game or GAME](a, seed=seed)


def _args(**kw):
    from simple_dqn_amd.main import build_parser
    a = build_parser().parse_args(["--environment", GAME])
    a.replay_size, a.exploration_decay_steps, a.target_steps, a.random_seed = 20000, 10000, 500, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def train_envs_rates(o):
    import simple_dqn_amd as sd
    forms = {"single_fused": dict(train_envs=0), "envs32_float32": dict(train_envs=32), "envs8_float32": dict(train_envs=8),
             "envs256_b256_float32": dict(train_envs=256, batch_size=256, replay_size=20480), "envs32_float16": dict(train_envs=32, datatype="float16")}
    agents = {}
    for name, kw in forms.items():
        a = _args(**kw)
        random.seed(1)
        env, mem, net = _env(sd, a), sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(3, a)
        ag = sd.Agent(env, mem, net, a)
        if a.train_envs:
            ag.play_random_vectorised(2000); ag.train_vectorised(1024)
        else:
            ag.play_random(2000); ag.train(1000)
        net.sync()
        agents[name] = (ag, net, a.train_envs)
    rates = dict((k, []) for k in forms)
    for _ in range(o.rounds):
        for name, (ag, net, n) in agents.items():
            steps = o.train_steps * (4 if n else 1)
            steps = -(-steps // n) * n if n else steps
            t0 = time.perf_counter()
            ag.train_vectorised(steps) if n else ag.train(steps)
            net.sync()
            rates[name].append(steps / (time.perf_counter() - t0))
    out = {}
    for name, r in rates.items():
        out["train_" + name] = dict(median=statistics.median(r), min=min(r), max=max(r))
    base = out["train_single_fused"]["median"]
    for name in forms:
        out["train_" + name]["x_single"] = out["train_" + name]["median"] / base
    return out


def both_games_rates(o, games=("catch", "breakout")):
    """evaluate (N = 32) and the --train_envs 32 train phase on each of `games`, alternated in one process, float32"""
    import simple_dqn_amd as sd
    ev, tr = {}, {}
    for g in games:
        a = _args(batch_size=32, environment=g)
        net, env = sd.DeepQNetwork(3, a), _env(sd, a, game=g)
        net.evaluate(env, 32, 20)
        ev[g] = (net, env)
        a = _args(train_envs=32, environment=g)
        random.seed(1)
        env, mem, net = _env(sd, a, game=g), sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(3, a)
        ag = sd.Agent(env, mem, net, a)
        ag.play_random_vectorised(2000); ag.train_vectorised(1024)
        net.sync()
        tr[g] = (ag, net)
    rates = dict(("%s_%s" % (k, g), []) for k in ("evaluate_n32", "train_envs32") for g in games)
    for r in range(o.rounds):
        for g in games:
            net, env = ev[g]
            t0 = time.perf_counter()
            net.evaluate(env, 32, o.eval_steps, 0.05, r)
            rates["evaluate_n32_" + g].append(32 * o.eval_steps / (time.perf_counter() - t0))
        for g in games:
            ag, net = tr[g]
            steps = o.train_steps * 4
            t0 = time.perf_counter()
            ag.train_vectorised(steps)
            net.sync()
            rates["train_envs32_" + g].append(steps / (time.perf_counter() - t0))
    return dict((k, dict(median=statistics.median(v), min=min(v), max=max(v))) for k, v in rates.items())


def main():
    global GAME
    p = argparse.ArgumentParser()
    p.add_argument("--environment", default="catch", choices=["catch", "breakout", "freeway", "both", "all"])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--train_steps", type=int, default=4000)
    p.add_argument("--eval_steps", type=int, default=400)
    p.add_argument("--json", default=None)
    p.add_argument("--train_envs", action="store_true")
    o = p.parse_args()
    import simple_dqn_amd as sd
    out = {}
    if o.environment in ("both", "all"):
        out = both_games_rates(o, ("catch", "breakout") if o.environment == "both" else ("catch", "breakout", "freeway"))
        for k, v in out.items():
            print("%-32s %s" % (k, " ".join("%s %.1f" % kv for kv in v.items())))
        if o.json:
            json.dump(out, open(o.json, "w"), indent=1)
        return
    GAME = o.environment
    if o.train_envs:
        out = train_envs_rates(o)
        for k, v in out.items():
            print("%-32s %s" % (k, " ".join("%s %.2f" % kv for kv in v.items())))
        if o.json:
            json.dump(out, open(o.json, "w"), indent=1)
        return
    # ---- train phase: two agents, alternated
    agents = {}
    for form in ("fused", "host"):
        a = _args()
        random.seed(1)
        env, mem, net = _env(sd, a), sd.ReplayMemory(a.replay_size, a), sd.DeepQNetwork(3, a)
        ag = sd.Agent(env, mem, net, a)
        ag._env_call = form == "fused"
        ag.play_random(2000)
        ag.train(1000)
        net.sync()
        agents[form] = (ag, net)
    rates = {"fused": [], "host": []}
    for _ in range(o.rounds):
        for form in ("fused", "host"):
            ag, net = agents[form]
            t0 = time.perf_counter()
            ag.train(o.train_steps)
            net.sync()
            rates[form].append(o.train_steps / (time.perf_counter() - t0))
    for form in rates:
        out["train_" + form] = dict(median=statistics.median(rates[form]), min=min(rates[form]), max=max(rates[form]))
    # ---- evaluation
    ag, net32 = agents["fused"]
    t = []
    for _ in range(o.rounds):
        t0 = time.perf_counter()
        ag.test(4000)
        net32.sync()
        t.append(4000 / (time.perf_counter() - t0))
    out["agent_test"] = dict(median=statistics.median(t), min=min(t), max=max(t))
    for dt in ("float32", "float16"):
        for n in (32, 256):
            a = _args(batch_size=n, datatype=dt)
            net, env = sd.DeepQNetwork(3, a), _env(sd, a)
            net.evaluate(env, n, 20)
            t = []
            for r in range(o.rounds):
                t0 = time.perf_counter()
                net.evaluate(env, n, o.eval_steps, 0.05, r)
                dtm = time.perf_counter() - t0
                t.append(n * o.eval_steps / dtm)
            med = statistics.median(t)
            out["evaluate_%s_n%d" % (dt, n)] = dict(median=med, min=min(t), max=max(t), us_per_launch_group=1e6 * n / med)
    for k, v in out.items():
        print("%-24s %s" % (k, " ".join("%s %.1f" % kv for kv in v.items())))
    if o.json:
        json.dump(out, open(o.json, "w"), indent=1)


if __name__ == "__main__":
    main()
