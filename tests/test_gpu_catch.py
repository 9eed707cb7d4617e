"""The device side of "catch" (DESIGN.md §18): the render kernel, the fused act step against the host-driven one bit for bit, the
vectorised evaluation against the oracle, and the learning test."""
import ctypes as C
import csv
import os
import random
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import make_args  # noqa: E402
from catch_oracle import CatchOracle, EvalOracle  # noqa: E402
from test_catch import random_baseline  # noqa: E402

pytestmark = pytest.mark.gpu
Q_TOL = 1e-4          # the tolerance tests/test_gpu_dqn.py uses for predict


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _args(**kw):
    d = dict(priority_alpha=0.6, priority_beta=0.4, priority_epsilon=1e-6, priority_beta_steps=1000, prioritized_replay=False,
             n_step=1, double_dqn=False, catch_balls=10, eval_envs=0)
    d.update(kw)
    return make_args(**d)


def _device_window(sd, buf):
    out = np.empty((buf.history_length,) + buf.dims, np.uint8)
    sd._lib.check(sd.load().sdqn_statebuf_read_device(buf._h, sd._lib.ptr(out, C.c_uint8)))
    return out


def _device_ring(mem):
    """frames [0, covered) of the HBM mirror, read through the gather kernel (prestates of indexes hist, 2 hist, ...)"""
    hist, B = mem.history_length, mem.batch_size
    idx = list(range(hist, mem.count - mem.n_step + 1, hist))
    frames = np.zeros((idx[-1],) + mem.dims, np.uint8)
    for o in range(0, len(idx), B):
        part = idx[o:o + B]
        pre = np.asarray(mem.gather(part + [part[-1]] * (B - len(part)))[0])
        for k, i in enumerate(part):
            frames[i - hist:i] = pre[k]
    return frames


@pytest.mark.parametrize("H,W", [(84, 84), (96, 96), (60, 52), (12, 12), (36, 30)])
def test_render_kernel_equals_host_and_oracle(sd, H, W):
    env, o = sd.CatchEnvironment(_args(screen_height=H, screen_width=W), seed=3), CatchOracle(H, W, 3)
    for t in range(400):
        a = (t * 7 + t // 5) % 3
        env.act(a); o.act(a)
        if t % 3 == 0:
            d = env.render_device()
            assert np.array_equal(d, o.screen()) and np.array_equal(d, env.getScreen()), t
        if o.terminal:
            env.restart(); o.restart()


@pytest.mark.parametrize("variant", ["uniform", "prioritized", "n_step3"])
def test_fused_act_step_equals_host_driven(sd, variant):
    kw = dict(uniform={}, prioritized=dict(prioritized_replay=True), n_step3=dict(n_step=3))[variant]
    args = _args(batch_size=32, random_seed=11, target_steps=100, **kw)
    steps, size = 3200, 700                                          # the ring wraps 4 times, the state buffer's 64 slots ~50 times
    sets = []
    for fused in (False, True):
        env, buf, mem = sd.CatchEnvironment(args, seed=77), sd.DeviceStateBuffer(args), sd.ReplayMemory(size, args)
        sets.append((fused, env, buf, mem, sd.DeepQNetwork(3, args)))
    pol = np.random.RandomState(5)
    actions = pol.randint(0, 3, steps)
    log = [[], []]
    for t in range(steps):
        spec = bool(t % 5 == 0)
        for k, (fused, env, buf, mem, net) in enumerate(sets):
            a = int(actions[t])
            if fused:
                r, term = net.act_step_env(buf, mem, env, a, speculate=spec)
            else:
                r = env.act(a)
                term = env.isTerminal()
                net.act_step(buf, mem, env.getScreen(), a, r, term, speculate=spec and not term)
            log[k].append((a, r, term))
            if term:
                env.restart()
        if t % 97 == 0 or t > steps - 70:
            w = [_device_window(sd, s[2]) for s in sets]
            assert np.array_equal(w[0], w[1]), t
            assert np.array_equal(sets[0][2].getState(), sets[1][2].getState()) and np.array_equal(w[1], sets[1][2].getState()), t
            assert np.array_equal(sets[0][1].getScreen(), sets[1][1].getScreen())
            if spec:                                                 # a pending speculation is collected with the same values
                assert np.array_equal(sets[0][4].predict_state(sets[0][2]), sets[1][4].predict_state(sets[1][2]))
    assert log[0] == log[1] and any(x[2] for x in log[0])
    m0, m1 = sets[0][3], sets[1][3]
    assert (m0.count, m0.current) == (m1.count, m1.current) == (size, steps % size)
    for name in ("screens", "actions", "rewards", "terminals"):
        assert np.array_equal(np.asarray(getattr(m0, name)), np.asarray(getattr(m1, name))), name
    d0, d1 = _device_ring(m0), _device_ring(m1)
    assert len(d0) >= size - 8 and np.array_equal(d0, d1)
    assert np.array_equal(d1, np.asarray(m1.screens)[:len(d1)])       # the kernel-rendered mirror == the host-rendered ring
    for s in (1, 2):
        mbs = []
        for m in (m0, m1):
            random.seed(s)
            mbs.append([np.array(x) for x in m.getMinibatch()])
        for x, y in zip(*mbs):
            assert np.array_equal(x, y)
    outs = []
    for (_, env, buf, mem, net) in sets:
        random.seed(9)
        for _ in range(20):
            net.train_from_memory(mem, 1)
        outs.append((net.get_weights(), mem.last_sample() if mem.prioritized else None, mem.priorities() if mem.prioritized else None))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(x, y)
    if variant == "prioritized":
        assert np.array_equal(outs[0][1][0], outs[1][1][0]) and np.array_equal(outs[0][1][1], outs[1][1][1])
        assert np.array_equal(outs[0][2], outs[1][2]) and len(set(outs[0][2].tolist())) > 3


def test_agent_fused_equals_host_driven(sd, tmp_path):
    from simple_dqn_amd.statistics import Statistics
    rows, weights = [], []
    for fused in (True, False):
        path = str(tmp_path / ("fused%d.csv" % fused))
        args = _args(batch_size=32, random_seed=21, target_steps=50, exploration_decay_steps=600, csv_file=path, random_starts=8)
        random.seed(21)
        env, mem, net = sd.CatchEnvironment(args, seed=21), sd.ReplayMemory(900, args), sd.DeepQNetwork(3, args)
        agent = sd.Agent(env, mem, net, args)
        assert agent._env_call
        agent._env_call = fused                                      # False: env.act + act_step(screen), the host-driven path
        st = Statistics(agent, net, mem, env, args)
        st.reset(); agent.play_random(400); st.write(0, "random")
        st.reset(); agent.train(1500, 0); st.write(1, "train")
        st.reset(); agent.test(300, 0); st.write(1, "test")
        st.close()
        rows.append([r[:13] for r in csv.reader(open(path))])        # (the last three columns are clock readings)
        weights.append(net.get_weights())
    assert rows[0] == rows[1] and len(rows[0]) == 4
    for x, y in zip(*weights):
        assert np.array_equal(x, y)


def _check_against_oracle(net, env, N, steps, eps, seed, check_q):
    B = net.batch_size
    out = net.evaluate(env, N, steps, eps, seed, trace=True)
    o = EvalOracle(N, net.history_length, env.dims[0], env.dims[1], eps, seed, env.balls_per_episode)
    explored = 0
    for t in range(steps):
        if check_q:                                                  # (i) the forward saw the oracle's states
            st = np.zeros((B,) + o.states.shape[1:], np.uint8); st[:N] = o.states
            err = np.abs(net.predict(st)[:N].astype(np.float64) - out["q"][t]).max()
            assert err < Q_TOL, (t, err)
        a, r, term = o.step(out["q"][t])                             # (ii) the rule on the library's own Q bits
        assert np.array_equal(a, out["actions"][t]), t
        assert np.array_equal(r, out["rewards"][t]) and np.array_equal(term, out["terminals"][t]), t   # (iii)
        explored += int((a != np.array([np.argmax(q) for q in out["q"][t]])).sum())
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(out[k], o.tally[k]), k
    assert out["steps"].tolist() == [steps] * N
    plain = net.evaluate(env, N, steps, eps, seed)                   # (iv)
    for k in ("steps", "reward", "caught", "missed", "episodes"):
        assert np.array_equal(plain[k], out[k]), k
    return out, explored


@pytest.mark.parametrize("N", [32, 5])
def test_evaluate_equals_the_oracle_float32(sd, N):
    args = _args(batch_size=32, random_seed=4)
    net, env = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=1)
    before = env.get_state()
    out, explored = _check_against_oracle(net, env, N, 300, 0.1, 1234 + N, check_q=True)
    assert env.get_state() == before
    assert out["caught"].sum() + out["missed"].sum() == N * (300 // 11) and out["episodes"].sum() == N * 2
    assert 0 < explored < 0.1 * 300 * N                              # some steps explored (a third of them pick the greedy action anyway)
    with pytest.raises(AssertionError):
        net.evaluate(env, 33, 10)
    with pytest.raises(AssertionError):
        net.evaluate(sd.CatchEnvironment(_args(screen_height=96, screen_width=96), seed=1), 4, 10)


@pytest.mark.parametrize("kw,N,steps", [(dict(datatype="float16"), 32, 120), (dict(datatype="float64", batch_size=8), 8, 60),
                                        (dict(screen_height=96, screen_width=96, batch_size=8), 5, 60), (dict(batch_norm=True), 32, 120)])
def test_evaluate_other_configurations(sd, kw, N, steps):
    args = _args(random_seed=6, **kw)
    net, env = sd.DeepQNetwork(3, args), sd.CatchEnvironment(args, seed=2)
    if kw.get("batch_norm"):
        run0 = [net.get_bn(l, running=True) for l in range(4)]
    _check_against_oracle(net, env, N, steps, 0.1, 99, check_q=False)
    if kw.get("batch_norm"):
        for l in range(4):
            for x, y in zip(run0[l], net.get_bn(l, running=True)):
                assert np.array_equal(x, y)


def test_evaluate_leaves_the_network_as_it_was(sd):
    """predict_state (with a speculation pending), train_from_memory and predict give what they give in a run that never evaluated"""
    res = []
    for evaluate in (False, True):
        args = _args(batch_size=32, random_seed=8, target_steps=10)
        env, buf, mem, net = sd.CatchEnvironment(args, seed=5), sd.DeviceStateBuffer(args), sd.ReplayMemory(400, args), sd.DeepQNetwork(3, args)
        for t in range(200):
            r, term = net.act_step_env(buf, mem, env, t % 3, speculate=(t == 199))
            if term:
                env.restart()
        got = []
        if evaluate:
            net.evaluate(env, 32, 40, 0.1, 3)
        got.append(net.predict_state(buf))                           # the speculation enqueued before the evaluation
        random.seed(2)
        got.append(net.train_from_memory(mem, 3, want_cost=True))
        if evaluate:
            net.evaluate(env, 7, 25, 0.1, 4)
        got.append(net.train_from_memory(mem, 2, want_cost=True))
        got.append(net.predict_state(buf))
        got.append(net.predict(np.asarray(mem.getMinibatch()[0])))
        got.extend(net.get_weights())
        res.append(got)
    for x, y in zip(*res):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- the learning test ------------------------------------------------------------------------------------------------------------
# Hyper-parameters of the short run (DESIGN.md §18 lists them): a ring of 20 000 transitions, exploration annealed from 1 to 0.1 over
# 10 000 steps, the target net refreshed every 500 steps, everything else at the command line's defaults.
LEARN = dict(environment="catch", replay_size=20000, exploration_decay_steps=10000, target_steps=500, random_steps=1000,
             test_steps=0, batch_size=32, num_actions=3, synthetic_frame_pool=0, game="catch", visualization_file=None,
             visualization_filters=4)
EPOCH_STEPS = 5000
BUDGET_STEPS = 20000       # training budget in environment steps: twice the slowest of three measured seeds — seeds 1, 2, 3 first met
                           # the criterion at the 10 000-step evaluation (evaluated every 5 000 steps; DESIGN.md §18 has the curves)
EVAL_STEPS = 770           # x 32 copies = 24 640 steps = 2 240 balls


def per_ball(net, env, seed):
    out = net.evaluate(env, 32, EVAL_STEPS, 0.05, seed)
    balls = int(out["caught"].sum() + out["missed"].sum())
    assert balls >= 2000
    return float(out["reward"].sum()) / balls


def learning_run(sd, seed, steps, every=None, **kw):
    """main.run's loop on catch; returns (mean reward per ball of the untrained net, [(env steps, mean reward per ball)])"""
    from simple_dqn_amd import main
    curve = []
    st = main.run(_args(random_seed=seed, epochs=0, train_steps=0, **dict(LEARN, **dict(kw, random_steps=0))))
    before = per_ball(st.net, st.env, 1000 + seed)
    chunk = every or steps
    args = _args(random_seed=seed, epochs=steps // chunk, train_steps=chunk, **dict(LEARN, **kw))
    if every is None:
        st = main.run(args)
        curve.append((steps, per_ball(st.net, st.env, 2000 + seed)))
        return before, curve
    # the same loop with an evaluation after every epoch (what main.run does with --eval_envs, kept apart from its tallies here)
    from simple_dqn_amd import Agent, CatchEnvironment, DeepQNetwork, ReplayMemory
    random.seed(seed)
    env = CatchEnvironment(args, seed=seed)
    mem, net = ReplayMemory(args.replay_size, args), DeepQNetwork(3, args)
    agent = Agent(env, mem, net, args)
    agent.play_random(args.random_steps)
    for epoch in range(args.epochs):
        agent.train(chunk, epoch)
        curve.append(((epoch + 1) * chunk, per_ball(net, env, 2000 + seed + epoch)))
    return before, curve


def _midpoint():
    return (random_baseline() + 1.0) / 2.0                           # "learned": half way from the random policy to catching every ball


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_agent_learns_catch(sd, seed):
    """From Xavier weights, BUDGET_STEPS environment steps of main.run's loop: the mean reward per ball over >= 2 000 balls
    (evaluate, 32 copies, epsilon 0.05) reaches the midpoint between the random policy's (tests/test_catch.py) and +1; the untrained
    net stays below it."""
    t0 = time.time()
    before, curve = learning_run(sd, seed, BUDGET_STEPS)
    after = curve[-1][1]
    print("seed %d: random baseline %.3f, midpoint %.3f, untrained %.3f, after %d steps %.3f, %.1f s"
          % (seed, random_baseline(), _midpoint(), before, BUDGET_STEPS, after, time.time() - t0))
    assert before < _midpoint()
    assert after >= _midpoint()


@pytest.mark.parametrize("name,kw", [("double_dqn", dict(double_dqn=True)), ("n_step3", dict(n_step=3)),
                                     ("prioritized", dict(prioritized_replay=True, priority_beta_steps=50000))])
def test_the_options_learn_catch(sd, name, kw):
    """The same loop and budget with --double_dqn, --n_step 3, --prioritized_replay (seed 1).  Asserted because a preliminary run of
    seeds 1, 2, 3 met the criterion for every option."""
    before, curve = learning_run(sd, 1, BUDGET_STEPS, **kw)
    after = curve[-1][1]
    print("%s: midpoint %.3f, untrained %.3f, after %d steps %.3f" % (name, _midpoint(), before, BUDGET_STEPS, after))
    assert before < _midpoint()
    assert after >= _midpoint()
