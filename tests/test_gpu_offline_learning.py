"""Offline training learns catch: a dataset of 20 000 random-play steps written by main.run --save_replay, then main.run
--offline_replay with --eval_envs 32, held to the criterion of tests/test_gpu_catch.py — the mean reward per ball over >= 2 000 balls
reaches the midpoint between the random policy's and +1, and the untrained net stays below it."""
import time

import pytest

from test_catch import random_baseline
from test_gpu_catch import LEARN, _args, _midpoint, per_ball

pytestmark = pytest.mark.gpu

SIZE = 20000
HORIZON = 40000
# training budget in learns: twice the slowest first crossing of the criterion among seeds 1, 2, 3, evaluated every 2 000 of 40 000 learns
# (tools/offline_curves.py --crossing; profiles/offline_crossings.json).  alpha 0: 4 000, 4 000, 4 000.  alpha 1: none of
# the three seeds crossed (last evaluations -0.39, -0.29, -0.32 against the midpoint 0.244), so that configuration runs the whole horizon
BUDGET = {0.0: 8000, 1.0: HORIZON}


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


@pytest.fixture(scope="module")
def dataset(sd, tmp_path_factory):
    """main.run's single-environment loop, random play only, written with --save_replay"""
    from simple_dqn_amd import main
    path = str(tmp_path_factory.mktemp("offline_learning") / "catch_random.ring")
    st = main.run(_args(random_seed=1, epochs=0, train_steps=0, save_replay=path, **dict(LEARN, random_steps=SIZE, replay_size=SIZE)))
    assert st.net.train_iterations == 0
    assert sd.ReplayMemory.peek(path) == dict(size=SIZE, count=SIZE, current=0, H=84, W=84, hist=4)
    return path


def _offline(sd, dataset, alpha):
    from simple_dqn_amd import main
    t0 = time.time()
    kw = dict(LEARN, random_steps=0, replay_size=SIZE, offline_replay=dataset, cql_alpha=alpha, eval_envs=32)
    st = main.run(_args(random_seed=1, epochs=0, train_steps=0, **kw))
    before = per_ball(st.net, st.env, 1001)
    assert st.mem.count == SIZE and st.net.train_iterations == 0           # --offline_replay accepted what --save_replay wrote
    st = main.run(_args(random_seed=1, epochs=1, train_steps=BUDGET[alpha], **dict(kw, test_steps=320)))      # (the test phase: 32 copies x 10 steps)
    assert st.net.train_iterations == BUDGET[alpha] and st.mem.count == SIZE and st.num_steps == 320
    after = per_ball(st.net, st.env, 2001)
    print("alpha %g: random baseline %.3f, midpoint %.3f, untrained %.3f, after %d learns %.3f, %.1f s"
          % (alpha, random_baseline(), _midpoint(), before, BUDGET[alpha], after, time.time() - t0))
    assert before < _midpoint()
    assert after >= _midpoint()


def test_offline_dqn_learns_catch_from_random_play(sd, dataset):
    _offline(sd, dataset, 0.0)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="--cql_alpha 1 on 20 000 random-play steps of catch: none of seeds 1, 2, 3 crossed the midpoint within "
                                       "40 000 learns (profiles/offline_crossings.json; DESIGN.md §35.8: on uniformly random data the "
                                       "regulariser pulls the policy toward the data's, which is the random one)")
def test_offline_cql_learns_catch_from_random_play(sd, dataset):
    _offline(sd, dataset, 1.0)
