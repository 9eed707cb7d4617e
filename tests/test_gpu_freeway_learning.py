"""The default train step learns freeway: tools/freeway_curves.py's loop, arguments and evaluation, held to the midpoint
between the uniformly random policy's score and the default configuration's measured plateau.

  random    0.177 crossings per 500-tick episode: tests/freeway_oracle.py on the CPU, 3 x 200 episodes (0.220, 0.125, 0.185; recomputed
            below), no device involved
  plateau   19.72: the mean of the default configuration's 20 evaluations between 110 000 and 300 000 environment steps, over seeds
            1, 2, 3 (18.93, 18.82, 21.41; profiles/freeway_curves.json, measured on an MI355X)
  criterion their midpoint, 9.95
  budget    80 000 environment steps: twice the slowest seed's first evaluation at or above the criterion (40 000, 30 000, 20 000 for
            seeds 1, 2, 3) — §18's and §22's rule.  At 80 000 steps the three curves stood at 26.1, 25.2 and 18.5."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from freeway_oracle import random_policy_score  # noqa: E402

pytestmark = pytest.mark.gpu
PLATEAU = 19.72
BUDGET_STEPS, EVERY = 80000, 10000


@pytest.fixture(scope="module")
def criterion():
    scores = [random_policy_score(200, seed)[0] for seed in (1, 2, 3)]
    rnd = sum(scores) / 3.0
    print("random policy on the oracle: %s crossings per 500-tick episode, mean %.3f" % (scores, rnd))
    assert 0.1 < rnd < 0.3
    return 0.5 * (rnd + PLATEAU)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_default_step_learns_freeway(criterion, seed):
    """From Xavier weights, BUDGET_STEPS environment steps of the --train_envs 32 loop at tools/freeway_curves.py's arguments: crossings
    per 500 ticks (32 copies x 1 000 steps, epsilon 0.05) reach the criterion; the random policy and the untrained net stay below it."""
    import freeway_curves
    rec = freeway_curves.run("envs32", seed, BUDGET_STEPS, EVERY)
    after = rec["curve"][-1][1]
    print("seed %d: criterion %.2f, random %.3f, untrained %.3f, curve %s, %.1f s"
          % (seed, criterion, rec["random"], rec["untrained"], " ".join("%.1f" % v for _, v in rec["curve"]), rec["seconds"]))
    assert rec["random"] < criterion and rec["untrained"] < criterion
    assert after >= criterion
