"""--quantiles learns catch: tests/test_gpu_catch.py's loop, arguments and criterion with six quantiles per action,
experience collected from 32 copies of the game and evaluated on 32 (--train_envs 32 --eval_envs 32 --quantiles 6)."""
import time

import pytest

from test_catch import random_baseline
from test_gpu_catch import _midpoint, learning_run

pytestmark = pytest.mark.gpu

# training budget in environment steps: twice the slowest first crossing of the criterion among seeds 1, 2, 3 of N = 6 in runs of 60 000
# steps evaluated every 5 000 (tools/quantile_curves.py; profiles/quantile_curves.json; DESIGN.md §29.3 has the table)
BUDGET_STEPS = 40000


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def test_quantile_regression_learns_catch(sd):
    """From Xavier weights, BUDGET_STEPS environment steps of main.run's loop with --quantiles 6 --train_envs 32 --eval_envs 32 (seed 1): the
    mean reward per ball over >= 2 000 balls reaches the midpoint between the random policy's and +1; the untrained net stays below it."""
    t0 = time.time()
    before, curve = learning_run(sd, 1, BUDGET_STEPS, quantiles=6, train_envs=32, eval_envs=32)
    after = curve[-1][1]
    print("random baseline %.3f, midpoint %.3f, untrained %.3f, after %d steps %.3f, %.1f s"
          % (random_baseline(), _midpoint(), before, BUDGET_STEPS, after, time.time() - t0))
    assert before < _midpoint()
    assert after >= _midpoint()
