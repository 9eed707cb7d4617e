"""--dueling learns catch: the loop, arguments, seed, budget and criterion of tests/test_gpu_catch.py's learning test with
--dueling true added."""
import time

import pytest

from test_catch import random_baseline
from test_gpu_catch import BUDGET_STEPS, _midpoint, learning_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def test_dueling_learns_catch(sd):
    """From Xavier weights, the budget of tests/test_gpu_catch.py::test_the_agent_learns_catch with --dueling true (seed 1): the mean reward per
    ball over >= 2 000 balls reaches the midpoint between the random policy's and +1; the untrained net stays below it."""
    t0 = time.time()
    before, curve = learning_run(sd, 1, BUDGET_STEPS, dueling=True)
    after = curve[-1][1]
    print("random baseline %.3f, midpoint %.3f, untrained %.3f, after %d steps %.3f, %.1f s"
          % (random_baseline(), _midpoint(), before, BUDGET_STEPS, after, time.time() - t0))
    assert before < _midpoint()
    assert after >= _midpoint()
