"""--munchausen learns catch: tests/test_gpu_catch.py's loop, arguments and criterion with Munchausen targets."""
import time

import pytest

from test_catch import random_baseline
from test_gpu_catch import _midpoint, learning_run

pytestmark = pytest.mark.gpu

# training budget in environment steps: twice the slowest first crossing of the criterion among seeds 1, 2, 3 in runs of up to 60 000
# steps evaluated every 5 000 (tools/munchausen_curves.py; DESIGN.md §22 has the three curves)
BUDGET_STEPS = 30000


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_munchausen_learns_catch(sd, seed):
    """From Xavier weights, BUDGET_STEPS environment steps of main.run's loop with --munchausen true at the command line's defaults
    (alpha 0.9, tau 0.03, clip -1): the mean reward per ball over >= 2 000 balls reaches the midpoint between the random policy's and +1;
    the untrained net stays below it."""
    t0 = time.time()
    before, curve = learning_run(sd, seed, BUDGET_STEPS, munchausen=True, munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-1.0)
    after = curve[-1][1]
    print("seed %d: random baseline %.3f, midpoint %.3f, untrained %.3f, after %d steps %.3f, %.1f s"
          % (seed, random_baseline(), _midpoint(), before, BUDGET_STEPS, after, time.time() - t0))
    assert before < _midpoint()
    assert after >= _midpoint()
