"""One profiled train step from a 64-slot ring per configuration: the kernel ids that launch, and how often, are what resolve_route
(simple_dqn_amd/csrc/launch_route.h, through tests/route_emul.py) predicts for that handle — a launching route is one sample, a route that
rides in a sibling's launch none.  The batch sizes are the smallest at which each riding rule switches."""
import random

import pytest

import route_emul as R
from oracle.dqn_numpy import xavier_weights
from oracle.replay_numpy import synthetic_fill
from util import make_args

pytestmark = pytest.mark.gpu

HEAD, UPDATE, PREP = 4, 12, 15
STAGES = {"fused": (0, 1, 2, 3, 5, 16, 17, 18), "h16_block_tile": (0, 1, 2, 3, 5, 7, 9, 24, 18)}      # the routed launches of a step
# (datatype, B) -> the stage ids that launch nothing
CASES = [("float32", 32, ()), ("float32", 128, (2,)), ("float32", 160, ()), ("float16", 32, (0, 2)), ("float16", 128, (0, 2, 9, 18))]


@pytest.mark.parametrize("datatype,B,silent", CASES)
def test_profiled_step_launches_what_the_resolver_predicts(datatype, B, silent):
    import simple_dqn_amd as sd
    A = 4
    args = make_args(batch_size=B, datatype=datatype, replay_size=64)
    mem = sd.ReplayMemory(64, args)
    synthetic_fill(mem, 5, num_actions=A)
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    net.set_weights(xavier_weights(A, 12), 1)
    net.set_weights(xavier_weights(A, 11), 0)
    structure = net.step_structure()[0]
    h16 = 2 if datatype == "float16" else 0
    want, rides = {HEAD: 1, UPDATE: 1, PREP: 1}, []
    for kid in STAGES[structure]:
        # conv1_wgrad rides in the float16 weight-gradient launch by default (option c1w_in_wgrads = 1 -> LV_C1W_IN_WGRADS = 16); all of
        # fc4_wgrad rides in bwd3; a ring step at B <= 32 carries the host's copy of its indexes
        variant = 16 if structure == "h16_block_tile" and kid in (R.K_BWD1, R.K_WGRADS) else 0
        unit, form, rides_in = R.route(kid, B, 2, h16, 0, f4w=int(kid == 16), ring=1, hidx=int(B <= 32), variant=variant)
        assert form != "FORM_INVALID", kid
        if unit == "none":
            rides.append(kid)
            assert rides_in in STAGES[structure], (kid, rides_in)
        else:
            want[kid] = 1
    assert tuple(sorted(rides)) == silent
    net.profile(True, -1); net.profile_reset()
    random.seed(3)
    net.train_from_memory(mem, 1)
    got = {p["id"]: p["launches"] for p in net.profile_read() if p["launches"] > 0}
    net.profile(False)
    print("launches:", got)
    assert got == want
