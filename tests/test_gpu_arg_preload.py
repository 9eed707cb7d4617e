"""Option arg_preload (gemm_engine.h: Lead): with 1 the step kernels take their hot arguments from the leading parameter block that the
command processor preloads into SGPRs, with 0 from the by-value struct.  The host passes the same values both ways, so three steps of
train_from_memory must leave bit-identical weights, RMSProp state and Q-values — in every case whose argument blocks differ: indexes in
the kernel arguments (B <= 32) or in device memory (B = 40), the tuple API (staged states instead of the ring), a third net slot
(--double_dqn), one launch per backward problem (fused_launches = 0), and B = 128, where the block stays off.  One step at B = 32 is also held to the numpy oracle."""
import random

import numpy as np
import pytest

from util import make_args
from oracle.dqn_numpy import OracleDQN, xavier_weights
from oracle.replay_numpy import ReplayOracle, synthetic_fill

pytestmark = pytest.mark.gpu
A, RING = 4, 2000
Q_TOL = 1e-4          # tests/test_gpu_dqn.py: Q-values of a single step against the oracle


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


def _run(sd, preload, B, tuple_api=False, steps=3, options=(), **kw):
    args = make_args(batch_size=B, **kw)
    mem = sd.ReplayMemory(RING, args)
    synthetic_fill(mem, 0, num_actions=A)
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    net.set_weights(xavier_weights(A, 21), 0)
    net.update_target_network()
    for name, value in options:
        net.set_option(name, value)
    net.set_option("arg_preload", preload)
    random.seed(5)
    if tuple_api:
        for _ in range(steps):
            net.train([x.copy() for x in mem.getMinibatch()])
    else:
        net.train_from_memory(mem, steps)
    random.seed(6)
    q = net.predict(mem.getMinibatch()[0]).copy()
    return [net.get_layer(i, 0) for i in range(5)], [net.get_layer(i, 2) for i in range(5)], q


CASES = {
    "ring_b32": dict(B=32),
    "ring_b16": dict(B=16),
    "ring_b40": dict(B=40),
    "tuple_b32": dict(B=32, tuple_api=True),
    "double_dqn_b32": dict(B=32, double_dqn=True),
    "unfused_b32": dict(B=32, options=(("fused_launches", 0),)),
    "ring_b128": dict(B=128),               # the kernels share templates with B >= 128, where the block is switched off on the host
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_arg_preload_is_bit_identical(sd, case):
    on, off = _run(sd, 1, **CASES[case]), _run(sd, 0, **CASES[case])
    for i in range(5):
        assert np.array_equal(on[0][i], off[0][i]), "weights layer %d" % i
        assert np.array_equal(on[1][i], off[1][i]), "RMSProp state layer %d" % i
    assert np.array_equal(on[2], off[2]), "Q"
    assert np.isfinite(on[2]).all() and np.abs(on[2]).max() > 0


def test_one_step_with_arg_preload_matches_the_oracle(sd):
    B = 32
    args = make_args(batch_size=B)
    mem, omem = sd.ReplayMemory(RING, args), ReplayOracle(RING, batch_size=B)
    synthetic_fill(mem, 0, num_actions=A)
    synthetic_fill(omem, 0, num_actions=A)
    mem.sync_mirror()
    net = sd.DeepQNetwork(A, args)
    ws = xavier_weights(A, 22)
    net.set_weights(ws, 0)
    net.update_target_network()
    net.set_option("arg_preload", 1)
    o = OracleDQN(A, batch_size=B, weights=ws)
    random.seed(3)
    omb = omem.getMinibatch()
    random.seed(3)
    net.train_from_memory(mem, 1)
    o.train(omb)
    err = float(np.abs(net.predict(omb[0]) - o.predict(omb[0])).max())
    print("Q max-abs err vs oracle after one step: %.3e" % err)
    assert err < Q_TOL
