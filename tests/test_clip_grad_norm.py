"""--clip_grad_norm without a device: the oracle's formula against torch.nn.utils.clip_grad_norm_, the flag and its
range check, the bindings, and what the compiler made of the two kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from clip_oracle import ClipOracle, clip_gradients, clip_scale, grad_norm
from oracle.dqn_numpy import xavier_weights
from util import random_minibatch

SHAPES = [(256, 32), (512, 64), (576, 64), (512, 3136), (3, 512)]          # the network's layers at A = 3: 1.69 M values
BSZ = 32


def _grads(seed, scale=1.0):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal(s) * scale for s in SHAPES]


@pytest.mark.parametrize("max_norm", [10.0, 0.5, 1e-3])
def test_oracle_equals_torch_clip_grad_norm(max_norm):
    """float64 on both sides, the same tensors: torch sees the MEAN gradient g / bsz.  Relative tolerance 1e-12: the formula's own
    rounding, both sides fp64 over fewer than 2 M terms."""
    g = _grads(1)
    clipped, norm, scale = clip_gradients(g, BSZ, max_norm, np.float64)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
    for p, gi in zip(params, g):
        p.grad = torch.from_numpy(gi / BSZ)
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert scale < 1                                                       # (a gaussian draw of 1.69 M values: norm ~ 40)
    assert abs(norm - total) <= 1e-12 * total
    t_scale = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(scale) - t_scale) <= 1e-12 * t_scale
    for c, p in zip(clipped, params):
        np.testing.assert_allclose(c / BSZ, p.grad.numpy(), rtol=1e-12, atol=0)


def test_scale_one_leaves_every_array_identical():
    g = _grads(2, scale=1e-3)
    clipped, norm, scale = clip_gradients(g, BSZ, 10.0, np.float64)
    assert scale == 1 and norm == grad_norm(g, BSZ)
    assert all(c is gi for c, gi in zip(clipped, g))
    # a non-finite norm clips nothing either
    g[3][0, 0] = np.nan
    clipped, norm, scale = clip_gradients(g, BSZ, 10.0, np.float32)
    assert np.isnan(norm) and scale == 1 and all(c is gi for c, gi in zip(clipped, g))
    assert clip_scale(float("inf"), 10.0, np.float32) == 1


def test_oracle_step_with_a_loose_bound_is_the_plain_step():
    """ClipOracle with G far above the norm moves exactly as OracleDQN does; with G below it, by a smaller step"""
    from oracle.dqn_numpy import OracleDQN
    A, B = 3, 4
    ws = xavier_weights(A, 5)
    mb = random_minibatch(B, A, 6)
    plain, loose, tight = OracleDQN(A, batch_size=B, weights=ws), ClipOracle(A, batch_size=B, weights=ws, clip_grad_norm=1e9), \
        ClipOracle(A, batch_size=B, weights=ws, clip_grad_norm=1e-3)
    for o in (plain, loose, tight):
        o.train(mb)
    assert loose.last_scale == 1 and tight.last_scale < 1 and tight.last_norm == loose.last_norm
    for i in range(5):
        assert np.array_equal(plain.W[i], loose.W[i]) and np.array_equal(plain.S[i], loose.S[i])
        assert np.abs(tight.S[i]).max() < np.abs(plain.S[i]).max()


def test_parser_and_range_check():
    from simple_dqn_amd import main
    a = main.build_parser().parse_args([])
    assert a.clip_grad_norm == 0.0 and main.check_clip_grad_norm(a) == 0.0
    a = main.build_parser().parse_args(["--clip_grad_norm", "10"])
    assert a.clip_grad_norm == 10.0 and main.check_clip_grad_norm(a) == 10.0
    groups = {g.title: [x.dest for x in g._group_actions] for g in main.build_parser()._action_groups}
    assert "clip_grad_norm" in groups["Deep Q-learning network"]


@pytest.mark.parametrize("value", ["-1", "nan", "inf"])
def test_main_run_refuses_before_touching_the_device(value, monkeypatch):
    from simple_dqn_amd import main
    import simple_dqn_amd

    def no_device(*a, **k):
        raise RuntimeError("a device object was constructed")
    for cls in ("DeepQNetwork", "ReplayMemory"):
        monkeypatch.setattr(simple_dqn_amd, cls, no_device)
    args = main.build_parser().parse_args(["--random_steps", "0", "--epochs", "0", "--clip_grad_norm", value])
    with pytest.raises(ValueError) as ei:
        main.run(args)
    assert "--clip_grad_norm" in str(ei.value)


def test_bindings_are_declared_and_exported():
    import simple_dqn_amd as sd
    sig = sd._lib.SIGNATURES
    assert sig["sdqn_net_set_clip_grad_norm"] == (C.c_int, [C.c_void_p, C.c_double])
    assert sig["sdqn_net_get_clip_grad_norm"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double)])
    assert sig["sdqn_net_last_grad_norm"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    lib = sd.load()
    for name in ("sdqn_net_set_clip_grad_norm", "sdqn_net_get_clip_grad_norm", "sdqn_net_last_grad_norm"):
        assert getattr(lib, name) is not None
    assert sd.DeepQNetwork.UPDATE_FORMS[4] == "clip"


def test_isa_census_of_the_clip_kernels():
    """registers, LDS and scratch of the two kernels (float and double instances) as the compiler reports them: no scratch, LDS below 4 KB,
    at most 128 registers (full residency of a 256-thread workgroup)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_census
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("hipcc not installed")
    rows = isa_census.census_rows("sdqn_clip.hip")
    for kernel in ("grad_sqnorm_kernel", "grad_scale_kernel"):
        hit = [r for r in rows if kernel in r["name"]]
        assert len(hit) == 2, [r["name"] for r in rows]                    # <float>, <double>
        for k in hit:
            print("%s: vgpr %d agpr %d lds %d scratch %d" % (k["name"], k["vgpr"], k["agpr"], k["lds"], k["scratch"]))
            assert k["scratch"] == 0 and k["lds"] < 4096 and k["vgpr"] + k["agpr"] <= 128
