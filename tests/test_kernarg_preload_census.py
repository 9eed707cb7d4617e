"""The kernels of the default B < 128 fp32 step take their hot arguments as leading scalar / pointer parameters (gemm_engine.h: Lead) that
gfx950's command processor preloads into SGPRs at wave launch.  Checked WITHOUT a GPU from the compiler's kernel descriptors
(tools/isa_census.py, built with the flags csrc/Makefile gives each translation unit): every such kernel reports a preload length > 0, and
the preload costs no residency — the resource limits of tests/test_isa_census.py hold and nothing spills."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_census.HIPCC), reason="hipcc not installed")

# launch name -> (translation unit, mangled-name fragments that select exactly one kernel)
STEP_KERNELS = {
    "conv1_fwd": ("r3", ("conv1_bf16_kernelILb1E",)),
    "update": ("k", ("update_kernelILb0E",)),
    "conv2_fwd": ("r3", ("gemm_kernelINS_10Conv2FwdWTELi16E",)),
    "conv3_fwd": ("r3", ("gemm36_kernelINS_10Conv3FwdWTE",)),
    "fc4_fwd": ("r3", ("gemm_kernelINS_6StagedINS_8Fc4FwdWTEEELi14E",)),
    "head": ("k", ("head_kernelILi4ELb0ELb0ELb0ELb0ELb0E",)),
    "fc4_dgrad": ("r3", ("gemm_kernelINS_6StagedINS_10Fc4DgradWTEEELi16E",)),
    "bwd3": ("r3", ("gemm_multi_kernelILi512E", "Conv3DgradWT", "Fc4WgradWTELi1E")),
    "bwd2": ("r3", ("gemm_multi_kernelILi512ENS_9NoProblemELi2ENS_12Conv2DgradWTELi8E",)),
    "bwd1": ("r3", ("conv1_wgrad_bf16_kernelILb1E",)),
}


@pytest.fixture(scope="module")
def rows():
    with ThreadPoolExecutor(2) as ex:
        r3, k = ex.map(isa_census.census_rows, ["sdqn_kernels_r3.hip", "sdqn_kernels.hip"])
    return {"r3": r3, "k": k}


def _find(rows, parts):
    hit = [r for r in rows if all(p in r["name"] for p in parts)]
    assert len(hit) == 1, (parts, [r["name"][:90] for r in hit])
    return hit[0]


@pytest.mark.parametrize("launch", sorted(STEP_KERNELS))
def test_step_kernel_preloads_its_leading_block(rows, launch):
    tu, parts = STEP_KERNELS[launch]
    k = _find(rows[tu], parts)
    assert k["preload"] > 0, (launch, k["name"][:80], k["preload"])
    assert k["scratch"] == 0, (launch, k["scratch"])


def test_preload_costs_no_residency(rows):
    r3 = rows["r3"]
    for launch in ("bwd3", "bwd2"):
        k = _find(r3, STEP_KERNELS[launch][1])
        assert k["vgpr"] + k["agpr"] <= 128 and k["lds"] <= 80 * 1024, (launch, k["vgpr"], k["agpr"], k["lds"])
    conv2 = _find(r3, STEP_KERNELS["conv2_fwd"][1])
    assert conv2["vgpr"] + conv2["agpr"] <= 64 and conv2["lds"] <= 80 * 1024, (conv2["vgpr"], conv2["lds"])
    conv1 = _find(r3, STEP_KERNELS["conv1_fwd"][1])
    assert conv1["lds"] <= 80 * 1024


def test_no_kernel_of_either_unit_uses_scratch(rows):
    bad = [(r["name"][:80], r["scratch"]) for tu in rows.values() for r in tu if r["scratch"]]
    assert not bad, bad
