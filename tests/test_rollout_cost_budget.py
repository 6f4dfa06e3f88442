"""CPU tier: the costed rollout kernel's resources on the three product builds, from the compiler's resource remarks the build keeps
(build/<variant>/kernel18.log, __graft_entry__.build_libs), as tests/test_rollout_fb_budget.py reads them: no scratch memory, the LDS of
the open-loop kernel (build/<variant>/kernel15.log: the cost uses no LDS beyond the step's) and at most 128 VGPRs, which
__launch_bounds__(64, 4) -- four waves per SIMD -- allows.  The one accumulator register per lane shows as one VGPR over the closed-loop
kernel: 109 / 98 / 128 on the default / d12 / d30 build, occupancy 4 / 4 / 3 waves per SIMD as that kernel's."""
import pytest

from test_rollout_fb_budget import OPEN_LOOP, remarks

KERNEL = "_Z24jaco_rollout_cost_kernel19JacoRolloutCostArgs"


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_the_cost_costs_no_scratch_and_no_lds(variant):
    ck, ol = remarks(variant, "kernel18.log", KERNEL), remarks(variant, "kernel15.log", OPEN_LOOP)
    print("%s: costed %s (occupancy %d waves/SIMD), open loop %s" % (variant, ck, ck["occupancy"], ol))
    assert ck["scratch"] == 0, ck
    assert ck["lds"] == ol["lds"], (ck, ol)
    assert ck["vgprs"] <= 128, ck
