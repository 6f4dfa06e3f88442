"""CPU tier: the operational-space rollout kernel's resources on the three product builds, from the compiler's resource remarks the build
keeps (build/<variant>/kernel19.log, __graft_entry__.build_libs), as tests/test_rollout_fb_budget.py reads them: the LDS of the open-loop
kernel (build/<variant>/kernel15.log: the law's scratch is the row area s.J, free where it runs), at most 128 VGPRs, which
__launch_bounds__(64, 4) -- four waves per SIMD -- allows, and no scratch memory: all three builds attain it.  121 / 117 / 125 VGPRs on the
default / d12 / d30 build, occupancy 4 / 4 / 3 waves per SIMD (the open-loop kernel: 4 / 5 / 3).  Kernels 16 and 18 are held by their own
budget tests (test_rollout_fb_budget.py, test_rollout_cost_budget.py), which read kernel 15's remarks too."""
import pytest

from test_rollout_fb_budget import OPEN_LOOP, remarks

KERNEL = "_Z23jaco_rollout_osc_kernel18JacoRolloutOscArgs"


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_the_controller_costs_no_scratch_and_no_lds(variant):
    k, ol = remarks(variant, "kernel19.log", KERNEL), remarks(variant, "kernel15.log", OPEN_LOOP)
    print("%s: osc rollout %s, open loop %s" % (variant, k, ol))
    assert k["lds"] == ol["lds"], (k, ol)
    assert k["vgprs"] <= 128, k
    assert k["scratch"] == 0, k
