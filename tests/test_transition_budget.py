"""CPU tier: the transition-Jacobian kernel's resources on the three product builds, from the compiler's resource remarks the build
keeps (build/<variant>/kernel20.log, __graft_entry__.build_libs), as tests/test_rollout_fb_budget.py reads them: the LDS of the open-loop
rollout kernel (build/<variant>/kernel15.log: an evaluation is that kernel's substep and nothing is kept beside it), at most 128 VGPRs,
which __launch_bounds__(64, 4) -- four waves per SIMD -- allows, and no scratch memory.  110 / 98 / 128 VGPRs on the default / d12 / d30
build, occupancy 4 / 4 / 3 waves per SIMD (the open-loop kernel's, set by its LDS on d30).  Kernels 15, 16, 18 and 19 are held by their own
budget tests, unchanged."""
import pytest

from test_rollout_fb_budget import OPEN_LOOP, remarks

KERNEL = "_Z25jaco_transition_fd_kernel18JacoTransitionArgs"


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_the_column_loop_costs_no_scratch_and_no_lds(variant):
    k, ol = remarks(variant, "kernel20.log", KERNEL), remarks(variant, "kernel15.log", OPEN_LOOP)
    print("%s: transition %s, open loop %s" % (variant, k, ol))
    assert k["lds"] == ol["lds"], (k, ol)
    assert k["vgprs"] <= 128, k
    assert k["scratch"] == 0, k
