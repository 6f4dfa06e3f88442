"""CPU tier: the cost-expansion kernel's resources on the three product builds, from the compiler's resource remarks the build keeps
(build/<variant>/kernel21.log, __graft_entry__.build_libs), as tests/test_rollout_fb_budget.py reads them: no scratch memory, LDS no larger
than the query kernel's (build/<variant>/kernel9.log: Jp and the nd x nd block live in the row area that kernel's walk borrows too) and
at most 128 VGPRs, which __launch_bounds__(64, 4) -- four waves per SIMD -- allows."""
import pytest

from test_rollout_fb_budget import remarks

KERNEL, QUERY = "_Z21jaco_cost_quad_kernel16JacoCostQuadArgs", "_Z17jaco_query_kernel13JacoQueryArgs"


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_the_expansion_costs_no_scratch_and_no_lds_beyond_the_query_kernels(variant):
    k, q = remarks(variant, "kernel21.log", KERNEL), remarks(variant, "kernel9.log", QUERY)
    print("%s: cost expansion %s, query %s" % (variant, k, q))
    assert k["scratch"] == 0, k
    assert k["lds"] <= q["lds"], (k, q)
    assert k["vgprs"] <= 128, k
