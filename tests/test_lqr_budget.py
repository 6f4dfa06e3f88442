"""CPU tier: the backward-pass kernel's resources on the three product builds, from the compiler's resource remarks the build keeps
(build/<variant>/kernel17.log, __graft_entry__.build_libs), as tests/test_rollout_fb_budget.py reads them: no scratch memory, and at
most 32 000 bytes of LDS per workgroup -- 25 of the 1 280-byte granules, so that five workgroups fit a CU.  The kernel reads no model,
so the three builds hold the same code; registers and occupancy are recorded in DESIGN.md, not pinned."""
import pytest

from test_rollout_fb_budget import remarks

KERNEL = "_Z15jaco_lqr_kernel11JacoLqrArgs"


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_no_scratch_and_five_workgroups_per_cu(variant):
    r = remarks(variant, "kernel17.log", KERNEL)
    print("%s: backward pass %s" % (variant, r))
    assert r["scratch"] == 0, r
    assert r["lds"] <= 32000, r
