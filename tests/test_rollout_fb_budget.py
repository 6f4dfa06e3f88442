"""CPU tier: the closed-loop rollout kernel's resources on the three product builds, from the compiler's resource remarks the build keeps
(build/<variant>/kernel16.log, __graft_entry__.build_libs), as tests/test_lds_budget.py reads them: no scratch memory, the LDS of the
open-loop kernel (build/<variant>/kernel15.log: the feedback law uses no LDS beyond the step's) and at most 128 VGPRs, which
__launch_bounds__(64, 4) -- four waves per SIMD -- allows."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL, OPEN_LOOP = "_Z22jaco_rollout_fb_kernel17JacoRolloutFbArgs", "_Z19jaco_rollout_kernel15JacoRolloutArgs"


def remarks(variant, log, kernel):
    path = os.path.join(ROOT, "build", variant, log)
    assert os.path.exists(path), "%s is missing: build the library first (python __graft_entry__.py)" % path
    text = open(path).read()
    assert "Function Name: %s " % kernel in text

    def remark(name):
        m = re.findall(r"remark:\s+%s: (\d+)" % re.escape(name), text)
        assert len(m) == 1, (name, m)
        return int(m[0])
    return {k: remark(n) for k, n in (("lds", "LDS Size [bytes/block]"), ("vgprs", "VGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
                                      ("occupancy", "Occupancy [waves/SIMD]"))}


@pytest.mark.parametrize("variant", ("default", "d12", "d30"))
def test_the_law_costs_no_scratch_and_no_lds(variant):
    fbk, ol = remarks(variant, "kernel16.log", KERNEL), remarks(variant, "kernel15.log", OPEN_LOOP)
    print("%s: closed loop %s, open loop %s" % (variant, fbk, ol))
    assert fbk["scratch"] == 0, fbk
    assert fbk["lds"] == ol["lds"], (fbk, ol)
    assert fbk["vgprs"] <= 128, fbk
