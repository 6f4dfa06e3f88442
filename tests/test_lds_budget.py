"""CPU tier: the light kernels' LDS and register budget, from the compiler's resource remarks the build keeps (build/default/kernel<n>.log,
__graft_entry__.build_libs).  MI355X hands LDS out in blocks of 1 280 bytes (160 KB / 128; measured, profiles/residency.txt): twelve
one-wave workgroups fit a CU up to 12 800 bytes each, eleven beyond.  168 VGPRs are what three waves per SIMD -- twelve per CU -- allow."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_GRANULE, LDS_PER_CU, ENVS_PER_CU = 1280, 160 * 1024, 12
LDS_TARGET = LDS_PER_CU // ENVS_PER_CU // LDS_GRANULE * LDS_GRANULE


def test_target_is_twelve_granule_rounded_workgroups_per_cu():
    assert LDS_TARGET == 12800 and ENVS_PER_CU * LDS_TARGET <= LDS_PER_CU < ENVS_PER_CU * (LDS_TARGET + LDS_GRANULE)


@pytest.mark.parametrize("log,kernel", [("kernel0.log", "_Z19jaco_physics_kernel12JacoStepArgs"), ("kernel1.log", "_Z26jaco_physics_kernel_listed12JacoStepArgs")])
def test_light_kernels_fit_twelve_envs_per_cu(log, kernel):
    path = os.path.join(ROOT, "build", "default", log)
    assert os.path.exists(path), "%s is missing: build the library first (python __graft_entry__.py)" % path
    text = open(path).read()
    assert "Function Name: %s " % kernel in text

    def remark(name):
        m = re.findall(r"remark:\s+%s: (\d+)" % re.escape(name), text)
        assert len(m) == 1, (name, m)
        return int(m[0])
    lds, vgprs = remark("LDS Size [bytes/block]"), remark("VGPRs")
    print("%s: LDS %d B (target <= %d), VGPRs %d, scratch %d B/lane" % (kernel, lds, LDS_TARGET, vgprs, remark("ScratchSize [bytes/lane]")))
    assert lds <= LDS_TARGET, lds
    assert vgprs == 168, vgprs
    assert remark("Occupancy [waves/SIMD]") == 3
