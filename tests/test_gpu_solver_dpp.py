"""GPU tier: the dense solver blocks and the controller's 6x6 eliminations with the pivot row as a DPP operand of the multiply-adds
(solver_blocks.h JACO_SOLVER_DPP: ldl_block, ldl_block0_dual, gj_inverse6, gj_solve6) against the read-lane forms, on the device.

If the build with the read-lane forms (tools/build_variant.sh solverbcast, -DJACO_SOLVER_DPP=0) lies next to the product library, both
libraries run, each in a fresh child process with its own time limit, and must agree bit for bit:
  (a) the 256-env picking case of tests/test_gpu_solver_blocks.py (4 env steps x frame_skip 2, seed 41: one env in eight gets small actions
      -- arm-row solves, side rows, bigger tiers -- env 200 spawns the hand in the pedestal; the controller runs every substep) on qpos, qvel,
      qacc, obs, reward and done after every env step, with the error flags 0 and qacc finite;
  (b) 64 envs x 20 substeps at ctrl level under disable_contact (the contact-free kernel) on qpos, qvel and qacc.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = "libjaco_env_solverbcast.so"
NSTEP = 4   # (of the picking case)
BF, NSUB = 64, 20


def _contact_free(qpos0):
    """Case (b) on the library JACO_ENV_LIB names: the state after 20 substeps of raw torques without contacts."""
    from mujoco_jaco_amd import workload
    from mujoco_jaco_amd.physics import BatchedMujoco
    q = workload.reset_states(qpos0, BF, seed=7, f32_draws=True)
    c = workload.random_ctrl(BF, seed=8, scale=0.2).astype(np.float32)
    env = BatchedMujoco(BF, device=0)
    env.set_option("disable_contact", 1)
    env.set_state(torch.tensor(q, dtype=torch.float32, device=env.device), None, None)
    env.send_forces(torch.tensor(c, device=env.device), nsub=NSUB)
    st = env.get_state()
    out = {"qpos": st[0].cpu().numpy(), "qvel": st[1].cpu().numpy(), "qacc": st[2].cpu().numpy(), "flags": env.flags().cpu().numpy()}
    env.close()
    return out


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from mujoco_jaco_amd.modelc import blob
import test_gpu_solver_blocks as T
import test_gpu_solver_dpp as D
M = blob.load(%r)
np.savez(sys.argv[1], **(T._gpu_rollout(M["qpos0"]) if sys.argv[2] == "picking" else D._contact_free(M["qpos0"])))
"""


def _both(tmp_path, case):
    if not os.path.exists(os.path.join(ROOT, "mujoco_jaco_amd", VARIANT)):
        pytest.skip("%s not built (tools/build_variant.sh solverbcast -DJACO_SOLVER_DPP=0)" % VARIANT)
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
    res = {}
    for lib in ("libjaco_env.so", VARIANT):
        out = str(tmp_path / (lib + ".npz"))
        subprocess.run([sys.executable, "-c", code, out, case], env={**os.environ, "JACO_ENV_LIB": lib}, check=True, timeout=120)   # (a failure ends the test)
        res[lib] = np.load(out)
    return res["libjaco_env.so"], res[VARIANT]


def test_picking_case_same_bits_as_the_read_lane_build(tmp_path):
    a, b = _both(tmp_path, "picking")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 2 + 6 * NSTEP
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["flags"] & 15).max() == 0
    assert all(np.isfinite(a["qacc%d" % (s + 1)]).all() for s in range(NSTEP))


def test_contact_free_kernel_same_bits_as_the_read_lane_build(tmp_path):
    a, b = _both(tmp_path, "contact_free")
    assert sorted(a.files) == sorted(b.files) == ["flags", "qacc", "qpos", "qvel"]
    for k in ("qpos", "qvel", "qacc"):
        assert a[k].shape[0] == BF and a[k].tobytes() == b[k].tobytes(), k
    assert (a["flags"] & 15).max() == 0 and np.isfinite(a["qacc"]).all()
