"""GPU tier: stage T (csrc/collision.h stage_touch / ray_hits_site) on the MI355X, held to an fp64 restatement of the stage fed the device's
own contact record (BatchedMujoco.record_contacts, read raw; sensordata()) -- the assertions of tests/test_touch_emu.py, from
tests/touch_binding.py, on the three builds.  One substep from set_state with zero velocity and warm start.

Measured, MI355X (worst |kernel - recomputation| / bound, the bound being (10 + n_k) 2^-23 sum fn; knife readings / non-zero readings;
pipeline figure |kernel - oracle sensordata| / largest reading, printed only) -- census and tiers identical to the emulator's:
  default  43 states   0.054   3 / 210   6.2e-7
  old       4 states   0.022   0 / 19    4.3e-6
  sensor   19 states   0.000   0 / 8     1.7e-4 (the 14 golden poses alone: 5.3e-4)
  dual     20 states   0.056   0 / 140   2.1e-6"""
import numpy as np
import pytest
import torch

import touch_binding as tb
from mujoco_jaco_amd.physics import BatchedMujoco

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def _run(name, q, ctrl, cap=128):
    B = len(q)
    sim = BatchedMujoco(B, robot_file=name)
    sim.record_contacts(cap)
    sim.set_state(_dev(q), torch.zeros(B, sim.nv, device="cuda:0"), torch.zeros(B, sim.nv, device="cuda:0"))
    sim.clear_flags()
    sim.send_forces(_dev(np.broadcast_to(ctrl, (B, sim.nu))), nsub=1)
    out = (sim._crec.cpu().numpy(), sim._cn.cpu().numpy(), sim.sensordata().cpu().numpy(), sim.flags().cpu().numpy().astype(np.uint32), sim.stats().cpu().numpy())
    sim.close()
    return out


@pytest.mark.parametrize("key", list(tb.SETS))
def test_stage_against_its_own_record(key):
    """tests/test_touch_emu.py, same name: every reading that is not knife within (10 + n_k) 2^-23 sum(fn) of the fp64 recomputation from the
    device's record, exactly 0 where nothing counts, nothing overflowed, knife readings below 2 % of the non-zero ones, the census on the
    record (default: every tier a touched env ends on, contacts past the 64th on sensor bodies, the early-out both ways)."""
    tb.check_set(key, _run, "MI355X")


def test_arm_only_model_reads_zero():
    """jaco2_reaching_torque under disable_contact (the contact-free kernel): sensordata is all zeros after a step."""
    sim = BatchedMujoco(3, robot_file="jaco2_reaching_torque")
    sim.set_option("disable_contact", 1)
    sim.send_forces(torch.full((3, 9), 0.1, device="cuda:0"), nsub=2)
    s = sim.sensordata().cpu().numpy()
    sim.close()
    assert s.shape == (3, 20) and (s == 0).all()
