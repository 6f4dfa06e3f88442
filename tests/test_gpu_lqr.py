"""GPU tier: jaco_lqr (mujoco_jaco_amd/csrc/lqr.h) on the MI355X through BatchedMujoco.lqr_backward and robot_config, the cases of
tests/lqr_binding.py (tests/test_lqr_emu.py is the CPU-tier twin, whose docstring states the reference, the inputs and the measures),
then the loop closed on the device: linearize -> ilqr_backward -> rollout_feedback (one iLQR iteration on jaco2_reaching_torque, 8 envs x
16 knots x 8 step sizes: at alpha = 1 the true cost falls to 0.81 .. 0.86 of the nominal's; no ratio is asserted).

Bounds = 3 x the largest value measured on the MI355X over the eight sets and the regularised solve of case 5, rounded down:
  K / k / Vxx0 / Vx0 / dV against the fp64 recursion ......... 2.14e-6 / 2.54e-6 / 3.75e-6 / 1.85e-6 / 1.51e-6 -> 6.4e-6 / 7.6e-6 / 1.1e-5 / 5.5e-6 / 4.5e-6
  K of the LQR form against lqr_gains in fp64 (K's bound) ..... 2.14e-6 (robot_config.lqr on the arm: 5.77e-7)
  relative excess of the closed loop's fp64 cost over the optimum ... 0 (smallest) .. 3.01e-12 (largest) -> at most 9.0e-12; the floor
    asserted is test_lqr_emu.py's -1e-13 (the rounding of the two fp64 sums); no undercut was measured
  |cost change from dx0 = 0 / (dV1 + dV2) - 1| ................. 1.51e-6 -> 4.5e-6
TVLQR posture hold: rollout_fb_binding's posture-hold plan with the gains of robot_config.lqr against the same plan with those of
lqr_gains (fp64, rounded to fp32): the two closed loops agree within test_gpu_rollout_fb.py's qpos / qvel bounds against the fp64
closed loop (fd_binding.verr; 1.2e-6 / 8.5e-4); measured 5.86e-8 / 1.7e-7.
"""
import ctypes

import pytest
import torch

import lqr_binding as lb
from mujoco_jaco_amd.physics import BatchedMujoco

pytestmark = pytest.mark.gpu
BOUNDS = dict(gain=6.4e-6, kff=7.6e-6, Vxx0=1.1e-5, Vx0=5.5e-6, dV=4.5e-6)
EXCESS, EXCESS_FLOOR, DV_IDENTITY = 9.0e-12, -1e-13, 4.5e-6
HOLD_BOUNDS = (1.2e-6, 8.5e-4)   # test_gpu_rollout_fb.ORACLE_BOUNDS' qpos and qvel


def _raw(self, opt, n, prob, out):
    """jaco_lqr as it is: (return code, jaco_last_error)."""
    cast = lambda s: None if s is None else ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)
    rc = self.L.jaco_lqr(self.h, cast(opt), int(n), cast(prob), cast(out), self._stream())
    return rc, self.L.jaco_last_error(self.h).decode()


@pytest.fixture(scope="module")
def sim():
    s = BatchedMujoco(1)   # (the entry reads neither the model nor the envs)
    s.raw = _raw.__get__(s)
    yield s
    s.close()


def make_sim(model, q, v):
    s = BatchedMujoco(len(q), robot_file=model)
    s.set_state(torch.tensor(q, device=s.device), torch.tensor(v, device=s.device), None)
    return s


def within(m, bounds=BOUNDS):
    return all(m[k] <= bounds[k] for k in bounds)


@pytest.mark.parametrize("name", lb.SETS)
def test_against_the_fp64_recursion(sim, name):
    m = lb.case_reference(sim, name)
    print("MEASURE lqr gpu %s: %s" % (name, {k: "%.3g" % v for k, v in m.items()}))
    assert within(m), m


@pytest.mark.parametrize("name", lb.SETS)
def test_lqr_form_against_lqr_gains(sim, name):
    m = lb.case_lqr(sim, name)
    print("MEASURE lqr gpu %s: K against lqr_gains %.3g" % (name, m))
    assert m <= BOUNDS["gain"], m


@pytest.mark.parametrize("name", lb.SETS)
def test_closed_loop_is_optimal(sim, name):
    lo, hi, dv = lb.case_optimality(sim, name)
    print("MEASURE lqr gpu %s: excess cost %.3g .. %.3g, dV identity %.3g" % (name, lo, hi, dv))
    assert EXCESS_FLOOR <= lo and hi <= EXCESS and dv <= DV_IDENTITY, (lo, hi, dv)


def test_layout_and_fan_out_bit_for_bit(sim):
    lb.case_layout(sim)


def test_regularisation_and_failure(sim):
    m = lb.case_failure(sim, BOUNDS)
    print("MEASURE lqr gpu regularised: %s" % {k: "%.3g" % v for k, v in m.items()})
    assert within(m), m


@pytest.mark.parametrize("case", sorted(lb.REFUSALS))
def test_refusals(sim, case):
    lb.case_refusal(sim, case)


def test_robot_config_lqr_and_ilqr_backward():
    m = lb.case_config(make_sim)
    print("MEASURE lqr gpu robot_config.lqr against lqr_gains: %.3g" % m)
    assert m <= BOUNDS["gain"], m


def test_tvlqr_holds_a_posture_like_lqr_gains():
    eq, ev = lb.case_hold(make_sim)
    print("MEASURE lqr gpu posture hold: closed loops under lqr / lqr_gains differ by qpos %.3g, qvel %.3g" % (eq, ev))
    assert eq <= HOLD_BOUNDS[0] and ev <= HOLD_BOUNDS[1], (eq, ev)


def test_one_ilqr_iteration_lowers_the_true_cost():
    J0, J, dV, status = lb.case_ilqr(make_sim)
    print("MEASURE lqr gpu ilqr: nominal cost %s, best cost / nominal %s, dV1 %s" % (J0, J.min(1) / J0, dV[:, 0]))
    assert not status.any(), status
    assert (dV[:, 0] < 0).all(), dV
    assert (J.min(1) < J0).all(), (J, J0)
