"""CPU tier: the backward-pass kernel (mujoco_jaco_amd/csrc/lqr.h, jaco_lqr) on the wavefront emulator, through the product's own
BatchedMujoco.lqr_backward with the one launch replaced (tests/lqr_binding.py holds the inputs, the references and the cases;
tests/test_gpu_lqr.py is the GPU-tier twin).

Reference: the recursion of include/jaco_env.h in numpy fp64 on the same fp32 inputs.  Inputs: (nx, nu, T) = (2, 1, 1), (10, 3, 7),
(18, 6, 50), (36, 12, 50), (36, 18, 50) with the [q, dq] structure of one substep, (7, 2, 3) with a random stable A, three problems
each, 67 problems at (10, 3, 7), and the linearisation of the default model's nine hinge joints (18 x 6) over 50 knots; in the
reference every knot's smallest Cholesky pivot^2 is at least 1e-2 of max diag(Quu) (asserted; the smallest met is 5.2e-2).
Measures: per knot max |K - K_ref| / max |K_ref|, the same for k, per solve for Vxx0 and Vx0, |dV / dV_ref - 1| per entry.

Bounds = 3 x the largest value measured on the emulator over the eight sets and the regularised solve of case 5, rounded down:
  K / k / Vxx0 / Vx0 / dV against the fp64 recursion ......... 2.12e-6 / 2.38e-6 / 3.75e-6 / 2.02e-6 / 8.70e-7 -> 6.3e-6 / 7.1e-6 / 1.1e-5 / 6.0e-6 / 2.6e-6
  K of the LQR form against lqr_gains in fp64 (K's bound) ..... 2.07e-6
  relative excess of the closed loop's fp64 cost over the optimum ... 0 (smallest) .. 1.64e-12 (largest) -> at most 4.9e-12.  The floor
    asserted is -1e-13, not 0: the two costs are fp64 sums of up to 1e5 terms each, whose rounding is of the order of
    sqrt(1e5) x 1.1e-16 = 3.5e-14 of the cost; no undercut was measured on either tier
  |cost change from dx0 = 0 / (dV1 + dV2) - 1| ................. 9.65e-7 -> 2.8e-6
The loop closed through robot_config (the cases of the GPU tier, on the emulator): the posture-hold plan of rollout_fb_binding under the
gains of robot_config.lqr and under those of lqr_gains (fp64, rounded) agree within test_rollout_fb_emu.py's qpos / qvel bounds against
the fp64 closed loop (fd_binding.verr; measured 5.9e-8 / 3.7e-7; robot_config.lqr against lqr_gains there: 6.5e-7), and one iLQR iteration lowers the true cost at every step size tried
(to 0.81 .. 0.86 of the nominal's at alpha = 1).
"""
import numpy as np
import pytest

import lqr_binding as lb
from emu_sim import EmuSim

BOUNDS = dict(gain=6.3e-6, kff=7.1e-6, Vxx0=1.1e-5, Vx0=6.0e-6, dV=2.6e-6)
EXCESS, EXCESS_FLOOR, DV_IDENTITY = 4.9e-12, -1e-13, 2.8e-6
HOLD_BOUNDS = (1.5e-6, 7.8e-4)   # test_rollout_fb_emu.ORACLE_BOUNDS' qpos and qvel


@pytest.fixture(scope="module")
def sim():
    return EmuSim()


def within(m, bounds=BOUNDS):
    return all(m[k] <= bounds[k] for k in bounds)


@pytest.mark.parametrize("name", lb.SETS)
def test_against_the_fp64_recursion(sim, name):
    m = lb.case_reference(sim, name)
    print("MEASURE lqr emu %s: %s" % (name, {k: "%.3g" % v for k, v in m.items()}))
    assert within(m), m


@pytest.mark.parametrize("name", lb.SETS)
def test_lqr_form_against_lqr_gains(sim, name):
    m = lb.case_lqr(sim, name)
    print("MEASURE lqr emu %s: K against lqr_gains %.3g" % (name, m))
    assert m <= BOUNDS["gain"], m


@pytest.mark.parametrize("name", lb.SETS)
def test_closed_loop_is_optimal(sim, name):
    lo, hi, dv = lb.case_optimality(sim, name)
    print("MEASURE lqr emu %s: excess cost %.3g .. %.3g, dV identity %.3g" % (name, lo, hi, dv))
    assert EXCESS_FLOOR <= lo and hi <= EXCESS and dv <= DV_IDENTITY, (lo, hi, dv)


def test_layout_and_fan_out_bit_for_bit(sim):
    lb.case_layout(sim)


def test_regularisation_and_failure(sim):
    m = lb.case_failure(sim, BOUNDS)
    print("MEASURE lqr emu regularised: %s" % {k: "%.3g" % v for k, v in m.items()})
    assert within(m), m


@pytest.mark.parametrize("case", sorted(lb.REFUSALS))
def test_refusals(sim, case):
    lb.case_refusal(sim, case)


def test_one_launch_and_no_launch_for_nothing(sim):
    import torch
    g = lb.inputs("2x1x1")
    before = sim.launches["jaco_lqr"]
    lb.call(sim, g)
    assert sim.launches["jaco_lqr"] == before + 1
    r = sim.lqr_backward(*[torch.as_tensor(g[k]) for k in ("A", "B", "lxx", "luu")], problem_index=[])
    assert sim.launches["jaco_lqr"] == before + 1 and r["gain"].shape == (0, 1, 1, 2) and r["status"].shape == (0,)
    rc, why = sim.raw(*_good_records(g, 0))
    assert rc == 0, why   # n == 0 is accepted (and launches nothing)


def _good_records(g, n):
    import ctypes
    from mujoco_jaco_amd import _lib
    S = _lib.JACO_LQR_SHARED
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    keep = [np.ascontiguousarray(g[k]) for k in ("A", "B", "lxx", "luu", "Vxx")]
    out = np.zeros(16, np.float32)
    _good_records.keep = (keep, out)
    opt = _lib.JacoLqrOptions(nknots=1, nx=2, nu=1, shared_knots=S["lxx"] | S["luu"], shared_probs=S["lxx"] | S["luu"] | S["Vxx"])
    prob = _lib.JacoLqrProblem(p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), None, None, None, p(keep[4]), None, None, None, 3)
    return opt, n, prob, _lib.JacoLqrOut(None, None, p(out), None, None, None)


def test_robot_config_lqr_and_ilqr_backward():
    m = lb.case_config(EmuSim)
    print("MEASURE lqr emu robot_config.lqr against lqr_gains: %.3g" % m)
    assert m <= BOUNDS["gain"], m


def test_tvlqr_holds_a_posture_like_lqr_gains():
    eq, ev = lb.case_hold(EmuSim)
    print("MEASURE lqr emu posture hold: closed loops under lqr / lqr_gains differ by qpos %.3g, qvel %.3g" % (eq, ev))
    assert eq <= HOLD_BOUNDS[0] and ev <= HOLD_BOUNDS[1], (eq, ev)


def test_one_ilqr_iteration_lowers_the_true_cost():
    J0, J, dV, status = lb.case_ilqr(EmuSim)
    print("MEASURE lqr emu ilqr: nominal cost %s, best cost / nominal %s, dV1 %s" % (J0, J.min(1) / J0, dV[:, 0]))
    assert not status.any(), status
    assert (dV[:, 0] < 0).all(), dV
    assert (J.min(1) < J0).all(), (J, J0)


def test_python_surface_refuses_bad_shapes(sim):
    import torch
    g = {k: torch.as_tensor(v) for k, v in lb.inputs("10x3x7").items()}
    with pytest.raises(ValueError, match=r"A has shape \(3, 7, 10\)"):
        sim.lqr_backward(g["A"][..., 0], g["B"], g["lxx"], g["luu"])
    with pytest.raises(ValueError, match="lxx has shape"):
        sim.lqr_backward(g["A"], g["B"], g["lxx"][:9], g["luu"])
    with pytest.raises(ValueError, match="lx has shape"):
        sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], lx=g["lx"][:2])
    with pytest.raises(ValueError, match="rows and rows_out go together"):
        sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], rows=[0, 1, 2])
    with pytest.raises(ValueError, match="3 entries of problem_index but 2 entries of mu"):
        sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], problem_index=[0, 1, 2], mu=[0.0, 1.0])
    # Vxx None is lxx at the last knot; one mu serves every solve
    F = lb.full(lb.inputs("10x3x7"))
    a = lb.call(sim, lb.inputs("10x3x7"), lxx=F["lxx"].astype(np.float32), Vxx=None, mu=np.float32(1e-3))
    b = lb.call(sim, lb.inputs("10x3x7"), Vxx=lb.inputs("10x3x7")["lxx"], mu=np.full(3, 1e-3, np.float32))
    assert lb.same(a, b)
