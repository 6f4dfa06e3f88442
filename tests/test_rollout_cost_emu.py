"""CPU tier: the costed rollout kernel (mujoco_jaco_amd/csrc/rollout_cost.h, jaco_rollout_cost) under the wavefront emulator against the
emulated jaco_rollout_fb and jaco_rollout, the cost formula in fp64 and itself (tests/rollout_cost_binding.py holds the emulated call,
the inputs, the cases and the reference; tests/test_gpu_rollout_cost.py is the GPU-tier twin).

Shapes: rollout_fb_binding.shared's as they are -- 67 rollouts on the default model, 9 on the others, 6 knots x hold 3; 8 rollouts of
50 knots x hold 1 on the arm-only model -- with goals distinct per plan and knot, weights distinct per word and noise on every ctrl
word (rollout_cost_binding.shared).  In every rollout the ctrl, state and pose terms and the last knot's share are each at least 1 % of
J (asserted on the fp64 side), so a dropped term shows.
Case 3, the cost against the fp64 formula on the call's own fp32 outputs, measure |J - J64| / J64 (terms: |t - t64| / J64):
  the derived cap (rollout_cost_binding.cap), (T (nx + 3 + nu) + 8) 2^-24: 1.1e-5 .. 9.0e-5 for these shapes;
  the largest value measured on the emulator over every set, both goal modes, with and without gains, hold 1 and 3:
      cost 1.57e-7, terms 1.17e-7  ->  tight bounds 4.7e-7 / 3.5e-7 (3 x measured).
  robot_config.rollout_cost against the same formula on trajectories=True's outputs: 1.52e-7 -> 4.5e-7.
The MPPI loop (3 envs, 16 samples with sample 0 noise-free, 6 knots x hold 2, 4 iterations, sigma 2.0, seed 5; the goal asks for joint
velocities of 0.15 rad/s, which 12 substeps of motor torque can reach), the nominal's cost at the end over its cost at the start, per
env, both models alike (the two-arm model's first arm is the single arm): greedy 0.726, 0.732, 0.916; temperature 0.05: 0.726, 0.728,
0.907.  Seed and temperature were chosen here, on the emulator.
Everything else is bit for bit.
"""
import numpy as np
import pytest

import rollout_binding as rb
import rollout_cost_binding as cb
import rollout_fb_binding as fbb
from emu_sim import EmuSim

COST_BOUND, TERMS_BOUND, CONFIG_BOUND = 4.7e-7, 3.5e-7, 4.5e-7
SETS = [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)]
COST_CASES = [(m, False, gpk, gains, hold) for m in (rb.MODEL,) + rb.SMALL for gpk in (0, 1) for gains in (False, True) for hold in (1, 3)] + \
             [(rb.LONG_MODEL, True, gpk, gains, 1) for gpk in (0, 1) for gains in (False, True)]


def run(model, ctrl, qpos0=None, qvel0=None, **k):
    return cb.rollout_cost(model, ctrl, qpos0, qvel0, **k)


def run_fb(model, ctrl, qpos0=None, qvel0=None, **k):
    return fbb.rollout_fb(model, ctrl, qpos0, qvel0, **k)


def run_open(model, ctrl, qpos0=None, qvel0=None, **k):
    return rb.rollout(model, ctrl, qpos0, qvel0, **k)


def make_sim(model, q, v):
    return EmuSim(model, q, v)


@pytest.mark.parametrize("model,long", SETS)
def test_without_noise_it_is_the_closed_loop_rollout(model, long):
    cb.case_degenerate(run, run_fb, model, long)


@pytest.mark.parametrize("model,long", SETS)
def test_noise_is_one_fp32_add(model, long):
    cb.case_noise(run, run_open, model, long)


@pytest.mark.parametrize("model,long,goal_per_knot,gains,hold", COST_CASES)
def test_cost_matches_the_fp64_formula(model, long, goal_per_knot, gains, hold):
    eJ, eT, cap = cb.case_cost(run, model, long, goal_per_knot, gains, hold)
    print("MEASURE cost %s%s goal_per_knot %d gains %d hold %d: cost %.3g terms %.3g (cap %.3g)" % (model, " 50 x 1" if long else "", goal_per_knot, gains, hold, eJ, eT, cap))
    assert eJ <= cap and eT <= cap, (eJ, eT, cap)
    assert eJ <= COST_BOUND and eT <= TERMS_BOUND, (eJ, eT)


@pytest.mark.parametrize("model,long", SETS)
def test_cost_does_not_depend_on_the_outputs_asked_for_and_is_deterministic(model, long):
    cb.case_independence(run, model, long)


def test_fan_out_through_the_indices():
    cb.case_fan_out(run)


def test_bad_indices_write_the_status_word_alone():
    cb.case_bad_index(run)


def test_a_non_finite_rollout_costs_infinity_and_its_neighbours_nothing():
    cb.case_non_finite(run)


@pytest.mark.parametrize("case", sorted(cb.REFUSALS))
def test_refusals(case):
    with pytest.raises(ValueError) as e:
        cb.rollout_cost(cb.REFUSAL_MODEL, **cb.refusal_args(case))
    assert str(e.value) == "emu_rollout_cost returned -1: jaco_rollout_cost: " + cb.REFUSALS[case]
    for k, x in e.value.outputs.items():
        assert (x == (cb.STATUS_SENTINEL if k == "status" else cb.SENTINEL)).all(), k


def test_eighteen_actuators_are_accepted():
    """The two-arm model has exactly JACO_ROLLOUT_COST_MAX_NU actuators: every ctrl weight is in use.  (No model here has more, so the
    refusal of nu > 18 -- jaco_rollout_cost_resolve's -- has no case among the refusals above.)"""
    g = cb.shared("jaco2_dual_torque")
    assert g["c"].shape[2] == 18
    w = np.arange(1.0, 19.0)
    r = run("jaco2_dual_torque", g["c"][:2], g["q"][:2], g["v"][:2], want=("cost", "ctrl"), hold=1, weights=dict(wu=w))
    J = 0.5 * (w * r["ctrl"].astype(np.float64) ** 2).sum((1, 2))
    assert np.abs(r["cost"] / J - 1).max() < 1e-6


def test_no_rollouts_is_not_an_error():
    g = cb.shared(rb.MODEL)
    r = run(rb.MODEL, g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "cost", "terms"))
    assert r["qpos"].shape == (0, rb.KNOTS, g["q"].shape[1]) and r["cost"].shape == (0,) and r["terms"].shape == (0, 3)


def test_a_null_goal_record_is_three_null_pointers():
    g = cb.shared(rb.MODEL)
    k = dict(hold=1, want=cb.COST, weights=dict(wu=g["weights"]["wu"]))
    a = run(rb.MODEL, g["c"][:3], g["q"][:3], g["v"][:3], **k)
    same = run(rb.MODEL, g["c"][:3], g["q"][:3], g["v"][:3], no_goal=True, **k)
    cb.same(a, same)
    assert (a["terms"][:, 1:] == 0).all() and (a["cost"] == a["terms"][:, 0]).all() and (a["cost"] > 0).all()


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_robot_config_cost_matches_the_fp64_formula(model):
    e, cap = cb.case_config_cost(make_sim, model)
    print("MEASURE robot_config.rollout_cost %s: cost %.3g (cap %.3g)" % (model, e, cap))
    assert e <= cap and e <= CONFIG_BOUND, (e, cap)


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_greedy_mppi_never_increases_the_cost(model):
    h = cb.case_mppi(make_sim, model, None)
    print("MEASURE greedy MPPI %s: cost ratios %s" % (model, np.array2string(h[-1] / h[0], precision=3)))
    assert (np.diff(h, axis=0) <= 0).all() and (h[-1] < h[0]).all()


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_mppi_at_a_finite_temperature_lowers_the_cost(model):
    h = cb.case_mppi(make_sim, model, cb.MPPI_TEMPERATURE)
    print("MEASURE MPPI %s temperature %g: cost ratios %s" % (model, cb.MPPI_TEMPERATURE, np.array2string(h[-1] / h[0], precision=3)))
    assert (h[-1] < h[0]).all(), h


def test_python_tier_messages():
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    g = cb.shared(rb.MODEL)
    sim = make_sim(rb.MODEL, g["q"], g["v"])
    n = len(g["q"])
    z = torch.zeros(3, 2, 9)
    with pytest.raises(ValueError, match=r"rollout_cost: ctrl has shape \(3, 9\), not \[P, T, 9\]"):
        sim.rollout_cost(torch.zeros(3, 9))
    with pytest.raises(ValueError, match=r"rollout_cost: noise has shape \(3, 1, 9\), not \[n, 2, 9\]"):
        sim.rollout_cost(z, noise=torch.zeros(3, 1, 9))
    with pytest.raises(ValueError, match="4 entries of plan_index but 3 entries of noise"):
        sim.rollout_cost(z, noise=torch.zeros(3, 2, 9), plan_index=[0, 1, 2, 0])
    with pytest.raises(ValueError, match=r"x_goal has shape \(3, 5\), not \[3, 4\] or \[3, 2, 4\]"):
        sim.rollout_cost(z, dofs=[0, 1], x_goal=torch.zeros(3, 5))
    with pytest.raises(ValueError, match="x_goal is given per plan but p_goal per plan and knot"):
        sim.rollout_cost(z, dofs=[0, 1], x_goal=torch.zeros(3, 4), p_goal=torch.zeros(3, 2, 3))
    with pytest.raises(ValueError, match=r"wx has shape \(3,\), not \[4\]"):
        sim.rollout_cost(z, dofs=[0, 1], x_goal=torch.zeros(3, 4), wx=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="want .* names none or not only outputs"):
        sim.rollout_cost(z, want=("cost", "reward"))
    with pytest.raises(ValueError, match="jaco_rollout_cost: a non-zero pose weight needs a frame"):
        sim.rollout_cost(z, p_goal=torch.zeros(3, 3), wp=1.0)
    with pytest.raises(ValueError, match="jaco_rollout_cost: weight wu\\[0\\] is negative or not finite"):
        sim.rollout_cost(z, wu=-1.0)
    r = sim.rollout_cost(torch.as_tensor(g["c"][:3]), hold=2, wu=1.0)
    assert sim.launches["jaco_rollout_cost"] == 3 and set(r) == {"cost", "terms", "status"} and r["cost"].shape == (3,) and r["terms"].shape == (3, 3)
    cfg = BatchedMujocoConfig(sim)
    with pytest.raises(ValueError, match=r"u has shape \(%d, 2, 9\), not \[%d, T, 6\]" % (n, n)):
        cfg.rollout_cost(torch.zeros(n, 2, 9))
    with pytest.raises(ValueError, match=r"noise has shape \(%d, 2, 6\), not \[%d, S, 2, 6\]" % (n, n)):
        cfg.rollout_cost(torch.zeros(n, 2, 6), noise=torch.zeros(n, 2, 6))
    with pytest.raises(ValueError, match="noise or alphas, not both"):
        cfg.rollout_cost(torch.zeros(n, 2, 6), noise=torch.zeros(n, 4, 2, 6), k=torch.zeros(n, 2, 6), alphas=[0.5, 1.0])
    with pytest.raises(ValueError, match="the goals .* are given all per env or all per env and knot"):
        cfg.rollout_cost(torch.zeros(n, 2, 6), q_goal=torch.zeros(n, 6), ee_goal=torch.zeros(n, 2, 3))
    with pytest.raises(ValueError, match="the temperature 0 is not positive"):
        cfg.mppi_update(torch.zeros(n, 2, 6), torch.zeros(n, 4, 2, 6), torch.zeros(n, 4), 0)
    # the line search's fan-out, and the update's handling of unusable samples
    a = cfg.rollout_cost(torch.zeros(n, 2, 6), k=torch.ones(n, 2, 6), alphas=[0.0, 0.5, 1.0], w_u=1.0)
    assert a["cost"].shape == (n, 3) and (a["cost"][:, 0] == 0).all() and (a["cost"][:, 1] < a["cost"][:, 2]).all()
    u, eps = torch.zeros(2, 1, 6), torch.arange(3.0).reshape(1, 3, 1, 1).expand(2, 3, 1, 6)
    cost = torch.tensor([[1.0, float("inf"), 1.0], [float("nan"), 2.0, 3.0]])
    status = torch.tensor([[0, 0, 16], [0, 8, 1]], dtype=torch.int32)
    un, w = cfg.mppi_update(u, eps, cost, 1.0, status=status)
    assert torch.equal(w, torch.tensor([[0.5, 0.0, 0.5], [0.0, 0.0, 0.0]])) and torch.equal(un[0], torch.full((1, 6), 1.0)) and torch.equal(un[1], u[1])
