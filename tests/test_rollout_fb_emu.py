"""CPU tier: the closed-loop rollout kernel (mujoco_jaco_amd/csrc/rollout_fb.h, jaco_rollout_fb) under the wavefront emulator against the
emulated open-loop kernel, the law recomputed in fp64, the fp64 oracle in closed loop and itself (tests/rollout_fb_binding.py holds the
emulated call, the inputs, the cases and the references; tests/test_gpu_rollout_fb.py is the GPU-tier twin).

Shapes: rollout_binding's -- 67 rollouts on the default model, 9 on the others, 6 knots x hold 3; 8 rollouts of 50 knots x hold 1 on the
arm-only model.  Gains over every hinge dof of the model (9, 12 or 18 dofs), x_ref and the conditions the inputs meet in closed loop:
rollout_fb_binding.gains / reference_states / shared.
Reference of case 4 (fp64): the oracle with contacts disabled, the law in fp64 on the oracle's own state at each evaluation, both
modes.  Error measure: fd_binding.verr, max |x - ref| / (1 + |ref|), over every knot's qpos and qvel and every evaluation's ctrl.
Bounds = 3 x the largest value measured on the emulator:
  qpos / qvel / ctrl against the fp64 closed loop, four models, 6 x 3, both modes ... 4.94e-7 / 2.59e-4 / 1.87e-4 -> 1.5e-6 / 7.8e-4 / 5.6e-4
  qpos / qvel / ctrl against the fp64 closed loop, arm-only model, 50 x 1 ........... 8.06e-8 / 3.30e-5 / 1.27e-5 -> 2.4e-7 / 9.9e-5 / 3.8e-5
The law against its fp64 recomputation: the derived bound of rollout_fb_binding.law_bound, (nx + 3) 2^-24 (|ctrl| + |alpha kff| +
sum |gain| |d|) per word; the largest ratio measured is 0.36 (robot_config tier: 0.14).
Everything else is bit for bit: the degenerate call and the zero-deviation call against the emulated jaco_rollout, the closed loop
against jaco_rollout on its own commands, the fan-out through the indices against materialised plans and states.
"""
import pytest

import rollout_binding as rb
import rollout_fb_binding as fbb
from emu_sim import EmuSim

ORACLE_BOUNDS = (1.5e-6, 7.8e-4, 5.6e-4)
LONG_BOUNDS = (2.4e-7, 9.9e-5, 3.8e-5)
SETS = [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)]


def run(model, ctrl, qpos0=None, qvel0=None, **k):
    return fbb.rollout_fb(model, ctrl, qpos0, qvel0, **k)


def run_open(model, ctrl, qpos0=None, qvel0=None, **k):
    return rb.rollout(model, ctrl, qpos0, qvel0, **k)


def make_sim(model, q, v):
    return EmuSim(model, q, v)


def within(m, bounds):
    return all(x <= b for x, b in zip(m, bounds))


@pytest.mark.parametrize("model,long", SETS)
def test_without_feedback_it_is_the_open_loop_rollout(model, long):
    fbb.case_degenerate(run, run_open, model, long)


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", (rb.MODEL,) + rb.SMALL)
def test_a_closed_loop_is_an_open_loop_on_its_own_commands(model, per_substep):
    fbb.case_own_commands(run, run_open, model, per_substep)


def test_fifty_knots_are_an_open_loop_on_their_own_commands():
    fbb.case_own_commands(run, run_open, rb.LONG_MODEL, 0, long=True)


@pytest.mark.parametrize("model,long", SETS)
def test_the_law(model, long):
    w = fbb.case_law(run, model, long)
    print("MEASURE law %s%s: largest |u - u_ref| / bound %.3g" % (model, " 50 x 1" if long else "", w))
    assert w <= 1.0, w


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", (rb.MODEL,) + rb.SMALL)
def test_every_knot_matches_the_closed_loop_oracle(model, per_substep):
    eq, ev, eu, _ = fbb.case_oracle(run, model, per_substep)
    print("MEASURE oracle %s per_substep %d: qpos %.3g qvel %.3g ctrl %.3g" % (model, per_substep, eq, ev, eu))
    assert within((eq, ev, eu), ORACLE_BOUNDS), (eq, ev, eu)


def test_fifty_knots_match_the_closed_loop_oracle():
    eq, ev, eu, _ = fbb.case_oracle(run, rb.LONG_MODEL, 0, long=True)
    print("MEASURE oracle %s 50 x 1: qpos %.3g qvel %.3g ctrl %.3g" % (rb.LONG_MODEL, eq, ev, eu))
    assert within((eq, ev, eu), LONG_BOUNDS), (eq, ev, eu)


@pytest.mark.parametrize("model,long", SETS)
def test_zero_deviation_is_the_open_loop_rollout(model, long):
    fbb.case_zero_deviation(run, run_open, model, long)


def test_fan_out_through_the_indices():
    fbb.case_fan_out(run)


def test_bad_indices_are_flagged_and_write_nothing_else():
    fbb.case_bad_index(run)


@pytest.mark.parametrize("case", sorted(fbb.REFUSALS))
def test_refusals(case):
    with pytest.raises(ValueError) as e:
        fbb.rollout_fb(fbb.REFUSAL_MODEL, **fbb.refusal_args(case))
    assert str(e.value) == "emu_rollout_fb returned -1: jaco_rollout_fb: " + fbb.REFUSALS[case]
    for k, x in e.value.outputs.items():
        assert (x == (fbb.STATUS_SENTINEL if k == "status" else fbb.SENTINEL)).all(), k


def test_no_rollouts_is_not_an_error():
    g = rb.shared(rb.MODEL)
    r = run(rb.MODEL, g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "ctrl"))
    assert r["qpos"].shape == (0, rb.KNOTS, g["q"].shape[1]) and r["ctrl"].shape == (0, rb.KNOTS, 9)


def test_status_or_ctrl_alone_is_an_output():
    g = fbb.shared(rb.MODEL)
    full = fbb.closed(run, rb.MODEL)
    for k in ("status", "ctrl"):
        alone = run(rb.MODEL, g["c"][:5], g["q"], g["v"], hold=g["hold"], want=(k,), **fbb.plan_args(g, slice(0, 5)))
        assert set(alone) == {k} and (fbb.bits(alone[k]) == fbb.bits(full[k][:5])).all()


@pytest.mark.parametrize("model", sorted(fbb.HOLD_MODELS))
def test_robot_config_holds_a_posture(model):
    w = fbb.case_hold_posture(make_sim, model)
    print("MEASURE robot_config.rollout_feedback %s: first knot's |u - u_ref| / bound %.3g" % (model, w))
    assert w <= 1.0, w


def test_python_tier_messages():
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    g = fbb.shared(rb.MODEL)
    sim = make_sim(rb.MODEL, g["q"], g["v"])
    n = len(g["q"])
    with pytest.raises(ValueError, match=r"ctrl has shape \(3, 9\), not \[P, T, 9\]"):
        sim.rollout_feedback(torch.zeros(3, 9))
    with pytest.raises(ValueError, match="feedforward has shape"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), feedforward=torch.zeros(3, 1, 9))
    with pytest.raises(ValueError, match="a gain needs dofs"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), gain=torch.zeros(3, 2, 9, 4))
    with pytest.raises(ValueError, match=r"gain has shape \(3, 2, 9, 4\), not \[3, 2, 9, 6\]"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), gain=torch.zeros(3, 2, 9, 4), dofs=[0, 1, 2])
    with pytest.raises(ValueError, match=r"x_ref has shape None, not \[3, 2, 4\]"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), gain=torch.zeros(3, 2, 9, 4), dofs=[0, 1])
    with pytest.raises(ValueError, match="alpha needs feedforward"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), alpha=torch.ones(3))
    with pytest.raises(ValueError, match="4 entries of plan_index but 3 entries of alpha"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), feedforward=torch.zeros(3, 2, 9), plan_index=[0, 1, 2, 0], alpha=torch.ones(3))
    with pytest.raises(ValueError, match="jaco_rollout_fb: dof 9 belongs to a free joint"):
        sim.rollout_feedback(torch.zeros(3, 2, 9), gain=torch.zeros(3, 2, 9, 4), x_ref=torch.zeros(3, 2, 4), dofs=[0, 9])
    r = sim.rollout_feedback(torch.as_tensor(g["c"][:3]), hold=2, per_substep=True, final_only=True)
    assert sim.launches["jaco_rollout_fb"] == 2 and set(r) == {"qpos", "qvel", "status", "ctrl"} and r["qpos"].shape == (3, 1, 23) and r["ctrl"].shape == (3, 12, 9)
    cfg = BatchedMujocoConfig(sim)
    with pytest.raises(ValueError, match=r"u has shape \(%d, 2, 9\), not \[%d, T, 6\]" % (n, n)):
        cfg.rollout_feedback(torch.zeros(n, 2, 9))
    with pytest.raises(ValueError, match=r"K has shape .* not \[%d, 2, 6, 12\]" % n):
        cfg.rollout_feedback(torch.zeros(n, 2, 6), K=torch.zeros(n, 2, 6, 6))
    with pytest.raises(ValueError, match="alphas need k"):
        cfg.rollout_feedback(torch.zeros(n, 2, 6), alphas=[0.5, 1.0])
