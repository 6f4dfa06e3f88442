"""CPU tier: the rollout kernel (mujoco_jaco_amd/csrc/rollout.h, jaco_rollout) under the wavefront emulator against the fp64 oracle, the
emulated step kernel, the emulated query and itself (tests/rollout_binding.py holds the emulated call, the inputs, the cases and the
references; tests/test_gpu_rollout.py is the GPU-tier twin).

Reference (fp64): the oracle with contacts disabled; per rollout qpos / qvel at the fp32 inputs and a zero warm start, then
step(ctrl_k, hold) per knot.  Error measure: fd_binding.verr, max |x - ref| / (1 + |ref|), over every knot's qpos and qvel.
Shapes: 67 rollouts on the default model, 9 on the others, 6 knots x hold 3; 8 rollouts of 50 knots x hold 1 on the arm-only model.
The inputs have limit rows over the horizon in a third to two thirds of the rollouts and none in at least a fifth, stay off the actuator
model's knife edges and keep every limit row further from its threshold than one fp32 spacing per substep taken (asserted in the
binding on the fp64 side).
Bounds = 3 x the largest value measured on the emulator:
  qpos / qvel against the oracle, four models, 6 x 3 ........................... 2.55e-7 / 1.07e-4 -> 7.7e-7 / 3.2e-4
  qpos / qvel against the oracle, arm-only model, 50 x 1 ....................... 4.35e-8 / 8.87e-6 -> 1.3e-7 / 2.7e-5
  xpos / xmat against the emulated query at the returned qpos rows ............. 1.20e-7 / 3.00e-7 -> 3.6e-7 / 9.0e-7
    (the rollout's pose sees the compensated low words of the state, the query its fp32 rounding)
  robot_config: first knot's dq against dq + h forward_dynamics, two models .... 1.90e-8 -> 5.7e-8
Against the emulated step kernel (set_state, then send_forces(ctrl_k, hold) + get_state per knot with the low words kept, as a handle
keeps them) the emulated rollout is the same host code and agrees bit for bit, flags included.
"""
import pytest

import query_binding as qb
import rollout_binding as rb
from emu_sim import EmuSim

ORACLE_BOUNDS = (7.7e-7, 3.2e-4)
LONG_BOUNDS = (1.3e-7, 2.7e-5)
FRAME_BOUNDS = (3.6e-7, 9.0e-7)
CONFIG_BOUND = 5.7e-8


def run(model, ctrl, qpos0=None, qvel0=None, **k):
    return rb.rollout(model, ctrl, qpos0, qvel0, **k)


def query(model, qpos, qvel, frame):
    r = qb.query(model, qpos, qvel, [frame], want=("xpos", "xmat"))
    return r["xpos"][:, 0], r["xmat"][:, 0]


def make_sim(model, q, v):
    return EmuSim(model, q, v)


def within(m, bounds):
    return all(x <= b for x, b in zip(m, bounds))


@pytest.mark.parametrize("model", (rb.MODEL,) + rb.SMALL)
def test_every_knot_matches_the_oracle(model):
    eq, ev, _ = rb.case_oracle(run, model)
    print("MEASURE oracle %s: qpos %.3g qvel %.3g" % (model, eq, ev))
    assert within((eq, ev), ORACLE_BOUNDS), (eq, ev)


def test_fifty_knots_match_the_oracle():
    eq, ev, _ = rb.case_oracle(run, rb.LONG_MODEL, long=True)
    print("MEASURE oracle %s 50 x 1: qpos %.3g qvel %.3g" % (rb.LONG_MODEL, eq, ev))
    assert within((eq, ev), LONG_BOUNDS), (eq, ev)


@pytest.mark.parametrize("model,long", [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)])
def test_the_rollout_is_the_emulated_step_kernel_bit_for_bit(model, long):
    g = rb.shared(model, long)
    r = run(model, g["c"], g["q"], g["v"], want=("qpos", "qvel", "status"), hold=g["hold"])
    Q, V, flags = rb.emu_steps(model, g["q"], g["v"], g["c"], g["hold"])
    assert (rb.bits(r["qpos"]) == rb.bits(Q)).all() and (rb.bits(r["qvel"]) == rb.bits(V)).all()
    assert (r["status"] == flags).all()


def test_frame_outputs_match_the_query():
    m = rb.case_frames(run, query)
    print("MEASURE frames: xpos %.3g xmat %.3g" % m)
    assert within(m, FRAME_BOUNDS), m


def test_bitwise_self_consistency():
    rb.case_self_consistency(run)


def test_bad_state_indices_are_flagged_and_write_nothing_else():
    rb.case_bad_index(run)


@pytest.mark.parametrize("case", sorted(rb.REFUSALS))
def test_refusals(case):
    with pytest.raises(ValueError) as e:
        rb.rollout(rb.REFUSAL_MODEL, **rb.refusal_args(case))
    assert str(e.value) == "emu_rollout returned -1: jaco_rollout: " + rb.REFUSALS[case]
    for k, x in e.value.outputs.items():
        assert (x == (rb.STATUS_SENTINEL if k == "status" else rb.SENTINEL)).all(), k


def test_no_rollouts_is_not_an_error():
    g = rb.shared(rb.MODEL)
    r = run(rb.MODEL, g["c"][:0], g["q"], g["v"], want=("qpos",))
    assert r["qpos"].shape == (0, rb.KNOTS, g["q"].shape[1])


@pytest.mark.parametrize("model", (rb.MODEL, "jaco2_dual_torque"))
def test_robot_config_rollout(model):
    e = rb.case_config(make_sim, model)
    print("MEASURE robot_config.rollout %s: first knot's dq against dq + h forward_dynamics %.3g" % (model, e))
    assert e <= CONFIG_BOUND, e


def test_python_tier_messages():
    import torch
    g = rb.shared(rb.MODEL)
    sim = make_sim(rb.MODEL, g["q"], g["v"])
    with pytest.raises(ValueError, match=r"not \[n, T, 9\]"):
        sim.rollout(torch.zeros(3, 9))
    with pytest.raises(ValueError, match="3 ctrl sequences but 2 state indices"):
        sim.rollout(torch.zeros(3, 2, 9), state_index=[0, 1])
    with pytest.raises(ValueError, match="jaco_rollout: nknots 2 x hold 0"):
        sim.rollout(torch.zeros(3, 2, 9), hold=0)
    r = sim.rollout(torch.as_tensor(g["c"][:3]), hold=2, final_only=True)
    assert sim.launches["jaco_rollout"] == 2 and set(r) == {"qpos", "qvel", "status"} and r["qpos"].shape == (3, 1, 23)
