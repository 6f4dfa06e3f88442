"""CPU tier: the robot-configuration query kernel (mujoco_jaco_amd/csrc/query.h) under the wavefront emulator, against the fp64 oracle's
sim.forward() -- body poses, mj_jacBodyCom, qM, qfrc_bias -- in all three layouts of the library (default, _d12, _d30)."""
import os

import numpy as np
import pytest

import query_binding as qb
from mujoco_jaco_amd import workload
from mujoco_jaco_amd.modelc import blob
from mujoco_jaco_amd.robot_config import FrameTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name):
    return blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", name + ".jacomdl"))


def _errors(model, names, q, v):
    T = FrameTable.for_model(model)
    r = qb.query(model, q, v, [T.jaco_frame(n) for n in names])
    o = qb.oracle_answers(model, q, v, [T.body_id(n) for n in names])
    qm_rel = np.abs(r["qM"] - o["qM"]).max(axis=(1, 2)) / np.abs(o["qM"]).max(axis=(1, 2))
    bias_rel = np.abs(r["qfrc_bias"] - o["qfrc_bias"]).max(1) / np.maximum(np.abs(o["qfrc_bias"]).max(1), 1e-9)
    zero_cols = (o["jac"] == 0).all(axis=2)   # dofs that do not move the body: exactly zero columns in both
    assert ((r["jac"] == 0).all(axis=2) == zero_cols).all()
    assert (r["qM"] == np.transpose(r["qM"], (0, 2, 1))).all()
    return (np.abs(r["xpos"] - o["xpos"]).max(), np.abs(r["xmat"] - o["xmat"]).max(), np.abs(r["jac"] - o["jac"]).max(), qm_rel.max(), bias_rel.max())


def _check(errs, bounds):
    for what, e, b in zip(("xpos", "xmat", "jac", "qM rel", "qfrc_bias rel"), errs, bounds):
        assert e < b, (what, e, b)


CURTAIN_NAMES = ["EE", "object_body", "link3", "thumb_distal"]


def test_curtain_reset_states_match_oracle():
    """jaco2_curtain_torque, 256 envs: the picking reset distribution with random velocities."""
    M = _model("jaco2_curtain_torque")
    q = workload.reset_states(M["qpos0"], 256, seed=3, f32_draws=True).astype(np.float32)
    v = (np.random.default_rng(4).normal(size=(256, 21)) * 0.5).astype(np.float32)
    errs = _errors("jaco2_curtain_torque", CURTAIN_NAMES, q, v)
    print("curtain reset states: xpos %.3g, xmat %.3g, jac %.3g, qM rel %.3g, qfrc_bias rel %.3g" % errs)
    # measured: xpos 1.24e-7, xmat 2.71e-7, jac 2.73e-7, qM rel 5.4e-8, qfrc_bias rel 1.42e-7 (the stage-dump test holds qM to 1e-6)
    _check(errs, (3.5e-7, 8e-7, 8e-7, 1.6e-7, 4e-7))


def test_curtain_states_after_oracle_substeps_match_oracle():
    """... and the states 20 oracle substeps of random ctrl later (object falling, hand moving)."""
    from oracle_binding import Oracle
    M = _model("jaco2_curtain_torque")
    qo = workload.reset_states(M["qpos0"], 256, seed=3, f32_draws=True)
    vo, wo = np.zeros((256, 21)), np.zeros((256, 21))
    Oracle().step_batch(qo, vo, wo, np.ascontiguousarray(workload.random_ctrl(256, seed=5, scale=0.3)), nsub=20, nthreads=4)
    errs = _errors("jaco2_curtain_torque", CURTAIN_NAMES, qo.astype(np.float32), vo.astype(np.float32))
    print("curtain after 20 substeps: xpos %.3g, xmat %.3g, jac %.3g, qM rel %.3g, qfrc_bias rel %.3g" % errs)
    # measured: xpos 1.18e-7, xmat 2.92e-7, jac 2.87e-7, qM rel 5.89e-8, qfrc_bias rel 1.46e-7
    _check(errs, (3.5e-7, 8e-7, 8e-7, 1.6e-7, 4e-7))


@pytest.mark.parametrize("model,names", [
    ("jaco2_reaching_torque", ["EE", "link3", "thumb_distal"]),                              # default layout, arm only (9 dofs)
    ("jaco2_torque", ["EE", "link3", "thumb_distal"]),                                       # _d12 build
    ("jaco2_dual_torque", ["EE_1", "EE_2", "object_body_1", "link3_1", "thumb_distal_1"]),   # _d30 build: two arms, two free objects
])
def test_other_models_match_oracle(model, names):
    q, v = qb.random_states(_model(model), 64, 7)
    errs = _errors(model, names, q, v)
    print("%s: xpos %.3g, xmat %.3g, jac %.3g, qM rel %.3g, qfrc_bias rel %.3g" % ((model,) + errs))
    # measured (reaching / torque / dual): xpos 1.71e-7 / 1.35e-7 / 1.71e-7, xmat 2.09e-7 / 2.04e-7 / 2.99e-7, jac 2.04e-7 / 2.1e-7 / 2.99e-7,
    # qM rel 3.77e-7 / 3.81e-7 / 6.35e-7, qfrc_bias rel 6.01e-7 / 7.13e-7 / 7.61e-7: every bound 3x the largest of the three
    _check(errs, (5e-7, 9e-7, 9e-7, 1.9e-6, 2.2e-6))


def test_override_is_bit_identical_to_the_stepped_state():
    """The state an emulated step left in its buffers, queried in place, and the same floats handed in as a separate override (envs
    permuted on the way in, un-permuted on the way out): bit-identical outputs, every output."""
    from emu_binding import EmuEnv
    e = EmuEnv("jaco2_curtain_torque", 32)
    M = e.M
    e.qpos[:] = workload.reset_states(M["qpos0"], 32, seed=11, f32_draws=True).astype(np.float32)
    e.step(workload.random_ctrl(32, seed=12, scale=0.3).astype(np.float32), nsub=5)
    T = FrameTable.for_model("jaco2_curtain_torque")
    frames = [T.jaco_frame(n) for n in CURTAIN_NAMES]
    a = qb.query("jaco2_curtain_torque", e.qpos, e.qvel, frames)
    perm = np.random.default_rng(13).permutation(32)
    qp, qv = np.array(e.qpos[perm].astype(np.float64), np.float32), np.array(e.qvel[perm].astype(np.float64), np.float32)
    b = qb.query("jaco2_curtain_torque", qp, qv, frames)
    inv = np.argsort(perm)
    for k in qb.OUTS:
        assert np.array_equal(a[k], b[k][inv]), k


def test_ee_and_object_frames_reproduce_the_observation():
    """After a reset's forward pass (emulated jaco_reset), the "EE" frame's position is obs[1:4] and "object_body"'s obs[8:11], bit for bit:
    the frame is composed with ee_frame's float sequence."""
    from emu_binding import EmuJacoEnv
    e = EmuJacoEnv("jaco2_curtain_torque", 32, task_id=0, seed=5)
    for k in range(32):
        e.reset_env(k)
    obs = e.forward()
    T = FrameTable.for_model("jaco2_curtain_torque")
    r = qb.query("jaco2_curtain_torque", e.qpos, e.qvel, [T.jaco_frame("EE"), T.jaco_frame("object_body")], want=("xpos",))
    assert np.array_equal(r["xpos"][:, 0], obs[:, 1:4])
    assert np.array_equal(r["xpos"][:, 1], obs[:, 8:11])


def test_null_outputs_and_argument_checks():
    """Outputs not asked for are not written (NaN sentinels stay); an out-of-range body or frame count is refused."""
    from mujoco_jaco_amd import _lib
    T = FrameTable.for_model("jaco2_curtain_torque")
    q, v = qb.random_states(_model("jaco2_curtain_torque"), 4, 1)
    r = qb.query("jaco2_curtain_torque", q, v, [T.jaco_frame("EE")], want=("jac",))
    full = qb.query("jaco2_curtain_torque", q, v, [T.jaco_frame("EE")])
    assert set(r) == {"jac"} and np.array_equal(r["jac"], full["jac"])
    bad = _lib.JacoFrame()
    bad.body = 11   # 11 fused bodies: 0 .. 10
    with pytest.raises(ValueError):
        qb.query("jaco2_curtain_torque", q, v, [bad])
    with pytest.raises(ValueError):
        qb.query("jaco2_curtain_torque", q, v, [T.jaco_frame("EE")] * 17)
