"""GPU tier: jaco_query / robot_config.BatchedMujocoConfig on the MI355X -- oracle parity of poses, Jacobians, qM, qfrc_bias in the three
library builds, consistency with the env's observation, no side effects, a gravity-compensated closed loop and the two-arm model."""
import numpy as np
import pytest
import torch

import query_binding as qb
from mujoco_jaco_amd import workload
from mujoco_jaco_amd.modelc import blob
from mujoco_jaco_amd.physics import BatchedMujoco
from mujoco_jaco_amd.robot_config import BatchedMujocoConfig

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def _parity(model, names, q, v):
    sim = BatchedMujoco(q.shape[0], robot_file=model)
    sim.set_state(_dev(q), _dev(v), None)
    r = {k: t.cpu().numpy() for k, t in sim.query([sim.frames.jaco_frame(n) for n in names]).items()}
    o = qb.oracle_answers(model, q, v, [sim.frames.body_id(n) for n in names])
    sim.close()
    assert ((r["jac"] == 0).all(axis=2) == (o["jac"] == 0).all(axis=2)).all()
    assert (r["qM"] == np.transpose(r["qM"], (0, 2, 1))).all()
    qm_rel = (np.abs(r["qM"] - o["qM"]).max(axis=(1, 2)) / np.abs(o["qM"]).max(axis=(1, 2))).max()
    bias_rel = (np.abs(r["qfrc_bias"] - o["qfrc_bias"]).max(1) / np.maximum(np.abs(o["qfrc_bias"]).max(1), 1e-9)).max()
    errs = (np.abs(r["xpos"] - o["xpos"]).max(), np.abs(r["xmat"] - o["xmat"]).max(), np.abs(r["jac"] - o["jac"]).max(), qm_rel, bias_rel)
    print("%s x %d: xpos %.3g, xmat %.3g, jac %.3g, qM rel %.3g, qfrc_bias rel %.3g" % ((model, q.shape[0]) + errs))
    return errs


def test_oracle_parity_default_model():
    """jaco2_curtain_torque, 1 024 envs: picking resets with random velocities."""
    M = blob.load(qb.os.path.join(qb.ASSETS, "jaco2_curtain_torque.jacomdl"))
    q = workload.reset_states(M["qpos0"], 1024, seed=3, f32_draws=True).astype(np.float32)
    v = (np.random.default_rng(4).normal(size=(1024, 21)) * 0.5).astype(np.float32)
    errs = _parity("jaco2_curtain_torque", ["EE", "object_body", "link3", "thumb_distal"], q, v)
    # bounds of the emulator test (3x its measurement: xpos 1.24e-7, xmat 2.71e-7, jac 2.73e-7, qM rel 5.4e-8, qfrc_bias rel 1.42e-7)
    for e, b in zip(errs, (3.5e-7, 8e-7, 8e-7, 1.6e-7, 4e-7)):
        assert e < b, (errs, b)


@pytest.mark.parametrize("model,names", [("jaco2_torque", ["EE", "link3", "thumb_distal"]),
                                         ("jaco2_dual_torque", ["EE_1", "EE_2", "object_body_1", "link3_1", "thumb_distal_1"])])
def test_oracle_parity_d12_d30(model, names):
    """The _d12 and _d30 builds, 256 envs each."""
    q, v = qb.random_states(blob.load(qb.os.path.join(qb.ASSETS, model + ".jacomdl")), 256, 7)
    errs = _parity(model, names, q, v)
    # bounds of the emulator test (3x the largest emulator measurement of the three non-default models)
    for e, b in zip(errs, (5e-7, 9e-7, 9e-7, 1.9e-6, 2.2e-6)):
        assert e < b, (errs, b)


def test_ee_and_object_positions_equal_the_observation():
    """After env.reset() on 4 096 envs (picking), get_xyz("EE") is obs[:, 1:4] and get_xyz("object_body") obs[:, 8:11]."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    env = JacoBatchedEnv(4096, task="picking", seed=3)
    obs = env.reset()
    ee, ob = env.sim.get_xyz("EE"), env.sim.get_xyz("object_body")
    d_ee = (ee - obs[:, 1:4]).abs().max().item()
    print("EE vs obs[1:4]: max |diff| %.3g; object vs obs[8:11]: %.3g" % (d_ee, (ob - obs[:, 8:11]).abs().max().item()))
    assert torch.equal(ob, obs[:, 8:11])
    assert torch.equal(ee, obs[:, 1:4])
    env.close()


def test_query_has_no_side_effects():
    """A query writes nothing of the handle: state, flags, task rows, sensordata bit-identical before and after; send_forces with queries
    interleaved gives the states of the same run without them; an override equal to the state gives the in-place query's bits."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    env = JacoBatchedEnv(1024, task="picking", seed=5)
    env.reset()
    env.step(torch.zeros(1024, 7, device="cuda:0"))
    snap = lambda: [t.clone() for t in env.sim.get_state()] + [env.sim.flags().clone(), env.task_state().clone(), env.sim.sensordata().clone()]
    before = snap()
    cfg = env.robot_config
    cfg.J("EE"), cfg.M(), cfg.g(), cfg.R("object_body")
    r_state = env.sim.query([env.sim.frames.jaco_frame("EE")])
    r_over = env.sim.query([env.sim.frames.jaco_frame("EE")], qpos=before[0].clone(), qvel=before[1].clone())
    torch.cuda.synchronize()
    for a, b in zip(before, snap()):
        assert torch.equal(a, b)
    for k in r_state:
        assert torch.equal(r_state[k], r_over[k]), k
    env.close()
    M = blob.load(qb.os.path.join(qb.ASSETS, "jaco2_curtain_torque.jacomdl"))
    q = _dev(workload.reset_states(M["qpos0"], 512, seed=9, f32_draws=True))
    ctrl = _dev(workload.random_ctrl(512, seed=10, scale=0.3))
    finals = []
    for interleave in (False, True):
        sim = BatchedMujoco(512)
        sim.set_state(q, None, None)
        frames = [sim.frames.jaco_frame(n) for n in ("EE", "object_body", "link3")]
        for _ in range(10):
            if interleave:
                sim.query(frames)
            sim.send_forces(ctrl, nsub=1)
        finals.append(sim.get_state())
        torch.cuda.synchronize()
        sim.close()
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def _closed_loop_gpu(q0, nsub, gc=True):
    sim = BatchedMujoco(q0.shape[0], robot_file="jaco2_reaching_torque")
    sim.set_option("disable_contact", 1)
    cfg = BatchedMujocoConfig(sim)
    assert cfg.arm == list(range(6))
    qt = _dev(q0)
    sim.set_state(qt.clone(), torch.zeros(q0.shape[0], 9, device="cuda:0"), torch.zeros(q0.shape[0], 9, device="cuda:0"))
    for _ in range(nsub):
        fb = sim.get_feedback()
        u = qb.KP * (qt[:, :6] - fb["q"]) - qb.KD * fb["dq"]
        if gc:
            u = u - cfg.g()
        sim.send_forces(torch.cat([u, qt[:, 6:9]], 1).contiguous(), nsub=1)
    q = sim.get_state()[0].cpu().numpy().astype(np.float64)
    sim.close()
    return q


def test_closed_loop_gravity_compensation_against_the_oracle():
    """jaco2_reaching_torque (contacts off), 1 024 envs, 500 substeps of ctrl[arm] = -g() + PD with the fingers held, against the same loop
    on the fp64 oracle; without the -g term the arm sags."""
    q0 = qb.hold_states(1024, 21)
    q = _closed_loop_gpu(q0, 500)
    o = qb.closed_loop_oracle(q0, 500)
    drift = np.abs(q[:, :6] - o[:, :6]).max()
    q_nog = _closed_loop_gpu(q0, 500, gc=False)
    sag_with, sag_without = np.abs(q[:, :6] - q0[:, :6]).max(1), np.abs(q_nog[:, :6] - q0[:, :6]).max(1)
    print("closed loop: drift vs oracle %.3g; sag with -g max %.3g, without min %.3g (ratio %.3g)" % (drift, sag_with.max(), sag_without.min(), sag_without.min() / sag_with.max()))
    # emulator measurement (16 envs, tests/query_binding.closed_loop_emu): drift 4.17e-7 -> bound 3x
    assert drift < 1.25e-6, drift
    # oracle measurement (64 envs): sag with -g at most 1.67e-7, without at least 1.68e-2 -- a factor 1e5; required here: 100
    assert sag_without.min() > 100 * sag_with.max()


def test_two_arm_jacobians():
    """JacoBatchedEnv(n_robots=2).robot_config: J("EE_1") / J("EE_2") match the oracle; their column supports are disjoint."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    env = JacoBatchedEnv(256, n_robots=2)
    q, v = qb.random_states(blob.load(qb.os.path.join(qb.ASSETS, "jaco2_dual_torque.jacomdl")), 256, 17)
    env.sim.set_state(_dev(q), _dev(v), None)
    cfg = env.robot_config
    J1, J2 = cfg.J("EE_1", full=True).cpu().numpy(), cfg.J("EE_2", full=True).cpu().numpy()
    o = qb.oracle_answers("jaco2_dual_torque", q, v, [env.sim.frames.body_id("EE_1"), env.sim.frames.body_id("EE_2")])
    err = max(np.abs(J1 - o["jac"][:, 0]).max(), np.abs(J2 - o["jac"][:, 1]).max())
    print("two arms: J error %.3g" % err)
    assert err < 9e-7, err   # the d30 parity bound above (emulator jac 2.99e-7, 3x)
    s1, s2 = (J1 != 0).any(axis=(0, 1)), (J2 != 0).any(axis=(0, 1))
    assert s1.sum() == 6 and s2.sum() == 6 and not (s1 & s2).any()
    assert cfg.J("EE_1").shape == (256, 6, 6)
    env.close()
