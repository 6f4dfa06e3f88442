"""CPU tier: robot_config -- the MJCF-name frame table (against host FK, the oracle and the blob's own frames) and BatchedMujocoConfig's
shapes, arm selection and caching on a stand-in sim whose query runs on the emulated kernel."""
import os

import numpy as np
import pytest
import torch

import query_binding as qb
from emu_sim import EmuSim
from mujoco_jaco_amd.modelc import blob, kin, rot
from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, FrameTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["jaco2_curtain_torque", "jaco2_reaching_torque", "jaco2_torque", "jaco2_dual_torque"]


def _model(name):
    return blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", name + ".jacomdl"))


@pytest.mark.parametrize("model", MODELS)
def test_frame_table_composes_to_the_oracle_body_poses(model):
    """Every named non-mocap MJCF body: host FK of its fused body's weld root, composed with the table's pose, is the oracle's xpos / xmat."""
    from oracle_binding import Oracle
    T = FrameTable.for_model(model)
    M = T.M
    roots = {fb: r for r, fb in T.fid.items()}
    q, _ = qb.random_states(M, 8, 5)
    o = Oracle(model)
    worst = 0.0
    for e in range(8):
        qe = q[e].astype(np.float64)
        xpos, xquat, _, _ = kin.fk(M, qe)
        o.set("qpos", qe); o.set("qvel", np.zeros(int(M["nv"][0]))); o.forward()
        oxp, oxm = o.get("xpos").reshape(-1, 3), o.get("xmat").reshape(-1, 3, 3)
        for name in T.bodies:
            if not name or M["body_mocapid"][T.bodies.index(name)] >= 0:
                continue
            fb, p, qf = T.frame(name)
            if fb < 0:
                wp, wR = p, rot.quat_to_mat(qf)
            else:
                r = roots[fb]
                Rr = rot.quat_to_mat(xquat[r])
                wp, wR = xpos[r] + Rr @ p, Rr @ rot.quat_to_mat(qf)
            b = T.bodies.index(name)
            worst = max(worst, np.abs(wp - oxp[b]).max(), np.abs(wR - oxm[b]).max())
    print("%s: worst body pose difference %.3g" % (model, worst))
    assert worst < 1e-12   # measured 4.4e-16 .. 6.7e-16 (fp64 rounding of the compositions)


@pytest.mark.parametrize("model", MODELS)
def test_frame_table_equals_the_blob_frames(model):
    """The frames the model compiler stored (f_frame_EE, _EE_obj, _link1, _object_body, _object_dest): the same numbers exactly."""
    T = FrameTable.for_model(model)
    n = 0
    for key in T.M:
        if key.startswith("f_frame_"):
            fb, p, q = T.frame(key[len("f_frame_"):])
            assert np.array_equal(np.concatenate([[fb], p, q]), T.M[key]), key
            n += 1
    assert n >= (0 if model == "jaco2_dual_torque" else 2)   # (the two-arm model carries none: it has no env tier)


def test_mocap_and_unknown_names_are_refused():
    T = FrameTable.for_model("jaco2_curtain_torque")
    with pytest.raises(ValueError, match="markers"):
        T.jaco_frame("hand")
    with pytest.raises(ValueError, match="unknown"):
        T.jaco_frame("no_such_body")
    sim = EmuSim("jaco2_curtain_torque", *qb.random_states(T.M, 2, 1))
    with pytest.raises(ValueError):
        BatchedMujocoConfig(sim).J("subgoal_reach")


def test_config_shapes_arm_and_caching_on_the_default_model():
    M = _model("jaco2_curtain_torque")
    q, v = qb.random_states(M, 6, 3)
    sim = EmuSim("jaco2_curtain_torque", q, v)
    cfg = BatchedMujocoConfig(sim)
    assert cfg.arm == list(range(6)) and cfg.arm_qadr == list(range(6))
    J, Mq, g = cfg.J("EE"), cfg.M(), cfg.g()
    assert J.shape == (6, 6, 6) and Mq.shape == (6, 6, 6) and g.shape == (6, 6)
    assert cfg.J("EE", full=True).shape == (6, 6, 21) and cfg.M(full=True).shape == (6, 21, 21) and cfg.g(full=True).shape == (6, 21)
    n = sim.launches["jaco_query"]
    R, quat, x = cfg.R("object_body"), cfg.quaternion("object_body"), cfg.Tx("object_body")
    assert R.shape == (6, 3, 3) and quat.shape == (6, 4) and x.shape == (6, 3)
    assert sim.launches["jaco_query"] == n + 1   # a new name: one launch for every registered frame; then the cached result
    cfg.J("EE"), cfg.R("object_body"), cfg.M()
    assert sim.launches["jaco_query"] == n + 1
    sim.state_version += 1
    cfg.g()
    assert sim.launches["jaco_query"] == n + 2
    # the numbers are the query's: g = -qfrc_bias[arm]; the oracle's for poses and the quaternion (up to sign)
    r = sim.query([sim.frames.jaco_frame("EE")])
    assert torch.equal(cfg.g(), -r["qfrc_bias"][:, :6]) and torch.equal(cfg.M(), r["qM"][:, :6, :6])
    assert torch.equal(cfg.J("EE"), r["jac"][:, 0, :, :6])
    o = qb.oracle_answers("jaco2_curtain_torque", q, v, [sim.frames.body_id("object_body")])
    assert np.array_equal(x.numpy(), o["xpos"][:, 0])   # (a free body's position is its qpos: exact)
    from oracle_binding import Oracle
    orc = Oracle()
    b = sim.frames.body_id("object_body")
    for e in range(6):
        orc.set("qpos", q[e].astype(np.float64)); orc.forward()
        oq = orc.get("xquat").reshape(-1, 4)[b]
        assert min(np.abs(quat[e].numpy() - oq).max(), np.abs(quat[e].numpy() + oq).max()) < 2e-7   # measured 7.6e-8
    off = torch.tensor([0.01, -0.02, 0.03])
    assert torch.equal(cfg.Tx("object_body", x=off), x + R @ off)


def test_config_joint_override_is_spliced_into_qpos():
    """q = [B, n_arm] replaces the arm angles of the current state (qvel kept): the same outputs as a state with those angles."""
    M = _model("jaco2_curtain_torque")
    q, v = qb.random_states(M, 4, 8)
    sim = EmuSim("jaco2_curtain_torque", q, v)
    cfg = BatchedMujocoConfig(sim)
    qa = torch.tensor(np.random.default_rng(9).uniform(-1, 1, (4, 6)), dtype=torch.float32)
    J_over, g_over = cfg.J("EE", q=qa), cfg.g(q=qa)
    q2 = q.copy()
    q2[:, :6] = qa.numpy()
    cfg2 = BatchedMujocoConfig(EmuSim("jaco2_curtain_torque", q2, v))
    assert torch.equal(J_over, cfg2.J("EE")) and torch.equal(g_over, cfg2.g())
    assert not torch.equal(J_over, cfg.J("EE"))


def test_config_arms_of_the_two_arm_model():
    M = _model("jaco2_dual_torque")
    q, v = qb.random_states(M, 3, 4)
    sim = EmuSim("jaco2_dual_torque", q, v)
    c1, c2 = BatchedMujocoConfig(sim, ee="EE_1"), BatchedMujocoConfig(sim, ee="EE_2")
    assert len(c1.arm) == 6 and len(c2.arm) == 6 and not set(c1.arm) & set(c2.arm) and max(c1.arm + c2.arm) < 18
    J1, J2 = c1.J("EE_1", full=True), c1.J("EE_2", full=True)
    s1, s2 = (J1 != 0).any(0).any(0), (J2 != 0).any(0).any(0)
    assert s1.nonzero().flatten().tolist() == c1.arm and s2.nonzero().flatten().tolist() == c2.arm
    assert c1.J("EE_1").shape == (3, 6, 6) and c2.M().shape == (3, 6, 6)
