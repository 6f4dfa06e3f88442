"""GPU tier: jaco_ik / BatchedMujoco.ik / BatchedMujocoConfig.ik on the MI355X -- the emulator tests' assertions at 4 096 envs (default
model) and 256 envs (the other layouts), agreement with the emulator, determinism, no side effects on the handle, and the round trip
through set_state / jaco_forward / get_xyz.

Margins as in test_ik_emu.py: position tol_pos + 5e-7 m (the project's xpos parity bound), rotation tol_rot + 4.5e-7 rad (3 x the excess
measured on the emulator, 1.47e-7; this file on the MI355X: 1.99e-7 near, 2.81e-7 in the joint-limit runs).  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import ik_binding as ib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError
from mujoco_jaco_amd.robot_config import BatchedMujocoConfig

pytestmark = pytest.mark.gpu

MODEL = "jaco2_curtain_torque"
TOL_POS, TOL_ROT = ib.DEFAULTS["tol_pos"], ib.DEFAULTS["tol_rot"]
POS_MARGIN, ROT_MARGIN = 5e-7, 4.5e-7


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_ik(sim, frame, seeds, P, Qt=None, **options):
    r = sim.ik(frame, _dev(P), _dev(Qt), _dev(seeds), **options)
    return {"qpos": r["qpos"].cpu().numpy(), "converged": r["converged"].cpu().numpy().astype(np.int32), "iters": r["iters"].cpu().numpy(),
            "resid": torch.stack([r["err_pos"], r["err_rot"]], 1).cpu().numpy()}


def assert_on_target(model, name, r, P, Qt, which=None, label=""):
    which = np.ones(len(P), bool) if which is None else which
    ep, er = ib.oracle_errors(model, name, [0, 0, 0], r["qpos"], P, Qt)
    print("%s: oracle |e_p| max %.3g (excess over the kernel's %.3g), |e_r| max %.3g (excess %.3g), iterations max %d" % (
        label, ep[which].max(), (ep - r["resid"][:, 0])[which].max(), er[which].max(), (er - r["resid"][:, 1])[which].max(), r["iters"][which].max()))
    assert (ep[which] < TOL_POS + POS_MARGIN).all(), ep[which].max()
    assert (er[which] < TOL_ROT + ROT_MARGIN).all(), er[which].max()
    return ep, er


@pytest.fixture(scope="module")
def big():
    B = 4096
    sim = BatchedMujoco(B, robot_file=MODEL)
    yield sim, ib.load_model(MODEL), sim.frames, ib.picking_seeds(MODEL, B)
    sim.close()


@pytest.mark.parametrize("pose", [True, False])
def test_near_targets(big, pose):
    sim, M, tab, seeds = big
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.3)
    Qt = Qt if pose else None
    r = gpu_ik(sim, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    assert (r["converged"] == 1).all(), int((r["converged"] == 1).sum())
    assert_on_target(MODEL, "EE", r, P, Qt, label="near x 4096, %s" % ("pose" if pose else "position"))


@pytest.mark.parametrize("pose", [True, False])
def test_far_targets(big, pose):
    """The cap of the emulator test at 4 096 envs: the restatement converges on >= 240 / 256 of the envs, the kernel on at least the
    restatement's count minus 3 (the emulator agrees with the restatement on every one of these 4 096 envs, pose and position)."""
    sim, M, tab, seeds = big
    B = len(seeds)
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 1.0)
    Qt = Qt if pose else None
    r = gpu_ik(sim, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    _, _, conv64, _ = ib.ik_fp64(M, tab, "EE", [0, 0, 0], seeds, P, Qt)
    c = r["converged"] == 1
    print("far x %d, %s: kernel converged %d, fp64 restatement %d; they disagree on %d envs" % (B, "pose" if pose else "position", c.sum(), conv64.sum(), (c != (conv64 == 1)).sum()))
    assert conv64.sum() >= 240 * B // 256
    assert c.sum() >= conv64.sum() - 3
    assert_on_target(MODEL, "EE", r, P, Qt, which=c, label="far, converged envs")
    assert (r["iters"][~c] == ib.DEFAULTS["max_iters"]).all()


def test_untouched_words(big):
    sim, M, tab, seeds = big
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.3)
    s = seeds.copy()
    s[:, 12:16] = np.random.default_rng(0).normal(size=(len(s), 4)).astype(np.float32)
    s[0, 9], s[1, 10], s[2, 7] = np.float32(1e-42), -0.0, np.float32(3e-39)
    f = tab.jaco_frame("EE", point=[0, 0, 0])
    r = gpu_ik(sim, f, s, P, Qt)
    assert (r["converged"] == 1).all()
    assert (bits(r["qpos"])[:, 6:] == bits(s)[:, 6:]).all()
    r = gpu_ik(sim, f, s, P, None, dof_mask=0b111110)
    assert (bits(r["qpos"])[:, 0] == bits(s)[:, 0]).all() and (bits(r["qpos"])[:, 6:] == bits(s)[:, 6:]).all()
    assert (bits(r["qpos"])[:, 1:6] != bits(s)[:, 1:6]).any(axis=0).all()


@pytest.mark.parametrize("ee", ["EE_1", "EE_2"])
def test_the_other_arm_is_untouched(ee):
    model = "jaco2_dual_torque"
    seeds = ib.picking_seeds(model, 256)
    sim = BatchedMujoco(256, robot_file=model)
    P, Qt, _ = ib.targets(model, ee, [0, 0, 0], seeds, 0.3)
    r = gpu_ik(sim, sim.frames.jaco_frame(ee, point=[0, 0, 0]), seeds, P, Qt)
    mine = np.zeros(seeds.shape[1], bool)
    mine[sim.frames.chain(ee)[0]] = True
    sim.close()
    assert (r["converged"] == 1).all()
    assert (bits(r["qpos"])[:, ~mine] == bits(seeds)[:, ~mine]).all()
    assert (bits(r["qpos"])[:, mine] != bits(seeds)[:, mine]).any(axis=0).all()


@pytest.mark.parametrize("case", ["out_of_reach", "beyond_joint_1"])
def test_joint_limits(big, case):
    sim, M, tab, seeds = big
    if case == "out_of_reach":
        P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.0)
        P = (P + np.float32([2, 0, 0])).astype(np.float32)
    else:
        g = seeds.copy()
        g[:, 1] = 0.3
        P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], g, 0.0, clamp=False)
    r = gpu_ik(sim, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    if case == "out_of_reach":
        assert (r["converged"] == 0).all() and (r["iters"] == ib.DEFAULTS["max_iters"]).all()
    rng = M["f_range"].reshape(-1, 2).astype(np.float32)
    for b in np.nonzero(M["f_limited"])[0]:
        a = int(M["f_qposadr"][b])
        assert (r["qpos"][:, a] >= rng[b, 0]).all() and (r["qpos"][:, a] <= rng[b, 1]).all(), b
    ep, er = ib.oracle_errors(MODEL, "EE", [0, 0, 0], r["qpos"], P, Qt)
    print("%s: converged %d; residual vs oracle: position %.3g, rotation %.3g" % (case, (r["converged"] == 1).sum(), np.abs(ep - r["resid"][:, 0]).max(),
                                                                               np.abs(er - r["resid"][:, 1]).max()))
    assert np.abs(ep - r["resid"][:, 0]).max() < POS_MARGIN
    assert np.abs(er - r["resid"][:, 1]).max() < ROT_MARGIN


@pytest.mark.parametrize("model,ee", [("jaco2_reaching_torque", "EE"), ("jaco2_torque", "EE"), ("jaco2_dual_torque", "EE_1")])
def test_other_layouts(model, ee):
    seeds = ib.picking_seeds(model, 256)
    sim = BatchedMujoco(256, robot_file=model)
    P, Qt, _ = ib.targets(model, ee, [0, 0, 0], seeds, 0.3)
    f = sim.frames.jaco_frame(ee, point=[0, 0, 0])
    for quat in (Qt, None):
        r = gpu_ik(sim, f, seeds, P, quat)
        assert (r["converged"] == 1).all(), int((r["converged"] == 1).sum())
        assert_on_target(model, ee, r, P, quat, label="%s %s, %s" % (model, ee, "pose" if quat is not None else "position"))
    sim.close()


def test_agrees_with_the_emulator_and_with_itself(big):
    """64 envs of the far set, pose targets: two GPU calls against each other (bit-identical), and the GPU against the emulated kernel.
    Observed on the MI355X: NOT bit-identical with the emulator (the device build contracts a * b + c into fma and uses the 2.5-ulp
    divide / sqrt, the host build does neither, so the iterates differ in their last bits and each stops at its own first iterate inside
    the tolerance): flags equal on all 64, iteration counts differ on 1 env, max |dqpos| over the 63 envs both converge on 3.04e-5 rad.
    Bound: 9e-5 rad, 3 x that measurement."""
    sim, M, tab, seeds = big
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 1.0)
    f = tab.jaco_frame("EE", point=[0, 0, 0])
    a, b = gpu_ik(sim, f, seeds, P, Qt), gpu_ik(sim, f, seeds, P, Qt)
    for k in ("qpos", "resid"):
        assert (bits(a[k]) == bits(b[k])).all(), k
    assert (a["iters"] == b["iters"]).all() and (a["converged"] == b["converged"]).all()
    e = ib.ik(MODEL, f, seeds[:64], P[:64], Qt[:64])
    c = (e["converged"] == 1) & (a["converged"][:64] == 1)
    dq = np.abs(a["qpos"][:64] - e["qpos"])[c].max()
    same = (bits(a["qpos"][:64]) == bits(e["qpos"])).all()
    print("GPU vs emulator, 64 envs: bit-identical %s, max |dqpos| over the %d envs both converge on %.3g, iteration counts differ on %d, flags on %d"
          % (same, c.sum(), dq, (a["iters"][:64] != e["iters"]).sum(), (a["converged"][:64] != e["converged"]).sum()))
    assert (a["converged"][:64] != e["converged"]).sum() <= 1
    assert dq < GPU_EMU_QPOS_BOUND


GPU_EMU_QPOS_BOUND = 9e-5   # rad; 3 x the 3.04e-5 measured on the MI355X, see the test's docstring


def test_ik_leaves_the_handle_alone():
    """State, flags and a following send_forces are bit-identical to a twin handle that never called jaco_ik."""
    B = 512
    seeds = ib.picking_seeds(MODEL, B)
    ctrl = _dev(np.random.default_rng(8).uniform(-0.2, 0.2, (B, 9)))
    sims = [BatchedMujoco(B, robot_file=MODEL) for _ in range(2)]
    for s in sims:
        s.set_state(_dev(seeds), None, None)
        s.send_forces(ctrl, nsub=5)
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.5)
    v = sims[0].state_version
    r = sims[0].ik(sims[0].frames.jaco_frame("EE", point=[0, 0, 0]), _dev(P), _dev(Qt))   # seed: the current state
    assert sims[0].state_version == v and r["converged"].sum().item() >= B * 240 // 256
    snap = lambda s: [t.clone() for t in s.get_state()] + [s.flags().clone(), s.sensordata().clone()]
    for x, y in zip(snap(sims[0]), snap(sims[1])):
        assert torch.equal(x, y)
    for s in sims:
        s.send_forces(ctrl, nsub=20)
    for x, y in zip(snap(sims[0]), snap(sims[1])):
        assert torch.equal(x, y)
    with pytest.raises(JacoError, match="max_iters"):
        sims[0].ik(sims[0].frames.jaco_frame("EE"), _dev(P), max_iters=257)
    with pytest.raises(JacoError, match="empty active"):
        sims[0].ik(sims[0].frames.jaco_frame("object_body"), _dev(P))
    for s in sims:
        s.close()


def test_round_trip_through_set_state_and_forward():
    """BatchedMujocoConfig.ik through env.robot_config, set_state with the result, jaco_forward: get_xyz("EE") is on the target."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    B = 1024
    env = JacoBatchedEnv(B, task="picking", seed=3)
    env.reset()
    cfg = env.robot_config
    q0 = env.sim.get_state()[0]
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], q0.cpu().numpy(), 0.3)
    q, ok = cfg.ik("EE", _dev(P), quat=_dev(Qt))
    assert isinstance(cfg, BatchedMujocoConfig) and ok.all() and q.shape == (B, 6)
    assert torch.equal(env.sim.get_state()[0], q0)
    qn = q0.clone()
    qn[:, cfg.arm_qadr] = q
    env.sim.set_state(qn.contiguous(), None, None)
    obs = env.make_observation()   # jaco_forward
    d = (env.sim.get_xyz("EE") - _dev(P)).norm(dim=1).max().item()
    assert torch.equal(obs[:, 1:4], env.sim.get_xyz("EE"))
    print("round trip: max |get_xyz(EE) - target| %.3g" % d)
    assert d < TOL_POS + POS_MARGIN
    assert ((cfg.Tx("EE") - _dev(P)).norm(dim=1) < TOL_POS + POS_MARGIN).all()
    env.close()
