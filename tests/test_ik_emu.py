"""CPU tier: the inverse-kinematics kernel (mujoco_jaco_amd/csrc/ik.h, jaco_ik) under the wavefront emulator, judged by the fp64 oracle's
forward kinematics and compared with the fp64 numpy restatement of the algorithm (tests/ik_binding.py).

Margins.  Position: tol_pos + 5e-7 m, the project's bound on xpos parity with the oracle (test_query_emu.py).  Rotation: tol_rot + 4.5e-7
rad = 3 x the measured excess -- the largest |oracle e_r - kernel e_r| over the near and far sets of the default model was 1.47e-7 rad
(position: 1.21e-7 m, inside the 5e-7).  The other layouts measured 1.1e-7 .. 1.4e-7 rad.
"""
import numpy as np
import pytest

import ik_binding as ib
import query_binding as qb
from emu_sim import EmuSim
from mujoco_jaco_amd import _lib

MODEL = "jaco2_curtain_torque"
B = 256
TOL_POS, TOL_ROT = ib.DEFAULTS["tol_pos"], ib.DEFAULTS["tol_rot"]
POS_MARGIN, ROT_MARGIN = 5e-7, 4.5e-7
POINT = [0.02, -0.03, 0.05]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_on_target(model, name, point, r, P, Qt, which=None, label=""):
    """Check 1's oracle test for the envs `which` (default: all): the oracle's FK at the returned qpos is on the target."""
    which = np.ones(len(P), bool) if which is None else which
    ep, er = ib.oracle_errors(model, name, point, r["qpos"], P, Qt)
    print("%s: oracle |e_p| max %.3g (excess over the kernel's %.3g), |e_r| max %.3g (excess %.3g), iterations max %d" % (
        label, ep[which].max(), (ep - r["resid"][:, 0])[which].max(), er[which].max(), (er - r["resid"][:, 1])[which].max(), r["iters"][which].max()))
    assert (ep[which] < TOL_POS + POS_MARGIN).all(), ep[which].max()
    assert (er[which] < TOL_ROT + ROT_MARGIN).all(), er[which].max()
    return ep, er


@pytest.fixture(scope="module")
def default_model():
    return ib.load_model(MODEL), ib.table_of(MODEL), ib.picking_seeds(MODEL, B)


@pytest.mark.parametrize("pose", [True, False])
def test_near_targets_converge_onto_the_target(default_model, pose):
    """s = 0.3: every env converges, and the oracle's FK at the returned qpos is on the target."""
    M, tab, seeds = default_model
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.3)
    Qt = Qt if pose else None
    r = ib.ik(MODEL, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    assert (r["converged"] == 1).all(), int((r["converged"] == 1).sum())
    assert r["iters"].max() <= 8   # (the fp64 restatement: at most 6)
    assert_on_target(MODEL, "EE", [0, 0, 0], r, P, Qt, label="near, %s" % ("pose" if pose else "position"))


@pytest.mark.parametrize("pose", [True, False])
def test_far_targets_match_the_fp64_restatement(default_model, pose):
    """s = 1.0: the restatement converges on >= 240 of 256, the kernel on at least that minus 3; flagged envs are on target; the others ran out."""
    M, tab, seeds = default_model
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 1.0)
    Qt = Qt if pose else None
    r = ib.ik(MODEL, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    _, _, conv64, _ = ib.ik_fp64(M, tab, "EE", [0, 0, 0], seeds, P, Qt)
    c = r["converged"] == 1
    print("far, %s: kernel converged %d, fp64 restatement %d of %d" % ("pose" if pose else "position", c.sum(), conv64.sum(), B))
    assert conv64.sum() >= 240
    assert c.sum() >= conv64.sum() - 3
    assert_on_target(MODEL, "EE", [0, 0, 0], r, P, Qt, which=c, label="far, converged envs")
    assert (r["iters"][~c] == ib.DEFAULTS["max_iters"]).all()
    assert set(np.unique(r["converged"])) <= {0, 1}


@pytest.mark.parametrize("point", [[0, 0, 0], POINT])
def test_converged_envs_are_inside_the_tolerance_for_the_query_kernel(default_model, point):
    """Sharp, no margin: the two kernels compose the frame with the same float sequence, so for every converged env the query kernel's
    frame point at qpos_out has every component of target - point below tol_pos in fp32."""
    M, tab, seeds = default_model
    P, Qt, _ = ib.targets(MODEL, "EE", point, seeds, 1.0)
    f = tab.jaco_frame("EE", point=point)
    r = ib.ik(MODEL, f, seeds, P, Qt)
    q = qb.query(MODEL, r["qpos"], np.zeros((B, 21), np.float32), [f], want=("xpos", "xmat"))
    xp, R, pt = q["xpos"][:, 0], q["xmat"][:, 0], np.array(f.point[:], np.float32)
    # run_query: P = p + mul(R, point), mul's rows summed left to right, all fp32
    off = np.stack([(R[:, 3 * i] * pt[0] + R[:, 3 * i + 1] * pt[1]) + R[:, 3 * i + 2] * pt[2] for i in range(3)], 1).astype(np.float32)
    d = np.abs(P - (xp + off).astype(np.float32))
    c = r["converged"] == 1
    assert c.sum() >= 240
    assert d.dtype == np.float32 and (d[c] < np.float32(TOL_POS)).all(), d[c].max()


def test_seed_on_target_takes_no_iteration(default_model):
    M, tab, seeds = default_model
    f = tab.jaco_frame("EE", point=POINT)
    P, Qt, _ = ib.targets(MODEL, "EE", POINT, seeds, 0.0)
    r = ib.ik(MODEL, f, seeds, P, Qt)
    assert (r["iters"] == 0).all() and (r["converged"] == 1).all()
    assert (bits(r["qpos"]) == bits(seeds)).all()


def test_untouched_words_are_copied_bit_for_bit(default_model):
    """Fingers and free-joint coordinates (odd bit patterns included); a dof_mask that removes joint 0 leaves joint 0's word alone."""
    M, tab, seeds = default_model
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.3)
    s = seeds.copy()
    s[:, 12:16] = np.random.default_rng(0).normal(size=(B, 4)).astype(np.float32)   # not even unit quaternions: not IK's business
    s[0, 9], s[1, 10], s[2, 7] = np.float32(1e-42), -0.0, np.float32(3e-39)         # denormals and a negative zero
    f = tab.jaco_frame("EE", point=[0, 0, 0])
    r = ib.ik(MODEL, f, s, P, Qt)
    assert (r["converged"] == 1).all()
    assert (bits(r["qpos"])[:, 6:] == bits(s)[:, 6:]).all()
    assert (bits(r["qpos"])[:, :6] != bits(s)[:, :6]).any(axis=0).all()
    r = ib.ik(MODEL, f, s, P, None, dof_mask=0b111110)
    assert (bits(r["qpos"])[:, 0] == bits(s)[:, 0]).all() and (bits(r["qpos"])[:, 6:] == bits(s)[:, 6:]).all()
    assert (bits(r["qpos"])[:, 1:6] != bits(s)[:, 1:6]).any(axis=0).all()
    assert (r["converged"] == 1).sum() >= 240   # (five joints for three coordinates: still solvable)


@pytest.mark.parametrize("ee", ["EE_1", "EE_2"])
def test_the_other_arm_is_untouched_on_the_two_arm_model(ee):
    model = "jaco2_dual_torque"
    tab, seeds = ib.table_of(model), ib.picking_seeds(model, 64)
    P, Qt, _ = ib.targets(model, ee, [0, 0, 0], seeds, 0.3)
    r = ib.ik(model, tab.jaco_frame(ee, point=[0, 0, 0]), seeds, P, Qt)
    mine = np.zeros(seeds.shape[1], bool)
    mine[tab.chain(ee)[0]] = True
    assert mine.sum() == 6 and (r["converged"] == 1).all()
    assert (bits(r["qpos"])[:, ~mine] == bits(seeds)[:, ~mine]).all()
    assert (bits(r["qpos"])[:, mine] != bits(seeds)[:, mine]).any(axis=0).all()


@pytest.mark.parametrize("case", ["out_of_reach", "beyond_joint_1"])
def test_joint_limits_hold_and_the_residual_is_honest(default_model, case):
    """Out of reach (2 m away): not converged.  Both cases: limited joints inside the model's range exactly, and the reported residual is
    the oracle's residual at the returned qpos within the margins of the near-target test."""
    M, tab, seeds = default_model
    if case == "out_of_reach":
        P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.0)
        P = (P + np.float32([2, 0, 0])).astype(np.float32)
    else:   # the pose of a configuration with joint 1 at 0.3 rad, 0.57 rad below its range
        g = seeds.copy()
        g[:, 1] = 0.3
        P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], g, 0.0, clamp=False)
    r = ib.ik(MODEL, tab.jaco_frame("EE", point=[0, 0, 0]), seeds, P, Qt)
    if case == "out_of_reach":
        assert (r["converged"] == 0).all() and (r["iters"] == ib.DEFAULTS["max_iters"]).all()
    rng = M["f_range"].reshape(-1, 2).astype(np.float32)
    for b in np.nonzero(M["f_limited"])[0]:
        a = int(M["f_qposadr"][b])
        assert (r["qpos"][:, a] >= rng[b, 0]).all() and (r["qpos"][:, a] <= rng[b, 1]).all(), (b, r["qpos"][:, a].min(), r["qpos"][:, a].max())
    ep, er = ib.oracle_errors(MODEL, "EE", [0, 0, 0], r["qpos"], P, Qt)
    print("%s: converged %d; residual vs oracle: position %.3g, rotation %.3g" % (case, (r["converged"] == 1).sum(), np.abs(ep - r["resid"][:, 0]).max(),
                                                                               np.abs(er - r["resid"][:, 1]).max()))
    assert np.abs(ep - r["resid"][:, 0]).max() < POS_MARGIN
    assert np.abs(er - r["resid"][:, 1]).max() < ROT_MARGIN


def test_permuted_envs_give_permuted_results(default_model):
    M, tab, seeds = default_model
    P, Qt, _ = ib.targets(MODEL, "EE", POINT, seeds, 1.0)
    f = tab.jaco_frame("EE", point=POINT)
    a = ib.ik(MODEL, f, seeds, P, Qt)
    perm = np.random.default_rng(5).permutation(B)
    b = ib.ik(MODEL, f, seeds[perm], P[perm], Qt[perm])
    for k in ("qpos", "resid"):
        assert (bits(b[k]) == bits(a[k][perm])).all(), k
    assert (b["iters"] == a["iters"][perm]).all() and (b["converged"] == a["converged"][perm]).all()


@pytest.mark.parametrize("model,ee", [("jaco2_reaching_torque", "EE"), ("jaco2_torque", "EE"), ("jaco2_dual_torque", "EE_1"), ("jaco2_dual_torque", "EE_2")])
@pytest.mark.parametrize("pose", [True, False])
def test_other_layouts(model, ee, pose):
    """The arm-only model, the _d12 and the _d30 builds: near targets, the assertions of the default model."""
    tab, seeds = ib.table_of(model), ib.picking_seeds(model, B)
    P, Qt, _ = ib.targets(model, ee, [0, 0, 0], seeds, 0.3)
    Qt = Qt if pose else None
    r = ib.ik(model, tab.jaco_frame(ee, point=[0, 0, 0]), seeds, P, Qt)
    assert (r["converged"] == 1).all(), int((r["converged"] == 1).sum())
    assert_on_target(model, ee, [0, 0, 0], r, P, Qt, label="%s %s, %s" % (model, ee, "pose" if pose else "position"))


def test_argument_checks(default_model):
    M, tab, seeds = default_model
    s = seeds[:4]
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], s, 0.1)
    f = tab.jaco_frame("EE", point=[0, 0, 0])
    bad = tab.jaco_frame("EE", point=[0, 0, 0]); bad.body = 99
    with pytest.raises(ValueError, match="body"):
        ib.ik(MODEL, bad, s, P, Qt)
    with pytest.raises(ValueError, match="max_iters"):
        ib.ik(MODEL, f, s, P, Qt, max_iters=_lib.JACO_IK_MAX_ITERS + 1)
    world = tab.jaco_frame("EE", point=[0, 0, 0]); world.body = -1
    with pytest.raises(ValueError, match="empty active"):
        ib.ik(MODEL, world, s, P, Qt)
    with pytest.raises(ValueError, match="empty active"):   # a free body's chain has no hinge dof
        ib.ik(MODEL, tab.jaco_frame("object_body"), s, P, Qt)
    with pytest.raises(ValueError, match="empty active"):
        ib.ik(MODEL, f, s, P, Qt, dof_mask=1 << 7)
    with pytest.raises(ValueError, match="required"):
        ib.ik(MODEL, f, s, None, Qt)
    with pytest.raises(ValueError, match="positive"):
        ib.ik(MODEL, f, s, P, Qt, damping=0.0)
    full = ib.ik(MODEL, f, s, P, Qt, max_iters=_lib.JACO_IK_MAX_ITERS)
    lean = ib.ik(MODEL, f, s, P, Qt, resid=False, status=False)
    dflt = ib.ik(MODEL, f, s, P, Qt, defaults=True)
    assert (bits(lean["qpos"]) == bits(full["qpos"])).all() and (bits(dflt["qpos"]) == bits(full["qpos"])).all()
    assert (full["converged"] == 1).all() and "resid" not in lean and "iters" not in lean


def test_robot_config_ik_lands_tx_on_the_target(default_model):
    """BatchedMujocoConfig.ik on the emulator-backed sim: Tx(name, q=result, x=x) is on pos; the sim's state is not touched."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    M, tab, seeds = default_model
    n = 32
    sim = EmuSim(MODEL, seeds[:n], np.zeros((n, 21), np.float32))
    cfg = BatchedMujocoConfig(sim)
    P, Qt, G = ib.targets(MODEL, "EE", POINT, seeds[:n], 0.3)
    before = sim.qpos.clone()
    q, ok = cfg.ik("EE", torch.from_numpy(P), x=POINT)
    assert q.shape == (n, 6) and ok.dtype == torch.bool and ok.all()
    assert ((cfg.Tx("EE", q=q, x=POINT) - torch.from_numpy(P)).norm(dim=1) < TOL_POS + POS_MARGIN).all()
    P0, Qt0, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds[:n], 0.3)
    q2, ok2 = cfg.ik("EE", P0, quat=Qt0, q=seeds[:n, :6] + 0.05)   # body origin, pose target, explicit seed
    assert ok2.all()
    assert ((cfg.Tx("EE", q=q2) - torch.from_numpy(P0)).norm(dim=1) < TOL_POS + POS_MARGIN).all()
    assert torch.equal(sim.qpos, before) and sim.state_version == 0
    with pytest.raises(TypeError, match="unknown IK option"):
        cfg.ik("EE", P, lam=0.1)
