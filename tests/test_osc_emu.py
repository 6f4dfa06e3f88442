"""CPU tier: the operational-space controller kernel (mujoco_jaco_amd/csrc/osc.h, jaco_osc) under the wavefront emulator against
oracle/glue.py osc_generate in fp64 on the fp64 oracle's J, M[active, active], qfrc_bias[active], point and quaternion
(tests/osc_binding.py).

Error measure: max over the active dofs of |u - u_ref| / (1 + |u_ref|).  Bounds = 3 x the largest value measured on the emulator:
  regular branch, default model, B = 67 (all 67 envs have fp64 |det| >= 0.24: none on the knife edge) ........ 8.72e-6 -> 2.7e-5
  pseudo-inverse branch, the 8 elbow-scan configurations (fp64 |det| < 2.4e-7) ................................ 2.76e-6 -> 8.3e-6
  ... with dof_mask leaving dofs 0-3 (rank-4 matrix) ......................................................... 6.68e-6 -> 2.0e-5
  non-default gains (kp 30, ko 90, kv 12, vmax 0.2 / 0.6), targets inside / beyond both saturations ............ 4.16e-6 -> 1.3e-5
  the other layouts (B = 1 and 5; reaching, jaco2_torque, curtain_torque_sensor, both arms of dual_torque) ..... 7.14e-6: inside the
  regular bound, which they share.
Closed loop (jaco2_reaching_torque, B = 8, 200 x {osc -> one substep}): the fp64 reference's pose error |[e_p (m); e_r (rad)]| falls to
0.48 .. 0.57 of its start; the emulated loop's final EE position is at most 1.14e-6 m from the reference's -> bound 3.5e-6 m.
The emulator's stage dump (JDBG_*) does not hold the env step's arm torques, so there is no bit comparison with stage_osc_general.
"""
import numpy as np
import pytest

import ik_binding as ib
import osc_binding as ob
from emu_sim import EmuSim

MODEL = "jaco2_curtain_torque"
B = 67
REG_BOUND = 2.7e-5       # 3 x 8.72e-6 (emulator)
PINV_BOUND = 8.3e-6      # 3 x 2.76e-6
PINV4_BOUND = 2.0e-5     # 3 x 6.68e-6
OPT_BOUND = 1.3e-5       # 3 x 4.16e-6
LOOP_BOUND = 3.5e-6      # m; 3 x 1.14e-6
GAINS = dict(kp=30.0, ko=90.0, kv=12.0, vmax_xyz=0.2, vmax_abg=0.6)
REFUSALS = {
    "nframes0": "jaco_osc: nframes 0 outside [1, 2]",
    "nframes3": "jaco_osc: nframes 3 outside [1, 2]",
    "body_low": "jaco_osc: frame 0: body -1 outside [0, 11)",
    "body_high": "jaco_osc: frame 0: body 11 outside [0, 11)",
    "empty": "jaco_osc: frame 0: empty active dof set (a free body's frame, or a dof_mask that removes the whole chain)",
    "seven": "jaco_osc: frame 0: 7 active dofs, at most 6 (narrow the chain with dof_mask)",
    "overlap": "jaco_osc: frame 1: its active dofs overlap those of an earlier frame",
    "no_motor": "jaco_osc: frame 0: active dof 6 has no motor actuator",
    "gain": "jaco_osc: kp, ko, kv, vmax_xyz and vmax_abg must be positive",
    "null": "jaco_osc: the target positions, the target quaternions and the output ctrl are required",
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame_of(model, name):
    return ib.table_of(model).jaco_frame(name)


def motors(model, dofs):
    m = ob.motor_of(model)
    return [m[d] for d in dofs]


@pytest.fixture(scope="module")
def regular():
    """Test 1's inputs, the fp64 reference and the emulator's answer, computed once."""
    q, v = ob.states(MODEL, B)
    T6 = ob.targets6(MODEL, "EE", q)
    U, D, acts = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :])
    tp, tq = ob.kernel_targets(T6[:, None, :])
    r = ob.osc(MODEL, [frame_of(MODEL, "EE")], q, v, tp, tq)
    return dict(q=q, v=v, T6=T6, U=U[:, 0], D=D[:, 0], act=acts[0], tp=tp, tq=tq, r=r)


@pytest.fixture(scope="module")
def singular():
    q, v = ob.singular_states(MODEL, "EE", want=8)
    T6 = ob.targets6(MODEL, "EE", q)
    tp, tq = ob.kernel_targets(T6[:, None, :])
    return dict(q=q, v=v, T6=T6, tp=tp, tq=tq)


def test_regular_branch_matches_the_fp64_reference(regular):
    g = regular
    knife = (g["D"] > 2.5e-4) & (g["D"] < 4e-3)
    reg = g["D"] >= 4e-3
    assert knife.mean() <= 0.2, knife.sum()
    err = ob.error(g["r"]["ctrl"][:, motors(MODEL, g["act"])], g["U"])
    print("regular branch: %d of %d envs compared (%d on the knife edge), fp64 |det| min %.3g, error max %.3g" % (reg.sum(), B, knife.sum(), g["D"].min(), err[reg].max()))
    assert reg.sum() >= 0.8 * B
    assert (g["r"]["status"][reg, 0] == 0).all()
    assert err[reg].max() <= REG_BOUND, err[reg].max()
    assert (bits(g["r"]["ctrl"][:, 6:]) == 0).all()   # NULL ctrl_in: the words outside the active motors are zeros


def test_pseudo_inverse_branch_matches_the_fp64_reference(singular):
    g = singular
    U, D, acts = ob.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"][:, None, :])
    assert len(D) >= 8 and (D[:, 0] < 2.5e-4).all(), D[:, 0]
    r = ob.osc(MODEL, [frame_of(MODEL, "EE")], g["q"], g["v"], g["tp"], g["tq"])
    err = ob.error(r["ctrl"][:, motors(MODEL, acts[0])], U[:, 0])
    print("pseudo-inverse branch: fp64 |det| max %.3g, error max %.3g" % (D.max(), err.max()))
    assert (r["status"][:, 0] == 1).all()
    assert err.max() <= PINV_BOUND, err.max()


def test_four_active_dofs_take_the_pseudo_inverse_branch_and_leave_the_other_actuators_alone(singular, regular):
    for g, label in ((singular, "near-singular"), (regular, "regular")):
        mask = 0b001111
        U, D, acts = ob.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"][:, None, :], dof_mask=mask)
        assert acts[0] == [0, 1, 2, 3]
        cin = np.random.default_rng(4).normal(size=(len(g["q"]), 9)).astype(np.float32)
        r = ob.osc(MODEL, [frame_of(MODEL, "EE")], g["q"], g["v"], g["tp"], g["tq"], cin, dof_mask=mask)
        err = ob.error(r["ctrl"][:, :4], U[:, 0, :4])
        print("dof_mask 0b1111, %s states: error max %.3g" % (label, err.max()))
        assert (r["status"][:, 0] == 1).all()
        assert (bits(r["ctrl"][:, 4:]) == bits(cin[:, 4:])).all()
        assert err.max() <= PINV4_BOUND, err.max()


def test_options_and_both_saturations(regular):
    g = regular
    n = 16
    q, v = g["q"][:n], g["v"][:n]
    sat_xyz, sat_abg = GAINS["vmax_xyz"] / GAINS["kp"] * GAINS["kv"], GAINS["vmax_abg"] / GAINS["ko"] * GAINS["kv"]
    worst = 0.0
    for label, dist, ang in (("inside", (0.01, 0.03), (0.02, 0.06)), ("beyond", (0.25, 0.35), (0.8, 1.2))):
        T6 = ob.offset_targets(MODEL, "EE", q, dist, ang, seed=31)
        ep, er = ob.pose_error(MODEL, "EE", q, T6)
        nx, na = ep, np.sin(er / 2)   # |u_task| of the two halves: |p - p*| and |vec(q* conj(q))| = sin(angle / 2)
        assert ((nx < sat_xyz) & (na < sat_abg)).all() if label == "inside" else ((nx > sat_xyz) & (na > sat_abg)).all(), (nx, na)
        U, D, acts = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :], **GAINS)
        Udef = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :])[0]
        assert np.abs(U - Udef).max() > 1.0   # (the gains matter: the default ones give another answer)
        tp, tq = ob.kernel_targets(T6[:, None, :])
        r = ob.osc(MODEL, [frame_of(MODEL, "EE")], q, v, tp, tq, **GAINS)
        err = ob.error(r["ctrl"][:, :6], U[:, 0])
        print("gains %s, targets %s both saturations: error max %.3g" % (GAINS, label, err.max()))
        assert (r["status"][:, 0] == 0).all()
        worst = max(worst, err.max())
    assert worst <= OPT_BOUND, worst
    # a NULL options pointer = the defaults
    a = ob.osc(MODEL, [frame_of(MODEL, "EE")], q, v, g["tp"][:n], g["tq"][:n], defaults=True)["ctrl"]
    assert (bits(a) == bits(g["r"]["ctrl"][:n])).all()


@pytest.mark.parametrize("nenv", [1, 5])
@pytest.mark.parametrize("model", ["jaco2_reaching_torque", "jaco2_torque", "jaco2_curtain_torque_sensor"])
def test_other_layouts(model, nenv):
    q, v = ob.states(model, nenv)
    T6 = ob.targets6(model, "EE", q)
    U, D, acts = ob.reference(model, ["EE"], q, v, T6[:, None, :])
    assert (D >= 4e-3).all()
    tp, tq = ob.kernel_targets(T6[:, None, :])
    r = ob.osc(model, [frame_of(model, "EE")], q, v, tp, tq)
    err = ob.error(r["ctrl"][:, motors(model, acts[0])], U[:, 0])
    print("%s, B = %d: error max %.3g" % (model, nenv, err.max()))
    assert (r["status"] == 0).all() and err.max() <= REG_BOUND, err.max()
    other = [a for a in range(r["ctrl"].shape[1]) if a not in motors(model, acts[0])]
    assert (bits(r["ctrl"][:, other]) == 0).all()


@pytest.mark.parametrize("nenv", [1, 5])
def test_two_arms_in_one_call_equal_the_two_single_calls(nenv):
    model, names = "jaco2_dual_torque", ["EE_1", "EE_2"]
    q, v = ob.states(model, nenv)
    T6 = np.stack([ob.targets6(model, n, q) for n in names], 1)
    U, D, acts = ob.reference(model, names, q, v, T6)
    assert (D >= 4e-3).all() and not set(acts[0]) & set(acts[1])
    tp, tq = ob.kernel_targets(T6)
    fr = [frame_of(model, n) for n in names]
    cin = np.random.default_rng(6).normal(size=(nenv, 18)).astype(np.float32)
    both = ob.osc(model, fr, q, v, tp, tq, cin)
    for f in range(2):
        err = ob.error(both["ctrl"][:, motors(model, acts[f])], U[:, f])
        print("%s, B = %d, %s: error max %.3g" % (model, nenv, names[f], err.max()))
        assert err.max() <= REG_BOUND, err.max()
    assert (both["status"] == 0).all()
    one = [ob.osc(model, fr[f:f + 1], q, v, tp[:, f:f + 1], tq[:, f:f + 1], cin) for f in range(2)]
    for f in range(2):   # each arm's words are untouched by the other's call, and its own equal the joint call's
        mine, others = motors(model, acts[f]), [a for a in range(18) if a not in motors(model, acts[f])]
        assert (bits(one[f]["ctrl"][:, others]) == bits(cin[:, others])).all()
        assert (bits(one[f]["ctrl"][:, mine]) == bits(both["ctrl"][:, mine])).all()
    chained = ob.osc(model, fr[1:], q, v, tp[:, 1:], tq[:, 1:], one[0]["ctrl"])
    assert (bits(chained["ctrl"]) == bits(both["ctrl"])).all()
    swapped = ob.osc(model, fr[::-1], q, v, tp[:, ::-1], tq[:, ::-1], cin)
    assert (bits(swapped["ctrl"]) == bits(both["ctrl"])).all()


def test_pass_through_aliasing_and_null_ctrl_in(regular):
    g = regular
    fr = [frame_of(MODEL, "EE")]
    cin = np.zeros((B, 9), np.float32)
    w = bits(cin)
    w[:, 6] = 0x7fc12345      # a NaN with a payload
    w[:, 7] = 0x80000000      # -0
    w[:, 8] = 0x00000123      # a denormal
    w[:, :6] = 0xffc00001     # (the active words are overwritten whatever they held)
    r = ob.osc(MODEL, fr, g["q"], g["v"], g["tp"], g["tq"], cin)
    assert (bits(r["ctrl"][:, 6:]) == w[:, 6:]).all()
    assert (bits(r["ctrl"][:, :6]) == bits(g["r"]["ctrl"][:, :6])).all()
    a = ob.osc(MODEL, fr, g["q"], g["v"], g["tp"], g["tq"], cin, alias=True)
    assert (bits(a["ctrl"]) == bits(r["ctrl"])).all()
    masked = ob.osc(MODEL, fr, g["q"], g["v"], g["tp"], g["tq"], cin, dof_mask=0b110)
    assert (bits(masked["ctrl"][:, [0, 3, 4, 5, 6, 7, 8]]) == w[:, [0, 3, 4, 5, 6, 7, 8]]).all()
    n = ob.osc(MODEL, fr, g["q"], g["v"], g["tp"], g["tq"], None, status=False)
    assert n["status"] is None and (bits(n["ctrl"]) == bits(g["r"]["ctrl"])).all()


def refused(case):
    """Calls the emulated entry with the arguments of one refusal case; returns the message."""
    q, v = ob.states(MODEL, 2)
    frames, tp, tq, no_out, opts = ob.refusal_args(case)
    with pytest.raises(ValueError) as e:
        ob.osc(MODEL, frames, q, v, tp, tq, no_out=no_out, **opts)
    return str(e.value)


@pytest.mark.parametrize("case", ob.REFUSAL_CASES)
def test_refusals(case):
    assert refused(case) == "emu_osc returned -1: " + REFUSALS[case.split("_")[0] if case.startswith("null") else case]


def test_every_gain_and_every_null_pointer_is_checked():
    q, v = ob.states(MODEL, 1)
    tp, tq = np.zeros((1, 1, 3), np.float32), np.float32([[[1, 0, 0, 0]]])
    ee = [frame_of(MODEL, "EE")]
    for k in ("kp", "ko", "kv", "vmax_xyz", "vmax_abg"):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="must be positive"):
                ob.osc(MODEL, ee, q, v, tp, tq, **{k: bad})
    for kw in (dict(target_pos=None, target_quat=tq), dict(target_pos=tp, target_quat=None), dict(target_pos=tp, target_quat=tq, no_out=True)):
        with pytest.raises(ValueError, match="are required"):
            ob.osc(MODEL, ee, q, v, **kw)
    with pytest.raises(ValueError, match=r"outside \[1, 2\]"):
        ob.osc(MODEL, None, q, v, tp, tq)


def test_closed_loop_follows_the_fp64_reference():
    q0, T6 = ob.loop_inputs()
    ep0, er0 = ob.pose_error(ob.LOOP_MODEL, "EE", q0, T6)
    assert ((ep0 >= 0.05) & (ep0 <= 0.10) & (er0 <= 0.3)).all()
    qo = ob.closed_loop_oracle(q0, T6)
    ep1, er1 = ob.pose_error(ob.LOOP_MODEL, "EE", qo, T6)
    ratio = np.hypot(ep1, er1) / np.hypot(ep0, er0)
    assert (ratio < 0.7).all(), ratio   # the reference itself approaches its targets
    qe = ob.closed_loop_emu(q0, T6)
    com = ib.table_of(ob.LOOP_MODEL).com("EE")
    d = np.linalg.norm(ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qe)[0] - ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qo)[0], axis=1)
    print("closed loop: reference pose error ratio %.3g .. %.3g, EE distance emulator - reference max %.3g m" % (ratio.min(), ratio.max(), d.max()))
    assert d.max() <= LOOP_BOUND, d


def test_batched_osc_mirrors_abr_control_on_the_emulator(regular):
    """robot_config.BatchedOSC over the emulator: generate() = jaco_osc at the Euler targets' quaternions, state and ctrl passed through."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, BatchedOSC, quat_from_euler_rxyz
    g = regular
    sim = EmuSim(MODEL, g["q"], g["v"])
    ctl = BatchedMujocoConfig(sim).osc()
    assert isinstance(ctl, BatchedOSC) and ctl.names == ("EE",)
    qt = quat_from_euler_rxyz(torch.tensor(g["T6"][:, 3:], dtype=torch.float64)).numpy()
    ref = np.array([ob.glue.quat_from_euler(*t[3:]) for t in g["T6"]])
    assert np.abs(qt - ref).max() < 1e-15
    frame0 = [ib.table_of(MODEL).jaco_frame("EE", point=np.zeros(3))]
    u = ctl.generate(torch.tensor(g["T6"], dtype=torch.float32))
    qt32 = quat_from_euler_rxyz(torch.tensor(g["T6"][:, 3:], dtype=torch.float32)).numpy()
    direct = ob.osc(MODEL, frame0, g["q"], g["v"], g["tp"], qt32[:, None, :])["ctrl"]
    assert (bits(u.numpy()) == bits(direct)).all()
    err = ob.error(u.numpy()[:, :6], g["U"])
    assert err.max() <= REG_BOUND, err.max()   # (fp32 Euler -> quaternion in torch instead of fp64 in glue: inside the same bound)
    # q / dq / ctrl: spliced into the sim's state / passed through
    q2, v2 = ob.states(MODEL, B, seed=9, vseed=10)
    cin = np.random.default_rng(1).normal(size=(B, 9)).astype(np.float32)
    u2 = ctl.generate_pose(g["tp"][:, 0], g["tq"][:, 0], q=q2[:, :6], dq=v2[:, :6], ctrl=cin)
    qs, vs = g["q"].copy(), g["v"].copy()
    qs[:, :6], vs[:, :6] = q2[:, :6], v2[:, :6]
    d2 = ob.osc(MODEL, frame0, qs, vs, g["tp"], g["tq"], cin)["ctrl"]
    assert (bits(u2.numpy()) == bits(d2)).all() and (bits(u2.numpy()[:, 6:]) == bits(cin[:, 6:])).all()
    other = BatchedOSC(BatchedMujocoConfig(sim), kp=30, ko=90, kv=12, vmax=(0.2, 0.6)).generate(torch.tensor(g["T6"], dtype=torch.float32))
    d3 = ob.osc(MODEL, frame0, g["q"], g["v"], g["tp"], qt32[:, None, :], **GAINS)["ctrl"]
    assert (bits(other.numpy()) == bits(d3)).all()


def test_batched_osc_drives_both_arms_in_one_launch():
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    model, names = "jaco2_dual_torque", ("EE_1", "EE_2")
    q, v = ob.states(model, 3)
    sim = EmuSim(model, q, v)
    calls = []
    inner = sim.osc
    sim.osc = lambda *a, **k: (calls.append(len(a[0])), inner(*a, **k))[1]
    T6 = np.stack([ob.targets6(model, n, q) for n in names], 1)
    u = BatchedMujocoConfig(sim, ee="EE_1").osc(names).generate(torch.tensor(T6, dtype=torch.float32))
    assert calls == [2] and u.shape == (3, 18)
    U, D, acts = ob.reference(model, list(names), q, v, T6)
    for f in range(2):
        assert ob.error(u.numpy()[:, motors(model, acts[f])], U[:, f]).max() <= REG_BOUND
    with pytest.raises(ValueError, match="1 to 2 frames"):
        BatchedMujocoConfig(sim, ee="EE_1").osc(("EE_1", "EE_2", "link3_1"))
