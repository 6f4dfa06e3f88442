"""GPU tier: jaco_osc (mujoco_jaco_amd/csrc/osc.h) on the MI355X against oracle/glue.py osc_generate in fp64 on the fp64 oracle's
quantities, against the emulator, and against itself (tests/osc_binding.py holds inputs and references; tests/test_osc_emu.py is the
CPU-tier twin).

Error measure: max over the active dofs of |u - u_ref| / (1 + |u_ref|).  Bounds = 3 x the largest value measured on the MI355X:
  regular branch, default model, B = 67 ........................................ 1.06e-5 -> 3.2e-5
  pseudo-inverse branch, the 8 elbow-scan configurations ....................... 1.96e-6 -> 5.9e-6
  ... with dof_mask leaving dofs 0-3 ........................................... 7.97e-6 -> 2.4e-5
  non-default gains, targets inside / beyond both saturations .................. 4.77e-6 -> 1.4e-5
  GPU against the emulator on the regular set .................................. 4.21e-6 -> 1.3e-5
  closed loop, final EE position against the fp64 reference's .................. 3.34e-7 m -> 1.0e-6 m
The other layouts share the regular bound (largest measured: 6.64e-6).
"""
import ctypes

import numpy as np
import pytest
import torch

import ik_binding as ib
import osc_binding as ob
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError

pytestmark = pytest.mark.gpu
MODEL = "jaco2_curtain_torque"
B = 67
REG_BOUND = 3.2e-5       # 3 x 1.06e-5 (MI355X)
PINV_BOUND = 5.9e-6      # 3 x 1.96e-6
PINV4_BOUND = 2.4e-5     # 3 x 7.97e-6
OPT_BOUND = 1.4e-5       # 3 x 4.77e-6
EMU_BOUND = 1.3e-5       # 3 x 4.21e-6
LOOP_BOUND = 1.0e-6      # m; 3 x 3.34e-7
GAINS = dict(kp=30.0, ko=90.0, kv=12.0, vmax_xyz=0.2, vmax_abg=0.6)


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t, np.float32)).view(np.uint32)


def motors(model, dofs):
    m = ob.motor_of(model)
    return [m[d] for d in dofs]


def gpu_osc(sim, frames, q, v, tp, tq, ctrl=None, **options):
    r = sim.osc(frames, _dev(tp), _dev(tq), None if q is None else _dev(q), None if v is None else _dev(v), None if ctrl is None else _dev(ctrl), **options)
    return r["ctrl"].cpu().numpy(), r["singular"].cpu().numpy()


@pytest.fixture(scope="module")
def regular():
    q, v = ob.states(MODEL, B)
    T6 = ob.targets6(MODEL, "EE", q)
    U, D, acts = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :])
    tp, tq = ob.kernel_targets(T6[:, None, :])
    sim = BatchedMujoco(B, robot_file=MODEL)
    fr = [sim.frames.jaco_frame("EE")]
    u, sing = gpu_osc(sim, fr, q, v, tp, tq)
    yield dict(q=q, v=v, T6=T6, U=U[:, 0], D=D[:, 0], act=acts[0], tp=tp, tq=tq, u=u, sing=sing, sim=sim, fr=fr)
    sim.close()


def test_regular_branch_matches_the_fp64_reference(regular):
    g = regular
    knife = (g["D"] > 2.5e-4) & (g["D"] < 4e-3)
    reg = g["D"] >= 4e-3
    assert knife.mean() <= 0.2
    err = ob.error(g["u"][:, :6], g["U"])
    print("MEASURE regular: error max %.3g over %d envs" % (err[reg].max(), reg.sum()))
    assert not g["sing"][reg].any()
    assert err[reg].max() <= REG_BOUND, err[reg].max()
    assert (bits(g["u"][:, 6:]) == 0).all()


def test_gpu_agrees_with_the_emulator_and_with_itself(regular):
    g = regular
    emu = ob.osc(MODEL, g["fr"], g["q"], g["v"], g["tp"], g["tq"])
    err = ob.error(g["u"][:, :6], emu["ctrl"][:, :6])
    print("MEASURE gpu - emulator: error max %.3g" % err.max())
    assert err.max() <= EMU_BOUND, err.max()
    assert (emu["status"][:, 0] == g["sing"][:, 0]).all()
    again, sing = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], g["tq"])
    assert (bits(again) == bits(g["u"])).all() and (sing == g["sing"]).all()


def test_pseudo_inverse_branch_and_four_active_dofs():
    q, v = ob.singular_states(MODEL, "EE", want=8)
    T6 = ob.targets6(MODEL, "EE", q)
    tp, tq = ob.kernel_targets(T6[:, None, :])
    U, D, acts = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :])
    assert (D < 2.5e-4).all()
    sim = BatchedMujoco(len(q), robot_file=MODEL)
    fr = [sim.frames.jaco_frame("EE")]
    u, sing = gpu_osc(sim, fr, q, v, tp, tq)
    err = ob.error(u[:, :6], U[:, 0])
    print("MEASURE pinv: error max %.3g" % err.max())
    assert sing.all()
    assert err.max() <= PINV_BOUND, err.max()
    U4 = ob.reference(MODEL, ["EE"], q, v, T6[:, None, :], dof_mask=0b1111)[0]
    cin = np.random.default_rng(4).normal(size=(len(q), 9)).astype(np.float32)
    u4, sing4 = gpu_osc(sim, fr, q, v, tp, tq, cin, dof_mask=0b1111)
    err4 = ob.error(u4[:, :4], U4[:, 0, :4])
    print("MEASURE pinv4: error max %.3g" % err4.max())
    assert sing4.all() and (bits(u4[:, 4:]) == bits(cin[:, 4:])).all()
    assert err4.max() <= PINV4_BOUND, err4.max()
    sim.close()


def test_options_and_both_saturations(regular):
    g = regular
    sat_xyz, sat_abg = GAINS["vmax_xyz"] / GAINS["kp"] * GAINS["kv"], GAINS["vmax_abg"] / GAINS["ko"] * GAINS["kv"]
    worst = 0.0
    for label, dist, ang in (("inside", (0.01, 0.03), (0.02, 0.06)), ("beyond", (0.25, 0.35), (0.8, 1.2))):
        T6 = ob.offset_targets(MODEL, "EE", g["q"], dist, ang, seed=31)
        ep, er = ob.pose_error(MODEL, "EE", g["q"], T6)
        nx, na = ep, np.sin(er / 2)
        assert ((nx < sat_xyz) & (na < sat_abg)).all() if label == "inside" else ((nx > sat_xyz) & (na > sat_abg)).all()
        U = ob.reference(MODEL, ["EE"], g["q"], g["v"], T6[:, None, :], **GAINS)[0]
        tp, tq = ob.kernel_targets(T6[:, None, :])
        u, sing = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], tp, tq, **GAINS)
        assert not sing.any()
        worst = max(worst, ob.error(u[:, :6], U[:, 0]).max())
    print("MEASURE options: error max %.3g" % worst)
    assert worst <= OPT_BOUND, worst


@pytest.mark.parametrize("nenv", [1, 5])
@pytest.mark.parametrize("model", ["jaco2_reaching_torque", "jaco2_torque", "jaco2_curtain_torque_sensor"])
def test_other_layouts(model, nenv):
    q, v = ob.states(model, nenv)
    T6 = ob.targets6(model, "EE", q)
    U, D, acts = ob.reference(model, ["EE"], q, v, T6[:, None, :])
    tp, tq = ob.kernel_targets(T6[:, None, :])
    sim = BatchedMujoco(nenv, robot_file=model)
    u, sing = gpu_osc(sim, [sim.frames.jaco_frame("EE")], q, v, tp, tq)
    err = ob.error(u[:, motors(model, acts[0])], U[:, 0])
    print("MEASURE layout %s B=%d: error max %.3g" % (model, nenv, err.max()))
    assert not sing.any() and err.max() <= REG_BOUND, err.max()
    sim.close()


@pytest.mark.parametrize("nenv", [1, 5])
def test_two_arms_in_one_call_equal_the_two_single_calls(nenv):
    model, names = "jaco2_dual_torque", ["EE_1", "EE_2"]
    q, v = ob.states(model, nenv)
    T6 = np.stack([ob.targets6(model, n, q) for n in names], 1)
    U, D, acts = ob.reference(model, names, q, v, T6)
    tp, tq = ob.kernel_targets(T6)
    sim = BatchedMujoco(nenv, robot_file=model)
    fr = [sim.frames.jaco_frame(n) for n in names]
    cin = np.random.default_rng(6).normal(size=(nenv, 18)).astype(np.float32)
    both, sing = gpu_osc(sim, fr, q, v, tp, tq, cin)
    assert not sing.any()
    for f in range(2):
        err = ob.error(both[:, motors(model, acts[f])], U[:, f])
        print("MEASURE layout %s B=%d %s: error max %.3g" % (model, nenv, names[f], err.max()))
        assert err.max() <= REG_BOUND, err.max()
    one = [gpu_osc(sim, fr[f:f + 1], q, v, tp[:, f:f + 1], tq[:, f:f + 1], cin)[0] for f in range(2)]
    for f in range(2):
        mine, others = motors(model, acts[f]), [a for a in range(18) if a not in motors(model, acts[f])]
        assert (bits(one[f][:, others]) == bits(cin[:, others])).all()
        assert (bits(one[f][:, mine]) == bits(both[:, mine])).all()
    chained = gpu_osc(sim, fr[1:], q, v, tp[:, 1:], tq[:, 1:], one[0])[0]
    assert (bits(chained) == bits(both)).all()
    # the Gym tier: env.robot_config.osc(("EE_1", "EE_2")) is the same single launch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    sim.set_state(_dev(q), _dev(v), None)
    ctl = BatchedMujocoConfig(sim, ee="EE_1").osc(names)
    T6_dev, cin_dev = _dev(T6), _dev(cin)
    sim.launch_count()   # (reading the counter resets it)
    u = ctl.generate(T6_dev, ctrl=cin_dev)
    assert sim.launch_count() == 1
    assert ob.error(u.cpu().numpy()[:, motors(model, acts[0]) + motors(model, acts[1])], np.concatenate([U[:, 0], U[:, 1]], 1)).max() <= REG_BOUND
    sim.close()


def test_pass_through_aliasing_null_inputs_and_an_untouched_handle(regular):
    g = regular
    sims = [BatchedMujoco(B, robot_file=MODEL) for _ in range(2)]
    ctrl = _dev(np.random.default_rng(8).uniform(-0.2, 0.2, (B, 9)))
    for s in sims:
        s.set_state(_dev(g["q"]), _dev(g["v"]), None)
        s.send_forces(ctrl, nsub=3)
    sim = sims[0]
    fr = [sim.frames.jaco_frame("EE")]
    cin = np.zeros((B, 9), np.float32)
    w = cin.view(np.uint32)
    w[:, 6], w[:, 7], w[:, 8], w[:, :6] = 0x7fc12345, 0x80000000, 0x00000123, 0xffc00001   # NaN payload, -0, a denormal; the active words are overwritten
    cin_dev = torch.from_numpy(w.view(np.int32).copy()).to("cuda:0").view(torch.float32)
    version = sim.state_version
    qh, vh, _ = sim.get_state()
    # NULL qpos / qvel = the handle's state; ctrl_in words outside the active motors come out bit-identical
    r = sim.osc(fr, _dev(g["tp"]), _dev(g["tq"]), ctrl=cin_dev)
    r2 = sim.osc(fr, _dev(g["tp"]), _dev(g["tq"]), qh, vh, cin_dev)
    assert (bits(r["ctrl"]) == bits(r2["ctrl"])).all()
    assert (bits(r["ctrl"])[:, 6:] == w[:, 6:]).all() and not np.isnan(r["ctrl"].cpu().numpy()[:, :6]).any()
    # ctrl_out aliasing ctrl_in (straight through the C ABI), and NULL ctrl_in / NULL status
    buf = cin_dev.clone()
    tp, tq = _dev(g["tp"]), _dev(g["tq"])
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    arr = (_lib.JacoFrame * 1)(*fr)
    rc = sim.L.jaco_osc(sim.h, ctypes.cast(arr, ctypes.c_void_p), 1, None, None, None, vp(tp), vp(tq), vp(buf), vp(buf), None, sim._stream())
    assert rc == 0 and (bits(buf) == bits(r["ctrl"])).all()
    out = torch.empty(B, 9, device="cuda:0")
    rc = sim.L.jaco_osc(sim.h, ctypes.cast(arr, ctypes.c_void_p), 1, None, None, None, vp(tp), vp(tq), None, vp(out), None, sim._stream())
    assert rc == 0 and (bits(out)[:, 6:] == 0).all() and (bits(out)[:, :6] == bits(r["ctrl"])[:, :6]).all()
    # the handle: state, flags, sensordata and a following step equal a twin's that never called jaco_osc
    assert sim.state_version == version
    snap = lambda s: [t.clone() for t in s.get_state()] + [s.flags().clone(), s.sensordata().clone()]
    for x, y in zip(snap(sims[0]), snap(sims[1])):
        assert torch.equal(x, y)
    for s in sims:
        s.send_forces(ctrl, nsub=5)
    for x, y in zip(snap(sims[0]), snap(sims[1])):
        assert torch.equal(x, y)
    for s in sims:
        s.close()


def test_env_tier_handle_is_left_alone_and_robot_config_reaches_the_controller():
    """env.robot_config.osc().generate() on an env-tier handle: every word of the env snapshots (state, task rows, flags, sensordata ...)
    is the same before and after."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    env = JacoBatchedEnv(num_envs=16, task="picking", seed=3)
    env.reset()
    before = env.sim.save_envs().clone()
    T = torch.zeros(16, 6, device="cuda:0")
    T[:, :3] = env.sim.get_xyz("EE") + 0.05
    u = env.robot_config.osc().generate(T)
    assert u.shape == (16, 9) and torch.isfinite(u).all() and (u[:, 6:] == 0).all() and (u[:, :6] != 0).any()
    assert torch.equal(before, env.sim.save_envs())
    env.close()


@pytest.mark.parametrize("case", ob.REFUSAL_CASES)
def test_refusal_messages_equal_the_emulators(case):
    frames, tp, tq, no_out, opts = ob.refusal_args(case, B=2)
    q, v = ob.states(MODEL, 2)
    with pytest.raises(ValueError) as e:
        ob.osc(MODEL, frames, q, v, tp, tq, no_out=no_out, **opts)
    want = str(e.value).split(": ", 1)[1]
    sim = BatchedMujoco(2, robot_file=MODEL)
    vp = lambda a: None if a is None else ctypes.c_void_p(_dev(a).data_ptr())
    keep = [None if a is None else _dev(a) for a in (tp, tq)]
    out = torch.zeros(2, 9, device="cuda:0")
    opt = _lib.JacoOscOptions(**opts)
    arr = (_lib.JacoFrame * max(len(frames), 1))(*frames)
    rc = sim.L.jaco_osc(sim.h, ctypes.cast(arr, ctypes.c_void_p), len(frames), ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), None, None,
                        None if keep[0] is None else ctypes.c_void_p(keep[0].data_ptr()), None if keep[1] is None else ctypes.c_void_p(keep[1].data_ptr()),
                        None, None if no_out else ctypes.c_void_p(out.data_ptr()), None, sim._stream())
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == want
    assert (out == 0).all()
    sim.close()


def test_closed_loop_follows_the_fp64_reference():
    q0, T6 = ob.loop_inputs()
    ep0, er0 = ob.pose_error(ob.LOOP_MODEL, "EE", q0, T6)
    qo = ob.closed_loop_oracle(q0, T6)
    ep1, er1 = ob.pose_error(ob.LOOP_MODEL, "EE", qo, T6)
    assert (np.hypot(ep1, er1) / np.hypot(ep0, er0) < 0.7).all()
    sim = BatchedMujoco(ob.LOOP_B, robot_file=ob.LOOP_MODEL)
    sim.set_option("disable_contact", 1)
    sim.set_state(_dev(q0), torch.zeros(ob.LOOP_B, 9, device="cuda:0"), None)
    fr = [sim.frames.jaco_frame("EE")]
    tp, tq = [_dev(a) for a in ob.kernel_targets(T6)]
    cin = _dev(ob.loop_ctrl_row(q0))
    for _ in range(ob.LOOP_STEPS):
        sim.send_forces(sim.osc(fr, tp, tq, ctrl=cin)["ctrl"], nsub=1)
    qg = sim.get_state()[0].cpu().numpy()
    com = ib.table_of(ob.LOOP_MODEL).com("EE")
    d = np.linalg.norm(ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qg)[0] - ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qo)[0], axis=1)
    print("MEASURE loop: EE distance gpu - reference max %.3g m" % d.max())
    assert d.max() <= LOOP_BOUND, d
    sim.close()
