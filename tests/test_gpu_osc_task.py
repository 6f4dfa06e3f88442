"""GPU tier: jaco_osc_task (mujoco_jaco_amd/csrc/osc_task.h) on the MI355X against the fp64 restatement of abr_control's OSC.generate()
with ctrlr_dof and null_controllers (tests/osc_task_binding.py), against jaco_osc, against the emulator and against itself
(tests/test_osc_task_emu.py is the CPU-tier twin; inputs and cases are the same).

Error measure: osc_binding.error, max over the active dofs of |u - u_ref| / (1 + |u_ref|).  Bounds = 3 x the largest value measured on
the MI355X (MEASURE lines of a run with -s):
  regular branch, masks 0b000111 / 0b111000 / 0b100111 / 0b011011 (no env in the band, none singular) .. 5.39e-6 -> 1.6e-5
  pseudo-inverse by count: dof_mask 0b11, position only (n = 2 < k = 3) .............................. 4.44e-6 -> 1.3e-5
  pseudo-inverse branch of the filter: the 8 elbow-scan configurations, all six axes, both null terms .. 2.02e-6 -> 6.0e-6
  null-space terms, position only (both, both with rest_mask = wrist, damping alone, resting alone) .... 8.35e-6 -> 2.5e-5
  the filter: |Js M^-1 du|, du = with - without the null terms (the fp64 reference's own: 6.2e-15) .... 4.43e-6 -> 1.3e-5
  explicit axes 0b111111 against jaco_osc: bit-identical on the MI355X (measured 0); the bound is 8 ulps of an fp32 near 1 + |u|,
  what a regrouping of the last sums could move ........................................................ 0 -> 1e-6
  GPU against the emulator, position only ............................................................. 4.18e-6 -> 1.2e-5
  two frames on jaco2_dual_torque (position only + all six, resting term on both), B = 9 ............... 4.80e-6 -> 1.4e-5
  position only on jaco2_torque (d12) and jaco2_reaching_torque, B = 5 ................................. 3.04e-6 -> 9.1e-6
  closed loop (position only, Damping(10), RestingConfig(q0 + [0, 0, 0, 0.4, -0.4, 0.4], 20, 5)), final EE position against the fp64
  reference's .......................................................................................... 1.26e-7 m -> 3.7e-7 m
"""
import ctypes

import numpy as np
import pytest
import torch

import ik_binding as ib
import osc_binding as ob
import osc_task_binding as tb
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco
from osc_task_binding import ALL, NULL, POS

pytestmark = pytest.mark.gpu
MODEL = "jaco2_curtain_torque"
B = 67
MASKS = (0b000111, 0b111000, 0b100111, 0b011011)
SUBSET_BOUND = 1.6e-5     # 3 x 5.39e-6 (MI355X)
COUNT_BOUND = 1.3e-5      # 3 x 4.44e-6
PINVNULL_BOUND = 6.0e-6   # 3 x 2.02e-6
NULL_BOUND = 2.5e-5       # 3 x 8.35e-6
FILTER_BOUND = 1.3e-5     # 3 x 4.43e-6
ALL6_BOUND = 1e-6         # measured 0: 8 ulps of an fp32 near 1 + |u|
EMU_BOUND = 1.2e-5        # 3 x 4.18e-6
DUAL_BOUND = 1.4e-5       # 3 x 4.80e-6
LAYOUT_BOUND = 9.1e-6     # 3 x 3.04e-6
LOOP_BOUND = 3.7e-7       # m; 3 x 1.26e-7
NULL_CASES = {   # task keywords, rest_mask (None: no resting term)
    "both": (NULL, 0),
    "both_wrist": (NULL, 0b111000),
    "damping": (dict(null_kv=NULL["null_kv"]), None),
    "resting": (dict(rest_kp=NULL["rest_kp"], rest_kv=NULL["rest_kv"]), 0),
}


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t, np.float32)).view(np.uint32)


def motors(model, dofs):
    m = ob.motor_of(model)
    return [m[d] for d in dofs]


def gpu_osc(sim, frames, q, v, tp, tq, ctrl=None, rest=None, **kw):
    r = sim.osc(frames, _dev(tp), _dev(tq), _dev(q), _dev(v), _dev(ctrl), rest_qpos=_dev(rest), **kw)
    return r["ctrl"].cpu().numpy(), r["singular"].cpu().numpy()


@pytest.fixture(scope="module")
def inputs():
    """The inputs of the existing OSC tests, one 67-env handle and jaco_osc's answer, computed once."""
    q, v = ob.states(MODEL, B)
    T6 = ob.targets6(MODEL, "EE", q)
    tp, tq = ob.kernel_targets(T6[:, None, :])
    sim = BatchedMujoco(B, robot_file=MODEL)
    fr = [sim.frames.jaco_frame("EE")]
    u, sing = gpu_osc(sim, fr, q, v, tp, tq)
    yield dict(q=q, v=v, T6=T6[:, None, :], tp=tp, tq=tq, fr=fr, sim=sim, u=u, sing=sing)
    sim.close()


@pytest.fixture(scope="module")
def position_only(inputs):
    """Position-only control without a null term: the fp64 reference and the GPU's answer."""
    g = inputs
    u, sing = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], None, axes=POS)
    return dict(ref=tb.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"], axes=POS), u=u, sing=sing)


@pytest.mark.parametrize("mask", MASKS)
def test_regular_branch_under_axis_subsets(inputs, position_only, mask):
    g = inputs
    ref = position_only["ref"] if mask == POS else tb.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"], axes=mask)
    u, sing = (position_only["u"], position_only["sing"]) if mask == POS else gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], g["tq"] if mask & 56 else None, axes=mask)
    D = ref["det"][:, 0]
    knife = (D > 2.5e-4) & (D < 4e-3)
    reg = D >= 4e-3
    assert knife.mean() <= 0.2, knife.sum()
    if mask == POS:   # position only: fp64 |det X| is 5.07e-3 .. 1.09e-2 on these states, five times above the 1e-3 threshold
        assert D.min() >= 5e-3 and reg.all()
    err = ob.error(u[:, :6], ref["u"][:, 0])
    print("MEASURE subset %s: %d envs compared, error max %.3g" % (bin(mask), reg.sum(), err[reg].max()))
    assert not sing[reg].any()
    assert err[reg].max() <= SUBSET_BOUND, err[reg].max()
    assert (bits(u[:, 6:]) == 0).all()


def test_fewer_dofs_than_rows_take_the_pseudo_inverse_by_count(inputs):
    g = inputs
    ref = tb.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"], axes=POS, dof_mask=0b11)
    cin = np.random.default_rng(4).normal(size=(B, 9)).astype(np.float32)
    u, sing = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], None, cin, axes=POS, dof_mask=0b11)
    err = ob.error(u[:, :2], ref["u"][:, 0, :2])
    print("MEASURE count: n = 2 < k = 3, error max %.3g" % err.max())
    assert sing.all()
    assert (bits(u[:, 2:]) == bits(cin[:, 2:])).all()
    assert err.max() <= COUNT_BOUND, err.max()


def test_pseudo_inverse_branch_serves_the_filter():
    q, v = ob.singular_states(MODEL, "EE", want=8)
    T6 = ob.targets6(MODEL, "EE", q)[:, None, :]
    tp, tq = ob.kernel_targets(T6)
    rest = tb.rest_rows(MODEL, "EE", q)
    ref = tb.reference(MODEL, ["EE"], q, v, T6, axes=ALL, rest_qpos=rest, **NULL)
    assert ref["sing"].all() and (ref["det"] < 2.5e-4).all()
    sim = BatchedMujoco(len(q), robot_file=MODEL)
    u, sing = gpu_osc(sim, [sim.frames.jaco_frame("EE")], q, v, tp, tq, None, rest, axes=ALL, **NULL)
    err = ob.error(u[:, :6], ref["u"][:, 0])
    print("MEASURE pinv + null: error max %.3g" % err.max())
    assert sing.all()
    assert err.max() <= PINVNULL_BOUND, err.max()
    sim.close()


def null_case(g, label):
    kw, rm = NULL_CASES[label]
    rest = None if rm is None else tb.rest_rows(MODEL, "EE", g["q"], mask=rm)
    ref = tb.reference(MODEL, ["EE"], g["q"], g["v"], g["T6"], axes=POS, rest_qpos=rest, rest_mask=rm or 0, **kw)
    return rest, dict(axes=POS, rest_mask=rm or 0, **kw), ref


@pytest.mark.parametrize("label", list(NULL_CASES))
def test_null_space_terms_match_the_fp64_reference(inputs, position_only, label):
    g = inputs
    rest, task, ref = null_case(g, label)
    u, sing = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], None, None, rest, **task)
    assert np.abs(ref["u"] - position_only["ref"]["u"]).max() > 1.0   # (the term matters)
    err = ob.error(u[:, :6], ref["u"][:, 0])
    print("MEASURE null %s: error max %.3g" % (label, err.max()))
    assert not sing.any() and np.isfinite(u).all()
    assert err.max() <= NULL_BOUND, err.max()


def test_null_space_torques_do_not_move_the_task(inputs, position_only):
    g = inputs
    rest, task, ref = null_case(g, "both")
    u, _ = gpu_osc(g["sim"], g["fr"], g["q"], g["v"], g["tp"], None, None, rest, **task)
    du = u[:, :6].astype(np.float64) - position_only["u"][:, :6].astype(np.float64)
    img = np.array([np.abs(ref["Js"][e][0] @ np.linalg.solve(ref["M"][e][0], du[e])).max() for e in range(B)])
    n = np.linalg.norm(du, axis=1)
    print("MEASURE filter: |Js M^-1 du| max %.3g, |du| %.3g .. %.3g" % (img.max(), n.min(), n.max()))
    assert np.abs(du).max() > 1.0   # (du is not zero: the terms act)
    assert img.max() <= FILTER_BOUND, img.max()


def test_equivalences_with_jaco_osc_the_emulator_and_itself(inputs, position_only):
    g = inputs
    sim = g["sim"]
    # a NULL task record is jaco_osc: the same kernel, bit for bit (straight through the C ABI)
    tp, tq, qd, vd = _dev(g["tp"]), _dev(g["tq"]), _dev(g["q"]), _dev(g["v"])
    out, st = torch.empty(B, 9, device="cuda:0"), torch.empty(B, 1, dtype=torch.int32, device="cuda:0")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    arr = (_lib.JacoFrame * 1)(*g["fr"])
    sim.launch_count()
    rc = sim.L.jaco_osc_task(sim.h, ctypes.cast(arr, ctypes.c_void_p), 1, None, None, vp(qd), vp(vd), vp(tp), vp(tq), None, None, vp(out), vp(st), sim._stream())
    assert rc == 0 and sim.launch_count() == 1
    assert (bits(out) == bits(g["u"])).all() and ((st.cpu().numpy() != 0) == g["sing"]).all()
    # explicit all six axes, no null term: jaco_osc's answer from the other kernel
    six, sing6 = gpu_osc(sim, g["fr"], g["q"], g["v"], g["tp"], g["tq"], axes=ALL)
    err = ob.error(six[:, :6], g["u"][:, :6])
    print("MEASURE all six - jaco_osc: error max %.3g, bit-identical: %s" % (err.max(), (bits(six) == bits(g["u"])).all()))
    assert (sing6 == g["sing"]).all()
    assert err.max() <= ALL6_BOUND, err.max()
    # the emulator, position only
    emu = tb.osc_task(MODEL, g["fr"], g["q"], g["v"], g["tp"], None, axes=POS)
    err = ob.error(position_only["u"][:, :6], emu["ctrl"][:, :6])
    print("MEASURE gpu - emulator: error max %.3g" % err.max())
    assert err.max() <= EMU_BOUND, err.max()
    assert ((emu["status"] != 0) == position_only["sing"]).all()
    # itself, and one launch per call
    sim.launch_count()
    again, sing = gpu_osc(sim, g["fr"], g["q"], g["v"], g["tp"], None, axes=POS)
    assert sim.launch_count() == 1
    assert (bits(again) == bits(position_only["u"])).all() and (sing == position_only["sing"]).all()


def test_two_frames_with_different_axes_and_a_resting_term_on_both():
    model, names, nenv = "jaco2_dual_torque", ["EE_1", "EE_2"], 9
    q, v = ob.states(model, nenv)
    T6 = np.stack([ob.targets6(model, n, q) for n in names], 1)
    tp, tq = ob.kernel_targets(T6)
    rest = tb.rest_rows(model, "EE_1", q)
    rest = np.where(np.isnan(rest), tb.rest_rows(model, "EE_2", q, seed=18), rest)
    kw = dict(rest_kp=NULL["rest_kp"], rest_kv=NULL["rest_kv"])
    ref = tb.reference(model, names, q, v, T6, axes=[POS, ALL], rest_qpos=rest, **kw)
    sim = BatchedMujoco(nenv, robot_file=model)
    fr = [sim.frames.jaco_frame(n) for n in names]
    cin = np.random.default_rng(6).normal(size=(nenv, 18)).astype(np.float32)
    u, sing = gpu_osc(sim, fr, q, v, tp, tq, cin, rest, axes=[POS, ALL], **kw)
    mine = [motors(model, a) for a in ref["acts"]]
    err = max(ob.error(u[:, mine[f]], ref["u"][:, f]).max() for f in range(2))
    print("MEASURE dual: error max %.3g" % err)
    assert not sing.any()
    assert err <= DUAL_BOUND, err
    others = [a for a in range(18) if a not in mine[0] + mine[1]]
    assert len(others) == 6 and (bits(u[:, others]) == bits(cin[:, others])).all()
    one, _ = gpu_osc(sim, fr[:1], q, v, tp[:, :1], None, cin, rest, axes=POS, **kw)   # one arm alone: the other arm's words pass through too
    assert (bits(one[:, others + mine[1]]) == bits(cin[:, others + mine[1]])).all()
    assert (bits(one[:, mine[0]]) == bits(u[:, mine[0]])).all()
    sim.close()


@pytest.mark.parametrize("model", ["jaco2_torque", "jaco2_reaching_torque"])
def test_position_only_on_the_other_builds(model):
    q, v = ob.states(model, 5)
    T6 = ob.targets6(model, "EE", q)[:, None, :]
    tp = ob.kernel_targets(T6)[0]
    ref = tb.reference(model, ["EE"], q, v, T6, axes=POS)
    sim = BatchedMujoco(5, robot_file=model)
    u, sing = gpu_osc(sim, [sim.frames.jaco_frame("EE")], q, v, tp, None, axes=POS)
    err = ob.error(u[:, motors(model, ref["acts"][0])], ref["u"][:, 0])
    print("MEASURE layout %s: error max %.3g" % (model, err.max()))
    assert (ref["det"] >= 4e-3).all() and not sing.any()
    assert err.max() <= LAYOUT_BOUND, err.max()
    sim.close()


@pytest.mark.parametrize("case", list(tb.REFUSALS))
def test_refusal_messages_equal_the_emulators(inputs, case):
    g = inputs
    sim = g["sim"]
    tq, rest, task = tb.refusal_args(case, B)
    with pytest.raises(ValueError) as e:
        tb.osc_task(MODEL, g["fr"], g["q"], g["v"], g["tp"], tq, None, rest, **task)
    want = str(e.value).split(": ", 1)[1]
    assert want == "jaco_osc_task: " + tb.REFUSALS[case]
    raw = task.pop("raw_axes", None)
    rec = tb.task_record(1, **task)
    if raw is not None:
        rec.axes[:] = raw
    keep = [_dev(a) for a in (g["tp"], tq, rest)]
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    out = torch.zeros(B, 9, device="cuda:0")
    arr = (_lib.JacoFrame * 1)(*g["fr"])
    sim.launch_count()
    rc = sim.L.jaco_osc_task(sim.h, ctypes.cast(arr, ctypes.c_void_p), 1, None, ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), None, None,
                             vp(keep[0]), vp(keep[1]), vp(keep[2]), None, vp(out), None, sim._stream())
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == want
    assert sim.launch_count() == 0 and (out == 0).all()


def test_closed_loop_follows_the_fp64_reference():
    q0, T6 = ob.loop_inputs()
    rest = tb.loop_rest(q0)
    qo = tb.closed_loop_oracle(q0, T6, rest)
    sim = BatchedMujoco(ob.LOOP_B, robot_file=ob.LOOP_MODEL)
    sim.set_option("disable_contact", 1)
    sim.set_state(_dev(q0), torch.zeros(ob.LOOP_B, 9, device="cuda:0"), None)
    fr = [sim.frames.jaco_frame("EE")]
    tp, cin, rest_dev = _dev(ob.kernel_targets(T6)[0]), _dev(ob.loop_ctrl_row(q0)), _dev(rest)
    for _ in range(ob.LOOP_STEPS):
        sim.send_forces(sim.osc(fr, tp, ctrl=cin, axes=POS, rest_qpos=rest_dev, **NULL)["ctrl"], nsub=1)
    qg = sim.get_state()[0].cpu().numpy()
    com = ib.table_of(ob.LOOP_MODEL).com("EE")
    po, pg = ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qo)[0], ib.oracle_pose(ob.LOOP_MODEL, "EE", com, qg)[0]
    d = np.linalg.norm(pg - po, axis=1)
    left = np.linalg.norm(po - T6[:, :3], axis=1)
    print("MEASURE loop: the reference ends %.3g .. %.3g m from its targets; EE distance gpu - reference max %.3g m" % (left.min(), left.max(), d.max()))
    assert np.isfinite(qg).all()
    assert d.max() <= LOOP_BOUND, d
    sim.close()


def test_python_surface_reaches_the_right_entry_and_leaves_the_handle_alone(inputs, position_only):
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, BatchedOSC, Damping, RestingConfig
    g = inputs
    sims = [g["sim"], BatchedMujoco(B, robot_file=MODEL)]
    ctrl = _dev(np.random.default_rng(8).uniform(-0.2, 0.2, (B, 9)))
    for s in sims:
        s.set_state(_dev(g["q"]), _dev(g["v"]), None)
        s.send_forces(ctrl, nsub=2)
    sim = sims[0]
    version = sim.state_version
    qh, vh, _ = [t.cpu().numpy() for t in sim.get_state()]
    a, b, c = 0.3, -1.1, 2.0
    ctl = BatchedOSC(BatchedMujocoConfig(sim), ctrlr_dof=[1, 1, 1, 0, 0, 0], null_controllers=[Damping(10), RestingConfig([None, None, None, a, b, c], 20, 5)])
    sim.launch_count()
    u = ctl.generate_pose(_dev(g["tp"][:, 0]))
    assert sim.launch_count() == 1
    rest = np.full(g["q"].shape, np.nan, np.float32)
    rest[:, 3:6] = np.float32([a, b, c])
    frame0 = [sim.frames.jaco_frame("EE", point=np.zeros(3))]
    raw, _ = gpu_osc(sim, frame0, qh, vh, g["tp"], None, None, rest, axes=POS, rest_mask=0b111000, **NULL)
    assert (bits(u) == bits(raw)).all() and np.isfinite(raw).all()
    with pytest.raises(ValueError, match="needs target quaternions"):
        BatchedOSC(BatchedMujocoConfig(sim)).generate_pose(_dev(g["tp"][:, 0]))
    # without a task keyword BatchedMujoco.osc calls jaco_osc: on the given state it is the module's jaco_osc answer, bit for bit
    plain, _ = gpu_osc(sim, g["fr"], g["q"], g["v"], g["tp"], g["tq"])
    assert (bits(plain) == bits(g["u"])).all()
    # the handle: state, flags, sensordata and a following step equal a twin's that never called the controller
    assert sim.state_version == version
    snap = lambda s: [t.clone() for t in s.get_state()] + [s.flags().clone(), s.sensordata().clone()]
    for s in sims:
        s.send_forces(ctrl, nsub=3)
    for x, y in zip(snap(sims[0]), snap(sims[1])):
        assert torch.equal(x, y)
    sims[1].close()
