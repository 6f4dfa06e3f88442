"""GPU tier: jaco_joint (mujoco_jaco_amd/csrc/joint.h) on the MI355X against the formula of include/jaco_env.h in fp64 on the fp64
oracle's qM, qfrc_bias and qvel, against the emulator, and against itself (tests/joint_binding.py holds the inputs, the cases and the
reference; tests/test_joint_emu.py is the CPU-tier twin).

Error measure: max over the active dofs of |u - u_ref| / (1 + |u_ref|).  Bounds = 3 x the largest value measured on the MI355X:
  all terms (PD, qacc_ff, target_qvel), default and non-default gains, B = 67 .................... 9.21e-6 -> 2.8e-5
  targets of unlimited joints shifted by 2 pi k, k in -2 .. 2, and a target across +-pi ........... 4.72e-5 -> 1.4e-4
  limited joint 2 at 0.9 rad, target 5.4 rad ...................................................... 5.48e-6 -> 1.6e-5
  vmax below / above saturation, and the two unsaturated answers of the scale identity ............ 4.51e-6 -> 1.4e-5
  inverse dynamics (kp = kv = 0 with qacc_ff) ..................................................... 7.39e-7 -> 2.2e-6
  dof_mask subsets (one dof, dofs 0-3, dofs 0, 3, 5) .............................................. 6.79e-6 -> 2.0e-5
  GPU against the emulator on the all-terms set ................................................... 1.06e-5 -> 3.2e-5
  closed loop, final arm qpos against the fp64 reference's ........................................ 1.01e-7 rad -> 3.0e-7 rad
jaco2_dual_torque and jaco2_curtain_torque_old (B = 9) share the first bound (largest measured: 7.96e-6).
"""
import ctypes

import numpy as np
import pytest
import torch

import joint_binding as jb
import osc_binding as ob
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError

pytestmark = pytest.mark.gpu
ALL_BOUND = 2.8e-5    # 3 x 9.21e-6 (MI355X)
WRAP_BOUND = 1.4e-4   # 3 x 4.72e-5
LIM_BOUND = 1.6e-5    # 3 x 5.48e-6
SAT_BOUND = 1.4e-5    # 3 x 4.51e-6
ID_BOUND = 2.2e-6     # 3 x 7.39e-7
MASK_BOUND = 2.0e-5   # 3 x 6.79e-6
EMU_BOUND = 3.2e-5    # 3 x 1.06e-5
LOOP_BOUND = 3.0e-7   # rad; 3 x 1.01e-7


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


@pytest.fixture(scope="module")
def sims():
    """One BatchedMujoco per (model, B), opened on first use and closed at the end of the module."""
    open_ = {}

    def get(model, n):
        if (model, n) not in open_:
            open_[(model, n)] = BatchedMujoco(n, robot_file=model)
        return open_[(model, n)]
    yield get
    for s in open_.values():
        s.close()


@pytest.fixture(scope="module")
def run(sims):
    def call(model, q, v, t, tv, ff, cin, **options):
        return sims(model, len(q)).joint(_dev(t), _dev(tv), _dev(ff), _dev(q), _dev(v), _dev(cin), **options).cpu().numpy()
    return call


def abi_call(sim, opt, q, v, t, tv, ff, cin, out):
    """jaco_joint straight through the C ABI on device tensors (None: NULL); returns the return code."""
    vp = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    return sim.L.jaco_joint(sim.h, None if opt is None else ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), vp(q), vp(v), vp(t), vp(tv), vp(ff),
                            vp(cin), vp(out), sim._stream())


def test_all_terms_match_the_fp64_reference(run):
    worst = jb.case_all_terms(run)
    print("MEASURE all terms: error max %.3g" % worst)
    assert worst <= ALL_BOUND, worst


def test_unlimited_joints_wrap_and_take_the_short_way(run):
    worst = jb.case_wrapping(run)
    print("MEASURE wrapping: error max %.3g" % worst)
    assert worst <= WRAP_BOUND, worst


def test_a_limited_joint_follows_the_plain_difference(run):
    worst = jb.case_limited_joint_is_not_wrapped(run)
    print("MEASURE limited joint: error max %.3g" % worst)
    assert worst <= LIM_BOUND, worst


def test_velocity_limit_below_and_above_saturation(run):
    worst, resid, slack = jb.case_saturation(run)
    print("MEASURE saturation: error max %.3g" % worst)
    assert worst <= SAT_BOUND, worst
    assert (resid <= SAT_BOUND * slack).all()   # the same factor sat / max |e| on every dof


def test_inverse_dynamics_and_bias_compensation(run, sims):
    def query_bias(model, q, v):
        return sims(model, len(q)).query([], _dev(q), _dev(v), xpos=False, xmat=False, jac=False, qM=False)["qfrc_bias"].cpu().numpy()
    worst = jb.case_modes(run, query_bias)
    print("MEASURE inverse dynamics: error max %.3g" % worst)
    assert worst <= ID_BOUND, worst


def test_masks_pass_through_and_aliasing(run, sims):
    def run_alias(model, q, v, t, tv, ff, cin, **options):
        sim = sims(model, len(q))
        buf = _dev(cin)
        assert abi_call(sim, _lib.JacoJointOptions(**options), _dev(q), _dev(v), _dev(t), _dev(tv), _dev(ff), buf, buf) == 0
        return buf.cpu().numpy()
    worst = jb.case_masks_and_pass_through(run, run_alias)
    print("MEASURE masks: error max %.3g" % worst)
    assert worst <= MASK_BOUND, worst


def test_two_arms_twelve_dofs_in_one_call(run):
    worst = jb.case_two_arms(run)
    print("MEASURE jaco2_dual_torque: error max %.3g" % worst)
    assert worst <= ALL_BOUND, worst


def test_the_older_curtain_model(run):
    worst = jb.case_other_layout(run)
    print("MEASURE jaco2_curtain_torque_old: error max %.3g" % worst)
    assert worst <= ALL_BOUND, worst


def test_gpu_agrees_with_the_emulator_with_itself_and_with_the_handles_state(run, sims):
    g = jb.regular_inputs()
    u = run(jb.MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], None)
    emu = jb.joint(jb.MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"])
    err = jb.error(u[:, g["mot"]], emu[:, g["mot"]]).max()
    print("MEASURE gpu - emulator: error max %.3g" % err)
    assert err <= EMU_BOUND, err
    assert (jb.bits(run(jb.MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], None)) == jb.bits(u)).all()   # two identical calls
    # qpos = qvel = None: the handle's state, the very floats get_state returns; nothing of the handle is written
    sim = sims(jb.MODEL, jb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (jb.B, 9))), nsub=3)
    version, before = sim.state_version, sim.save_envs().clone()
    qh, vh, _ = sim.get_state()
    t, tv, ff = _dev(g["t"]), _dev(g["tv"]), _dev(g["ff"])
    sim.launch_count()   # (reading the counter resets it)
    a = sim.joint(t, tv, ff)
    assert sim.launch_count() == 1
    b = sim.joint(t, tv, ff, qh, vh)
    assert (jb.bits(a.cpu().numpy()) == jb.bits(b.cpu().numpy())).all()
    assert sim.state_version == version and torch.equal(before, sim.save_envs())


@pytest.mark.parametrize("case", sorted(jb.REFUSALS))
def test_refusals_leave_the_output_untouched(case, sims):
    sim = sims(jb.REFUSAL_MODEL, 2)
    q, _ = ob.states(jb.REFUSAL_MODEL, 2)
    with_target, no_out, opts = jb.refusal_args(case)
    out = torch.full((2, 9), 7.0, device="cuda:0")
    rc = abi_call(sim, _lib.JacoJointOptions(**opts), None, None, _dev(q) if with_target else None, None, None, None, None if no_out else out)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_joint: " + jb.REFUSALS[case]
    assert (out == 7.0).all()
    if not no_out:
        with pytest.raises(JacoError, match="jaco_joint: "):
            sim.joint(_dev(q) if with_target else None, **opts)


def test_an_empty_active_set_is_refused():
    """A model whose every actuator is a position servo (made here: every shipped model has motors), straight through the C ABI."""
    blob = jb.servo_only_blob()
    L = _lib.load(_lib.variant_for(blob))
    buf = ctypes.create_string_buffer(blob, len(blob))
    cfg = _lib.JacoConfig(ctypes.cast(buf, ctypes.c_void_p), len(blob), 2, 0, 50, 0, 0)
    h = ctypes.c_void_p()
    assert L.jaco_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    out = torch.full((2, 9), 7.0, device="cuda:0")
    rc = L.jaco_joint(h, None, None, None, None, None, None, None, ctypes.c_void_p(out.data_ptr()), BatchedMujoco._stream())
    msg = L.jaco_last_error(h).decode()
    L.jaco_destroy(h)
    assert rc == -1 and msg == "jaco_joint: " + jb.EMPTY_MESSAGE and (out == 7.0).all()


def test_closed_loop_follows_the_fp64_reference(sims):
    q0, tp = jb.loop_inputs()
    sim = sims(jb.LOOP_MODEL, jb.LOOP_B)
    sim.set_option("disable_contact", 1)
    sim.set_state(_dev(q0), torch.zeros(jb.LOOP_B, 9, device="cuda:0"), None)
    ik = sim.ik(jb.loop_frame(), _dev(tp))
    assert ik["converged"].all()
    row = ik["qpos"]   # the jaco_ik result row goes in as it is
    qo, errs = jb.closed_loop_oracle(q0, row.cpu().numpy())
    assert (np.diff(errs[:, jb.LOOP_STEPS - 20:], axis=1) < 0).all(), errs
    cin = _dev(ob.loop_ctrl_row(q0))
    for _ in range(jb.LOOP_STEPS):
        sim.send_forces(sim.joint(row, ctrl=cin, **jb.LOOP_GAINS), nsub=1)
    qg = sim.get_state()[0].cpu().numpy()
    d = np.abs(qg[:, :6] - qo[:, :6]).max()
    print("MEASURE loop: joint error %.3g -> %.3g rad in the reference; arm qpos gpu - reference max %.3g rad" % (errs[:, 0].max(), errs[:, -1].max(), d))
    assert d <= LOOP_BOUND, d


def test_robot_config_reaches_the_controller_in_one_launch(sims):
    """env.robot_config.joint() on a sim-tier handle: generate() from a per-joint list is the one launch of sim.joint on the full row."""
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    g = jb.regular_inputs()
    sim = sims(jb.MODEL, jb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    ctl = BatchedMujocoConfig(sim).joint(vmax=0.5, **jb.GAINS)
    t = _dev(g["t"][:, :6])
    sim.launch_count()
    u = ctl.generate(t)
    assert sim.launch_count() == 1
    direct = sim.joint(_dev(g["t"]), **jb.SAT)
    assert (jb.bits(u.cpu().numpy()) == jb.bits(direct.cpu().numpy())).all()
