"""GPU tier: jaco_rollout_osc (mujoco_jaco_amd/csrc/rollout_osc.h) on the MI355X against jaco_rollout, jaco_osc, the loop it replaces,
the fp64 closed loop, the emulator and itself (tests/rollout_osc_binding.py holds the inputs, the cases and the references;
tests/test_rollout_osc_emu.py is the CPU-tier twin, whose docstring states the references, the error measures, the shapes and the
conditions the inputs meet).

Bounds = 3 x the largest value measured on the MI355X:
  qpos / qvel / ctrl / xpos against the fp64 closed loop, four models, 6 x 3, both modes ... 4.16e-7 / 3.05e-4 / 1.30e-5 / 8.59e-8 -> 1.2e-6 / 9.1e-4 / 3.9e-5 / 2.5e-7
  qpos / qvel / ctrl / xpos against the fp64 closed loop, arm-only model, 50 x 1 ........... 3.76e-8 / 6.81e-6 / 8.83e-6 / 7.66e-8 -> 1.1e-7 / 2.0e-5 / 2.6e-5 / 2.2e-7
  ctrl against fp64, singular set ......................................................... 4.13e-6 -> 1.2e-5
  GPU against the emulator, four models, per_substep: qpos / qvel / ctrl ................... 4.32e-7 / 2.24e-4 / 1.13e-5 -> 1.2e-6 / 6.7e-4 / 3.3e-5
  compensated on, against the loop of jaco_osc + send_forces(u, 1), four models: qpos / qvel / ctrl ... 3.88e-8 / 8.37e-7 / 1.08e-5 -> 1.1e-7 / 2.5e-6 / 3.2e-5
  BatchedOSC.rollout holding the current pose, q against the fp64 reference ................ 3.57e-8 -> 1.0e-7
Bit for bit, across the kernels' translation units: the rollout against jaco_rollout on its own commands, the first evaluation against
jaco_osc, and -- on a handle of its own with option compensated = 0, where the tree walk reads no low words -- every evaluation against
jaco_osc on the previous output row, and on the arm-only model the whole call against the loop it replaces (get_state, osc,
send_forces(u, 1) under disable_contact), states and commands.  The fan-out, the outputs' independence, the pass-through words.
"""
import ctypes

import numpy as np
import pytest
import torch

import rollout_binding as rb
import rollout_osc_binding as rob
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError
from test_gpu_rollout_fb import GPU, _dev, _host, run_open, sims, within  # noqa: F401  (the fixtures: one handle per model and size, jaco_rollout)

pytestmark = pytest.mark.gpu
ORACLE_BOUNDS = (1.2e-6, 9.1e-4, 3.9e-5, 2.5e-7)
LONG_BOUNDS = (1.1e-7, 2.0e-5, 2.6e-5, 2.2e-7)
SINGULAR_BOUND = 1.2e-5
EMU_BOUNDS = (1.2e-6, 6.7e-4, 3.3e-5)
LOOP_BOUNDS = (1.1e-7, 2.5e-6, 3.2e-5)
HOLD_BOUND = 1.0e-7


def abi_call(sim, frames, target_pos, target_quat, ctrl=None, qpos0=None, qvel0=None, plan_index=None, state_index=None, nstates=None, frame=None,
             want=rob.OUTS, hold=1, final_only=0, per_substep=1, n=None, nknots=None, nplans=None, nframes=None, opt_nframes=None, no_opt=False, no_out=False,
             no_plan=False, no_pos=False, no_quat=False, **gains):
    """jaco_rollout_osc straight through the C ABI on device tensors, the arguments of rollout_osc_binding.rollout_osc: (return code,
    {output: device tensor handed in filled with the sentinels}); for n <= 0 the outputs have one rollout's rows, so that their pointers
    are not NULL."""
    p, ref = GPU.ptr, rb.ref
    tp, tq, c, q0, v0 = [GPU.f32(a) for a in (target_pos, target_quat, ctrl, qpos0, qvel0)]
    pidx, sidx = GPU.i32(plan_index), GPU.i32(state_index)
    n, nknots, nstates, outs = rb.prelude(GPU, (sim.nq, sim.nv, sim.nu), want, tp.shape[0], tp.shape[1], q0, v0, sim.num_envs, (pidx, sidx), n, nknots, nstates,
                                          hold, final_only, per_substep)
    opt, arr, plan, rec = rob.records(p, outs, frames, c, None if no_pos else tp, None if no_quat else tq, pidx, nknots, hold, final_only, per_substep,
                                      tp.shape[0] if nplans is None else nplans, nframes, opt_nframes, **gains)
    nf = (0 if frames is None else len(frames)) if nframes is None else nframes
    rc = sim.L.jaco_rollout_osc(sim.h, ref(opt, no_opt), None if arr is None else ctypes.cast(arr, ctypes.c_void_p), nf, ref(frame), n, p(sidx), nstates, p(q0), p(v0),
                                ref(plan, no_plan), ref(rec, no_out), sim._stream())
    return rc, outs


@pytest.fixture(scope="module")
def run(sims):
    def call(model, frames, target_pos, target_quat, ctrl=None, qpos0=None, qvel0=None, handle=None, **k):
        if handle is None:
            sim = sims(model, 2)   # (n is not tied to num_envs: any handle of the model serves)
        else:
            sim = sims(model, len(handle[0]))
            sim.set_state(_dev(handle[0]), _dev(handle[1]), None)
        rc, outs = abi_call(sim, frames, target_pos, target_quat, ctrl, qpos0, qvel0, **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)
    return call


def _osc_on(sim, frames, qpos, qvel, target_pos, target_quat, ctrl_in):
    B, nf = len(qpos), len(frames)
    r = sim._osc(frames, _dev(qpos), _dev(qvel), _dev(np.reshape(target_pos, (B, 3 * nf))), _dev(np.reshape(target_quat, (B, 4 * nf))), _dev(ctrl_in), None, None)
    return {"ctrl": r["ctrl"].cpu().numpy(), "status": r["status"].cpu().numpy()}


@pytest.fixture(scope="module")
def run_osc(sims):
    def call(model, frames, qpos, qvel, target_pos, target_quat, ctrl_in):
        return _osc_on(sims(model, len(qpos)), frames, qpos, qvel, target_pos, target_quat, ctrl_in)
    return call


@pytest.fixture(scope="module")
def contact_free():
    """Handles of their own for the loop: (model, n, compensated) -> a BatchedMujoco under disable_contact with that option."""
    open_ = {}

    def get(model, n, compensated):
        key = (model, n, compensated)
        if key not in open_:
            s = BatchedMujoco(n, robot_file=model)
            s.set_option("disable_contact", 1)
            s.set_option("compensated", int(compensated))
            open_[key] = s
        return open_[key]
    yield get
    for s in open_.values():
        s.close()


def _pair(sim):
    """(run, loop) of rollout_osc_binding.case_loop on one handle: the entry, and the loop it replaces."""
    def run_(model, frames, target_pos, target_quat, ctrl=None, qpos0=None, qvel0=None, **k):
        rc, outs = abi_call(sim, frames, target_pos, target_quat, ctrl, qpos0, qvel0, **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)

    def loop(model, frames, q, v, target_pos, target_quat, base):
        n, T = target_pos.shape[:2]
        nf = len(frames)
        sim.set_state(_dev(q), _dev(v), None)
        tp, tq, c = _dev(target_pos), _dev(target_quat), _dev(base)
        Q, V, U = [], [], []
        for k in range(T):
            qk, vk, _ = sim.get_state()
            u = sim.osc(frames, tp[:, k].reshape(n, nf, 3), tq[:, k].reshape(n, nf, 4), qk, vk, c[:, k].contiguous())["ctrl"]
            sim.send_forces(u, 1)
            qn, vn, _ = sim.get_state()
            Q.append(qn.clone()); V.append(vn.clone()); U.append(u.clone())
        return {key: torch.stack(x, 1).cpu().numpy() for key, x in (("qpos", Q), ("qvel", V), ("ctrl", U))}
    return run_, loop


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", rob.MODELS)
def test_an_osc_rollout_is_an_open_loop_on_its_own_commands(run, run_open, model, per_substep):
    rob.case_own_commands(run, run_open, model, per_substep)


def test_fifty_knots_are_an_open_loop_on_their_own_commands(run, run_open):
    rob.case_own_commands(run, run_open, rb.LONG_MODEL, 1, long=True)


@pytest.mark.parametrize("model", rob.MODELS)
def test_the_first_evaluation_is_jaco_osc(run, run_osc, model):
    rob.case_first_evaluation(run, run_osc, model)


@pytest.mark.parametrize("model", rob.MODELS)
def test_without_compensation_every_evaluation_is_jaco_osc(contact_free, model):
    """On a handle with compensated = 0, hold 1: ctrl[:, k] equals jaco_osc on output row k - 1 with target[:, k], bit for bit."""
    g = rob.shared(model)
    sim = contact_free(model, len(g["q"]), False)
    run_, _ = _pair(sim)
    r = run_(model, g["frames"], qpos0=g["q"], qvel0=g["v"], hold=1, want=rob.STATE + ("ctrl",), **rob.args(g))
    for k in range(g["tp"].shape[1]):
        qk, vk = (g["q"], g["v"]) if k == 0 else (r["qpos"][:, k - 1], r["qvel"][:, k - 1])
        o = _osc_on(sim, g["frames"], qk, vk, g["tp"][:, k], g["tq"][:, k], g["c"][:, k])
        assert (rob.bits(r["ctrl"][:, k]) == rob.bits(o["ctrl"])).all(), k


def test_without_compensation_the_call_is_the_loop_it_replaces(contact_free):
    model = "jaco2_reaching_torque"
    run_, loop = _pair(contact_free(model, rob.N, False))
    rob.case_loop(run_, loop, model, bitwise=True)


@pytest.mark.parametrize("model", rob.MODELS)
def test_against_the_loop_it_replaces_with_compensated_on(contact_free, model):
    run_, loop = _pair(contact_free(model, rob.N, True))
    m = rob.case_loop(run_, loop, model, bitwise=False)
    print("MEASURE loop %s: qpos %.3g qvel %.3g ctrl %.3g" % ((model,) + m))
    assert within(m, LOOP_BOUNDS), m


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", rob.MODELS)
def test_every_knot_matches_the_fp64_closed_loop(run, model, per_substep):
    m = rob.case_oracle(run, model, per_substep)
    print("MEASURE oracle %s per_substep %d: qpos %.3g qvel %.3g ctrl %.3g xpos %.3g" % ((model, per_substep) + m))
    assert within(m, ORACLE_BOUNDS), m


def test_fifty_knots_match_the_fp64_closed_loop(run):
    m = rob.case_oracle(run, rb.LONG_MODEL, 1, long=True)
    print("MEASURE oracle %s 50 x 1: qpos %.3g qvel %.3g ctrl %.3g xpos %.3g" % ((rb.LONG_MODEL,) + m))
    assert within(m, LONG_BOUNDS), m


def test_the_singular_set_sets_the_singular_bit(run, run_osc):
    e = rob.case_singular(run, run_osc)
    print("MEASURE singular: ctrl %.3g" % e)
    assert e <= SINGULAR_BOUND, e


@pytest.mark.parametrize("model", rob.MODELS)
def test_gpu_agrees_with_the_emulator(run, model):
    g = rob.shared(model)
    r = rob.call(run, model, 1)
    e = rob.rollout_osc(model, g["frames"], qpos0=g["q"], qvel0=g["v"], frame=g["ee"], hold=g["hold"], per_substep=1, **rob.args(g))
    mot, _ = rob.motors(model)
    m = (rob.verr(r["qpos"], e["qpos"]), rob.verr(r["qvel"], e["qvel"]), float(rob.ob.error(r["ctrl"][..., mot], e["ctrl"][..., mot]).max()))
    print("MEASURE gpu - emulator %s: qpos %.3g qvel %.3g ctrl %.3g" % ((model,) + m))
    assert (r["status"] == e["status"]).all()
    assert within(m, EMU_BOUNDS), m


def test_fan_out_through_the_indices(run):
    rob.case_fan_out(run)


def test_outputs_do_not_depend_on_one_another_or_on_final_only(run):
    rob.case_independence(run)


@pytest.mark.parametrize("model", rob.MODELS)
def test_the_other_ctrl_words_pass_through(run, model):
    rob.case_pass_through(run, model)


def test_bad_indices_are_flagged_and_write_nothing_else(run):
    rob.case_bad_index(run)


@pytest.mark.parametrize("case", sorted(rob.REFUSALS))
def test_refusals(sims, case):
    """Every refusal is JACO_EINVAL with the emulator's message and leaves the outputs untouched."""
    k = rob.refusal_args(case)
    handle = k.pop("handle", None)
    sim = sims(rob.REFUSAL_MODEL, 2 if handle is None else len(handle[0]))
    rc, outs = abi_call(sim, k.pop("frames"), k.pop("target_pos"), k.pop("target_quat"), **k)
    assert rc != 0 and sim.L.jaco_last_error(sim.h).decode() == "jaco_rollout_osc: " + rob.REFUSALS[case]
    for key, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if key == "status" else rb.SENTINEL)).all(), key


def test_nothing_is_written_and_one_launch(sims):
    """After a few real steps: one launch per call; the snapshot of every env, flags, sensordata and state_version bitwise unchanged; the
    NULL state = get_state()'s tensors handed in; n == 0 is OK with zero launches; status alone is an output."""
    model = rb.MODEL
    g = rob.shared(model)
    n = len(g["q"])
    sim = sims(model, n)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (n, sim.nu))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    tp, tq, c = _dev(g["tp"]), _dev(g["tq"]), _dev(g["c"])
    sim.launch_count()   # (reading the counter resets it)
    a = sim.rollout_osc(g["frames"], tp, tq, ctrl=c, hold=rb.HOLD, frame=g["ee"])
    assert sim.launch_count() == 1
    b = sim.rollout_osc(g["frames"], tp, tq, qh, vh, ctrl=c, hold=rb.HOLD, frame=g["ee"])
    assert set(a) == set(rob.OUTS) and all(torch.equal(a[key], b[key]) for key in a)
    assert a["ctrl"].shape == (n, rb.KNOTS * rb.HOLD, sim.nu) and a["qpos"].shape == (n, rb.KNOTS, sim.nq)
    p = sim.rollout_osc(g["frames"], tp, tq, ctrl=c, hold=rb.HOLD, per_substep=False, final_only=True)
    assert p["ctrl"].shape == (n, rb.KNOTS, sim.nu) and p["qpos"].shape == (n, 1, sim.nq) and set(p) == {"qpos", "qvel", "status", "ctrl"}
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    sim.launch_count()
    rc, outs = abi_call(sim, g["frames"], g["tp"][:3], g["tq"][:3], g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "status", "ctrl"))
    assert rc == 0 and sim.launch_count() == 0
    assert (outs["qpos"] == rb.SENTINEL).all() and (outs["ctrl"] == rb.SENTINEL).all() and (outs["status"] == rb.STATUS_SENTINEL).all()
    r = sim.rollout_osc(g["frames"], tp[:0], tq[:0])
    assert r["qpos"].shape == (0, rb.KNOTS, sim.nq) and sim.launch_count() == 0
    rc, outs = abi_call(sim, g["frames"], g["tp"], g["tq"], g["c"], g["q"], g["v"], hold=rb.HOLD, want=("status",))
    assert rc == 0 and set(outs) == {"status"} and torch.equal(outs["status"], a["status"])


def test_an_env_tier_handle_is_left_alone():
    """BatchedOSC.rollout on the sim of a gym-tier env: the env's state, flags and observation-side arrays stay as they were."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, BatchedOSC
    env = JacoBatchedEnv(4)
    try:
        env.reset()
        sim = env.sim
        before, flags = sim.save_envs().clone(), sim.flags().clone()
        osc = BatchedOSC(BatchedMujocoConfig(sim))
        t = torch.zeros(4, 2, 3, 6, device=sim.device)
        t[..., :3] = torch.tensor([0.3, 0.0, 0.5], device=sim.device)
        r = osc.rollout(t, hold=2)
        assert r["q"].shape == (4, 2, 3, 6) and r["u"].shape == (4, 2, 6, sim.nu)
        assert torch.equal(before, sim.save_envs()) and torch.equal(flags, sim.flags())
    finally:
        env.close()


@pytest.mark.parametrize("model", sorted(rob.CONFIG_MODELS))
def test_batched_osc_rollout_holds_the_current_pose(make_sim, model):
    e = rob.case_config(make_sim, model)
    print("MEASURE hold %s: q %.3g" % (model, e))
    assert e <= HOLD_BOUND, e


def test_python_tier_messages(sims):
    g = rob.shared(rb.MODEL)
    sim = sims(rb.MODEL, len(g["q"]))
    fr = g["frames"]
    with pytest.raises(ValueError, match=r"target_pos has shape \(3, 2, 3\), not \[P, T, 1, 3\]"):
        sim.rollout_osc(fr, torch.zeros(3, 2, 3), torch.zeros(3, 2, 1, 4))
    with pytest.raises(ValueError, match=r"target_quat has shape \(3, 2, 1, 3\), not \[3, 2, 1, 4\]"):
        sim.rollout_osc(fr, torch.zeros(3, 2, 1, 3), torch.zeros(3, 2, 1, 3))
    with pytest.raises(ValueError, match=r"ctrl has shape \(3, 1, 9\), not \[3, 2, 9\]"):
        sim.rollout_osc(fr, torch.zeros(3, 2, 1, 3), torch.zeros(3, 2, 1, 4), ctrl=torch.zeros(3, 1, 9))
    with pytest.raises(ValueError, match="4 entries of plan_index but 3 entries of state_index"):
        sim.rollout_osc(fr, torch.zeros(3, 2, 1, 3), torch.zeros(3, 2, 1, 4), plan_index=[0, 1, 2, 0], state_index=[0, 1, 2])
    with pytest.raises(JacoError, match="jaco_rollout_osc: kp, ko, kv, vmax_xyz and vmax_abg must be positive"):
        sim.rollout_osc(fr, torch.zeros(3, 2, 1, 3), torch.zeros(3, 2, 1, 4), kp=-1.0)
