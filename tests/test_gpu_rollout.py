"""GPU tier: jaco_rollout (mujoco_jaco_amd/csrc/rollout.h) on the MI355X against the fp64 oracle, the step kernel, jaco_query, the
emulator and itself (tests/rollout_binding.py holds the inputs, the cases and the references; tests/test_rollout_emu.py is the CPU-tier
twin, whose docstring states the reference, the error measure, the shapes and the conditions the inputs meet).

Bounds = 3 x the largest value measured on the MI355X:
  qpos / qvel against the oracle, four models, 6 x 3 ........................... 3.74e-7 / 1.59e-4 -> 1.1e-6 / 4.8e-4
  qpos / qvel against the oracle, arm-only model, 50 x 1 ....................... 3.88e-8 / 8.26e-6 -> 1.2e-7 / 2.5e-5
  qpos / qvel against the step kernel (disable_contact = 1, set_state, then send_forces(ctrl_k, hold) + get_state per knot), five
    input sets ................................................................ 0 / 0 -> 0 / 0: bit for bit
    (per input set smaller than the figure against the oracle: asserted)
  xpos / xmat against jaco_query at the returned qpos rows ..................... 1.15e-7 / 2.73e-7 -> 3.5e-7 / 8.2e-7
  robot_config: first knot's dq against dq + h forward_dynamics, two models .... 1.88e-8 -> 5.6e-8
  GPU against the emulator, default model: qpos / qvel ......................... 6.49e-8 / 1.02e-5 -> 1.9e-7 / 3.1e-5
"""
import ctypes

import numpy as np
import pytest
import torch

import rollout_binding as rb
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError

pytestmark = pytest.mark.gpu
ORACLE_BOUNDS = (1.1e-6, 4.8e-4)
LONG_BOUNDS = (1.2e-7, 2.5e-5)
STEP_BOUNDS = (0.0, 0.0)
FRAME_BOUNDS = (3.5e-7, 8.2e-7)
CONFIG_BOUND = 5.6e-8
EMU_BOUNDS = (1.9e-7, 3.1e-5)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def within(m, bounds):
    return all(x <= b for x, b in zip(m, bounds))


@pytest.fixture(scope="module")
def sims():
    """One BatchedMujoco per (model, num_envs), opened on first use and closed at the end of the module."""
    open_ = {}

    def get(model, n):
        if (model, n) not in open_:
            open_[(model, n)] = BatchedMujoco(n, robot_file=model)
        return open_[(model, n)]
    yield get
    for s in open_.values():
        s.close()


_TORCH = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
# the GPU tier of rollout_binding.prelude: device tensors, and one rollout's rows for n <= 0, so that no output pointer is NULL
GPU = rb.Tier(lambda a, dtype: _dev(a, _TORCH[dtype]), lambda shape, value, dtype: torch.full(shape, value, dtype=_TORCH[dtype], device="cuda:0"),
              lambda t: ctypes.c_void_p(t.data_ptr()), 1)


def abi_call(sim, ctrl, qpos0=None, qvel0=None, state_index=None, nstates=None, frame=None, want=rb.OUTS, hold=1, final_only=0, n=None, nknots=None,
             no_opt=False, no_out=False, no_ctrl=False):
    """jaco_rollout straight through the C ABI on device tensors, the arguments of rollout_binding.rollout: (return code, {output: device
    tensor handed in filled with the sentinels}); for n <= 0 the outputs have one rollout's rows, so that their pointers are not NULL."""
    p, ref = GPU.ptr, rb.ref
    c, q0, v0, idx = GPU.f32(ctrl), GPU.f32(qpos0), GPU.f32(qvel0), GPU.i32(state_index)
    n, nknots, nstates, outs = rb.prelude(GPU, (sim.nq, sim.nv, sim.nu), want, c.shape[0], c.shape[1], q0, v0, sim.num_envs, n=n, nknots=nknots, nstates=nstates,
                                          hold=hold, final_only=final_only)
    rec = _lib.JacoRolloutOut(*[p(outs.get(k)) for k in rb.OUTS])
    opt = _lib.JacoRolloutOptions(nknots=nknots, hold=hold, final_only=final_only)
    rc = sim.L.jaco_rollout(sim.h, ref(opt, no_opt), ref(frame), n, p(idx), nstates, p(q0), p(v0), None if no_ctrl else p(c), ref(rec, no_out), sim._stream())
    return rc, outs


@pytest.fixture(scope="module")
def run(sims):
    def call(model, ctrl, qpos0=None, qvel0=None, handle=None, **k):
        if handle is None:
            sim = sims(model, 2)   # (n is not tied to num_envs: any handle of the model serves)
        else:
            sim = sims(model, len(handle[0]))
            sim.set_state(_dev(handle[0]), _dev(handle[1]), None)
        rc, outs = abi_call(sim, ctrl, qpos0, qvel0, **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return {k: (t.cpu().numpy().view(np.uint32) if k == "status" else t.cpu().numpy()) for k, t in outs.items()}
    return call


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


def step_kernel(model, g):
    """Case 2's reference: a handle with disable_contact = 1, set_state(q, v, zeros), then send_forces(ctrl_k, hold) + get_state per knot."""
    sim = BatchedMujoco(len(g["q"]), robot_file=model)
    try:
        sim.set_option("disable_contact", 1)
        sim.set_state(_dev(g["q"]), _dev(g["v"]), torch.zeros(len(g["q"]), sim.nv, device="cuda:0"))
        Q, V = [], []
        for k in range(g["c"].shape[1]):
            sim.send_forces(_dev(g["c"][:, k]), g["hold"])
            q, v, _ = sim.get_state()
            Q.append(q.cpu().numpy()); V.append(v.cpu().numpy())
        assert (sim.flags().cpu().numpy() & 31 == 0).all()
        return np.stack(Q, 1), np.stack(V, 1)
    finally:
        sim.close()


@pytest.mark.parametrize("model,long", [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)])
def test_every_knot_matches_the_oracle_and_the_step_kernel(run, model, long):
    eq, ev, r = rb.case_oracle(run, model, long)
    print("MEASURE oracle %s%s: qpos %.3g qvel %.3g" % (model, " 50 x 1" if long else "", eq, ev))
    Q, V = step_kernel(model, rb.shared(model, long))
    sq, sv = rb.verr(r["qpos"], Q), rb.verr(r["qvel"], V)
    print("MEASURE step kernel %s%s: qpos %.3g qvel %.3g" % (model, " 50 x 1" if long else "", sq, sv))
    assert within((eq, ev), LONG_BOUNDS if long else ORACLE_BOUNDS), (eq, ev)
    assert within((sq, sv), STEP_BOUNDS), (sq, sv)
    assert sq < eq and sv < ev, (sq, eq, sv, ev)   # the two fp32 paths agree better with each other than either does with fp64


def test_frame_outputs_match_the_query(run, sims):
    def query(model, qpos, qvel, frame):
        sim = sims(model, len(qpos))
        r = sim.query([frame], _dev(qpos), _dev(qvel), jac=False, qM=False, qfrc_bias=False)
        return r["xpos"][:, 0].cpu().numpy(), r["xmat"][:, 0].cpu().numpy()
    m = rb.case_frames(run, query)
    print("MEASURE frames: xpos %.3g xmat %.3g" % m)
    assert within(m, FRAME_BOUNDS), m


def test_bitwise_self_consistency(run):
    rb.case_self_consistency(run)


def test_bad_state_indices_are_flagged_and_write_nothing_else(run):
    rb.case_bad_index(run)


@pytest.mark.parametrize("case", sorted(rb.REFUSALS))
def test_refusals_leave_the_outputs_untouched(case, sims):
    k = rb.refusal_args(case)
    handle = k.pop("handle", None)
    sim = sims(rb.REFUSAL_MODEL, rb.REFUSAL_ENVS if handle is not None else 2)
    rc, outs = abi_call(sim, **k)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_rollout: " + rb.REFUSALS[case]   # (the emulator's text: test_rollout_emu.py)
    for name, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if name == "status" else rb.SENTINEL)).all(), name
    if case == "hold_0":
        with pytest.raises(JacoError, match="jaco_rollout: nknots 2 x hold 0"):
            sim.rollout(_dev(k["ctrl"]), _dev(k["qpos0"]), _dev(k["qvel0"]), hold=0)


def test_nothing_is_written_and_one_launch(sims):
    """After a few real steps: one launch per call; the snapshot of every env, flags, sensordata and state_version bitwise unchanged; the
    NULL state = get_state()'s tensors handed in (rollout_binding.case_self_consistency); n == 0 is OK with zero launches."""
    g = rb.shared(rb.MODEL)
    sim = sims(rb.MODEL, rb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (rb.B, 9))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    c = _dev(g["c"])
    ee = rb.frames(rb.MODEL)[1]
    sim.launch_count()   # (reading the counter resets it)
    a = sim.rollout(c, hold=rb.HOLD, frame=ee)
    assert sim.launch_count() == 1
    b = sim.rollout(c, qh, vh, hold=rb.HOLD, frame=ee)
    assert set(a) == set(rb.OUTS) and all(torch.equal(a[k], b[k]) for k in a)
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    sim.launch_count()
    rc, outs = abi_call(sim, g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "status"))
    assert rc == 0 and sim.launch_count() == 0
    assert (outs["qpos"] == rb.SENTINEL).all() and (outs["status"] == rb.STATUS_SENTINEL).all()
    assert sim.rollout(c[:0], hold=rb.HOLD)["qpos"].shape == (0, rb.KNOTS, sim.nq) and sim.launch_count() == 0


@pytest.mark.parametrize("model", (rb.MODEL, "jaco2_dual_torque"))
def test_robot_config_rollout(make_sim, model):
    e = rb.case_config(make_sim, model)
    print("MEASURE robot_config.rollout %s: first knot's dq against dq + h forward_dynamics %.3g" % (model, e))
    assert e <= CONFIG_BOUND, e


def test_gpu_agrees_with_the_emulator(run):
    g = rb.shared(rb.MODEL)
    r = run(rb.MODEL, g["c"], g["q"], g["v"], want=("qpos", "qvel", "status"), hold=g["hold"])
    e = rb.rollout(rb.MODEL, g["c"], g["q"], g["v"], want=("qpos", "qvel", "status"), hold=g["hold"])
    m = (rb.verr(r["qpos"], e["qpos"]), rb.verr(r["qvel"], e["qvel"]))
    print("MEASURE gpu - emulator: qpos %.3g qvel %.3g" % m)
    assert (r["status"] == e["status"]).all()
    assert within(m, EMU_BOUNDS), m
