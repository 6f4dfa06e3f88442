"""GPU tier: jaco_rollout_fb (mujoco_jaco_amd/csrc/rollout_fb.h) on the MI355X against jaco_rollout, the law recomputed in fp64, the fp64
oracle in closed loop, the emulator and itself (tests/rollout_fb_binding.py holds the inputs, the cases and the references;
tests/test_rollout_fb_emu.py is the CPU-tier twin, whose docstring states the references, the error measure, the shapes and the
conditions the inputs meet).

Bounds = 3 x the largest value measured on the MI355X:
  qpos / qvel / ctrl against the fp64 closed loop, four models, 6 x 3, both modes ... 3.98e-7 / 2.84e-4 / 9.43e-5 -> 1.2e-6 / 8.5e-4 / 2.8e-4
  qpos / qvel / ctrl against the fp64 closed loop, arm-only model, 50 x 1 ........... 6.80e-8 / 3.31e-5 / 1.28e-5 -> 2.0e-7 / 9.9e-5 / 3.8e-5
  GPU against the emulator, default model, both modes: qpos / qvel / ctrl ........... 6.49e-8 / 1.01e-5 / 4.51e-6 -> 1.9e-7 / 3.0e-5 / 1.3e-5
The law against its fp64 recomputation: the derived bound of rollout_fb_binding.law_bound; the largest ratio measured is 0.36 (robot_config tier: 0.10).
Bit for bit, across the two kernels' translation units: the degenerate call and the zero-deviation call against jaco_rollout, the
closed loop against jaco_rollout on its own commands, the fan-out through the indices against materialised plans and states.
"""
import numpy as np
import pytest
import torch

import rollout_binding as rb
import rollout_fb_binding as fbb
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError
from test_gpu_rollout import GPU, _dev, abi_call as open_abi_call

pytestmark = pytest.mark.gpu
ORACLE_BOUNDS = (1.2e-6, 8.5e-4, 2.8e-4)
LONG_BOUNDS = (2.0e-7, 9.9e-5, 3.8e-5)
EMU_BOUNDS = (1.9e-7, 3.0e-5, 1.3e-5)
SETS = [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)]


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


def abi_call(sim, ctrl, qpos0=None, qvel0=None, kff=None, gain=None, xref=None, dofs=(), alpha=None, plan_index=None, state_index=None, nstates=None,
             frame=None, want=fbb.OUTS, hold=1, final_only=0, per_substep=0, n=None, nknots=None, nplans=None, ndofs=None, no_opt=False, no_out=False,
             no_ctrl=False, no_plan=False):
    """jaco_rollout_fb straight through the C ABI on device tensors, the arguments of rollout_fb_binding.rollout_fb: (return code,
    {output: device tensor handed in filled with the sentinels}); for n <= 0 the outputs have one rollout's rows, so that their pointers
    are not NULL."""
    p, ref = GPU.ptr, rb.ref
    c, kf, G, X, al, q0, v0 = [GPU.f32(a) for a in (ctrl, kff, gain, xref, alpha, qpos0, qvel0)]
    pidx, sidx = GPU.i32(plan_index), GPU.i32(state_index)
    n, nknots, nstates, outs = rb.prelude(GPU, (sim.nq, sim.nv, sim.nu), want, c.shape[0], c.shape[1], q0, v0, sim.num_envs, (pidx, sidx, al), n, nknots, nstates,
                                          hold, final_only, per_substep)
    opt, plan, rec = fbb.records(p, outs, c, kf, G, X, al, pidx, dofs, nknots, hold, final_only, per_substep, c.shape[0] if nplans is None else nplans, ndofs, no_ctrl)
    rc = sim.L.jaco_rollout_fb(sim.h, ref(opt, no_opt), ref(frame), n, p(sidx), nstates, p(q0), p(v0), ref(plan, no_plan), ref(rec, no_out), sim._stream())
    return rc, outs


def _host(outs):
    return {k: (t.cpu().numpy().view(np.uint32) if k == "status" else t.cpu().numpy()) for k, t in outs.items()}


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
        return _host(outs)
    return call


@pytest.fixture(scope="module")
def run_open(sims):
    def call(model, ctrl, qpos0, qvel0, state_index=None, frame=None, want=rb.OUTS, hold=1):
        """jaco_rollout through the C ABI on device tensors."""
        sim = sims(model, 2)
        rc, outs = open_abi_call(sim, ctrl, qpos0, qvel0, state_index, frame=frame, want=want, hold=hold)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)
    return call


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


@pytest.mark.parametrize("model,long", SETS)
def test_without_feedback_it_is_the_open_loop_rollout(run, run_open, model, long):
    fbb.case_degenerate(run, run_open, model, long)


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", (rb.MODEL,) + rb.SMALL)
def test_a_closed_loop_is_an_open_loop_on_its_own_commands(run, run_open, model, per_substep):
    fbb.case_own_commands(run, run_open, model, per_substep)


def test_fifty_knots_are_an_open_loop_on_their_own_commands(run, run_open):
    fbb.case_own_commands(run, run_open, rb.LONG_MODEL, 0, long=True)


@pytest.mark.parametrize("model,long", SETS)
def test_the_law(run, model, long):
    w = fbb.case_law(run, model, long)
    print("MEASURE law %s%s: largest |u - u_ref| / bound %.3g" % (model, " 50 x 1" if long else "", w))
    assert w <= 1.0, w


@pytest.mark.parametrize("per_substep", (0, 1))
@pytest.mark.parametrize("model", (rb.MODEL,) + rb.SMALL)
def test_every_knot_matches_the_closed_loop_oracle(run, model, per_substep):
    eq, ev, eu, _ = fbb.case_oracle(run, model, per_substep)
    print("MEASURE oracle %s per_substep %d: qpos %.3g qvel %.3g ctrl %.3g" % (model, per_substep, eq, ev, eu))
    assert within((eq, ev, eu), ORACLE_BOUNDS), (eq, ev, eu)


def test_fifty_knots_match_the_closed_loop_oracle(run):
    eq, ev, eu, _ = fbb.case_oracle(run, rb.LONG_MODEL, 0, long=True)
    print("MEASURE oracle %s 50 x 1: qpos %.3g qvel %.3g ctrl %.3g" % (rb.LONG_MODEL, eq, ev, eu))
    assert within((eq, ev, eu), LONG_BOUNDS), (eq, ev, eu)


@pytest.mark.parametrize("model,long", SETS)
def test_zero_deviation_is_the_open_loop_rollout(run, run_open, model, long):
    fbb.case_zero_deviation(run, run_open, model, long)


def test_fan_out_through_the_indices(run):
    fbb.case_fan_out(run)


def test_bad_indices_are_flagged_and_write_nothing_else(run):
    fbb.case_bad_index(run)


@pytest.mark.parametrize("case", sorted(fbb.REFUSALS))
def test_refusals_leave_the_outputs_untouched(case, sims):
    k = fbb.refusal_args(case)
    handle = k.pop("handle", None)
    sim = sims(fbb.REFUSAL_MODEL, rb.REFUSAL_ENVS if handle is not None else 2)
    rc, outs = abi_call(sim, **k)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_rollout_fb: " + fbb.REFUSALS[case]   # (the emulator's text: test_rollout_fb_emu.py)
    for name, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if name == "status" else rb.SENTINEL)).all(), name
    if case == "dof_free":
        with pytest.raises(JacoError, match="jaco_rollout_fb: dof 9 belongs to a free joint"):
            sim.rollout_feedback(_dev(k["ctrl"]), _dev(k["qpos0"]), _dev(k["qvel0"]), gain=_dev(k["gain"]), x_ref=_dev(k["xref"]), dofs=k["dofs"])


def test_nothing_is_written_and_one_launch(sims):
    """After a few real steps: one launch per call; the snapshot of every env, flags, sensordata and state_version bitwise unchanged; the
    NULL state = get_state()'s tensors handed in; n == 0 is OK with zero launches."""
    g = fbb.shared(rb.MODEL)
    sim = sims(rb.MODEL, rb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (rb.B, 9))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    c, G, X = _dev(g["c"]), _dev(g["gain"]), _dev(g["xref"])
    ee = rb.frames(rb.MODEL)[1]
    k = dict(gain=G, x_ref=X, dofs=g["dofs"], hold=rb.HOLD, frame=ee)
    sim.launch_count()   # (reading the counter resets it)
    a = sim.rollout_feedback(c, **k)
    assert sim.launch_count() == 1
    b = sim.rollout_feedback(c, qh, vh, per_substep=False, **k)
    assert set(a) == set(fbb.OUTS) and all(torch.equal(a[key], b[key]) for key in a)
    assert a["ctrl"].shape == (rb.B, rb.KNOTS, 9) and not torch.equal(a["ctrl"], c)
    p = sim.rollout_feedback(c, per_substep=True, final_only=True, **k)
    assert p["ctrl"].shape == (rb.B, rb.KNOTS * rb.HOLD, 9) and p["qpos"].shape == (rb.B, 1, sim.nq)
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    sim.launch_count()
    rc, outs = abi_call(sim, g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "status", "ctrl"))
    assert rc == 0 and sim.launch_count() == 0
    assert (outs["qpos"] == rb.SENTINEL).all() and (outs["ctrl"] == rb.SENTINEL).all() and (outs["status"] == rb.STATUS_SENTINEL).all()
    r = sim.rollout_feedback(c[:0], hold=rb.HOLD)
    assert r["qpos"].shape == (0, rb.KNOTS, sim.nq) and r["ctrl"].shape == (0, rb.KNOTS, 9) and sim.launch_count() == 0


@pytest.mark.parametrize("per_substep", (0, 1))
def test_gpu_agrees_with_the_emulator(run, per_substep):
    g = fbb.shared(rb.MODEL)
    r = fbb.closed(run, rb.MODEL, per_substep)
    e = fbb.rollout_fb(rb.MODEL, g["c"], g["q"], g["v"], hold=g["hold"], per_substep=per_substep, want=fbb.STATE + ("ctrl",), **fbb.plan_args(g))
    m = (rb.verr(r["qpos"], e["qpos"]), rb.verr(r["qvel"], e["qvel"]), rb.verr(r["ctrl"], e["ctrl"]))
    print("MEASURE gpu - emulator per_substep %d: qpos %.3g qvel %.3g ctrl %.3g" % ((per_substep,) + m))
    assert (r["status"] == e["status"]).all()
    assert within(m, EMU_BOUNDS), m


@pytest.mark.parametrize("model", sorted(fbb.HOLD_MODELS))
def test_robot_config_holds_a_posture(make_sim, model):
    w = fbb.case_hold_posture(make_sim, model)
    print("MEASURE robot_config.rollout_feedback %s: first knot's |u - u_ref| / bound %.3g" % (model, w))
    assert w <= 1.0, w
