"""GPU tier: jaco_rollout_cost (mujoco_jaco_amd/csrc/rollout_cost.h) on the MI355X against jaco_rollout_fb and jaco_rollout, the cost
formula in fp64, the emulator and itself (tests/rollout_cost_binding.py holds the inputs, the cases and the reference;
tests/test_rollout_cost_emu.py is the CPU-tier twin, whose docstring states the shapes, the measure and the derived cap).

Case 3, |J - J64| / J64 on the call's own fp32 outputs: the derived cap (T (nx + 3 + nu) + 8) 2^-24, and the tight bounds = 3 x the
largest value measured on the MI355X:
  cost / terms over every set, both goal modes, with and without gains, hold 1 and 3 ... 1.46e-7 / 1.29e-7 -> 4.4e-7 / 3.9e-7
  robot_config.rollout_cost .......................................................... 1.62e-7 -> 4.9e-7
GPU against the emulator, default model, cost: the two tiers sum in the same order on trajectories that differ by roundings of the
substep (test_gpu_rollout_fb.py's EMU_BOUNDS), so the costs agree to the states' agreement, not bit for bit: 2.36e-7 -> 7.1e-7.
The MPPI loops' cost ratios are the emulator's to three digits (tests/test_rollout_cost_emu.py).
Bit for bit, across the kernels' translation units: the degenerate call against jaco_rollout_fb, the noisy call against jaco_rollout
on the summed ctrl, cost-only against every output and final_only, two runs, the fan-out against materialised plans.
"""
import numpy as np
import pytest
import torch

import rollout_binding as rb
import rollout_cost_binding as cb
from test_gpu_rollout_fb import GPU, _dev, _host, abi_call as fb_abi_call, run_open  # noqa: F401  (run_open: the fixture, jaco_rollout)

pytestmark = pytest.mark.gpu
COST_BOUND, TERMS_BOUND, CONFIG_BOUND, EMU_BOUND = 4.4e-7, 3.9e-7, 4.9e-7, 7.1e-7
SETS = [(m, False) for m in (rb.MODEL,) + rb.SMALL] + [(rb.LONG_MODEL, True)]
COST_CASES = [(m, False, gpk, gains, hold) for m in (rb.MODEL,) + rb.SMALL for gpk in (0, 1) for gains in (False, True) for hold in (1, 3)] + \
             [(rb.LONG_MODEL, True, gpk, gains, 1) for gpk in (0, 1) for gains in (False, True)]


@pytest.fixture(scope="module")
def sims():
    """One BatchedMujoco per (model, num_envs), opened on first use and closed at the end of the module."""
    from mujoco_jaco_amd.physics import BatchedMujoco
    open_ = {}

    def get(model, n):
        if (model, n) not in open_:
            open_[(model, n)] = BatchedMujoco(n, robot_file=model)
        return open_[(model, n)]
    yield get
    for s in open_.values():
        s.close()


def abi_call(sim, ctrl, qpos0=None, qvel0=None, noise=None, xgoal=None, pgoal=None, weights=None, goal_per_knot=0, kff=None, gain=None, xref=None, dofs=(),
             alpha=None, plan_index=None, state_index=None, nstates=None, frame=None, want=cb.OUTS, hold=1, final_only=0, n=None, nknots=None, nplans=None,
             ndofs=None, no_opt=False, no_out=False, no_ctrl=False, no_plan=False, no_goal=False):
    """jaco_rollout_cost straight through the C ABI on device tensors, the arguments of rollout_cost_binding.rollout_cost: (return code,
    {output: device tensor handed in filled with the sentinels}); for n <= 0 the outputs have one rollout's rows, so that their pointers
    are not NULL."""
    p, ref = GPU.ptr, rb.ref
    c, kf, G, X, al, q0, v0, eps, xg, pg = [GPU.f32(a) for a in (ctrl, kff, gain, xref, alpha, qpos0, qvel0, noise, xgoal, pgoal)]
    pidx, sidx = GPU.i32(plan_index), GPU.i32(state_index)
    n, nknots, nstates, outs = rb.prelude(GPU, (sim.nq, sim.nv, sim.nu), want, c.shape[0], c.shape[1], q0, v0, sim.num_envs, (eps, pidx, sidx, al), n, nknots,
                                          nstates, hold, final_only)
    opt, plan, goal, rec = cb.records(p, outs, c, kf, G, X, al, pidx, eps, xg, pg, weights, dofs, nknots, hold, final_only, goal_per_knot,
                                      c.shape[0] if nplans is None else nplans, ndofs, no_ctrl)
    rc = sim.L.jaco_rollout_cost(sim.h, ref(opt, no_opt), ref(frame), n, p(sidx), nstates, p(q0), p(v0), ref(plan, no_plan), ref(goal, no_goal), ref(rec, no_out),
                                 sim._stream())
    return rc, outs


def _caller(sims, call):
    def run(model, ctrl, qpos0=None, qvel0=None, handle=None, **k):
        if handle is None:
            sim = sims(model, 2)   # (n is not tied to num_envs: any handle of the model serves)
        else:
            sim = sims(model, len(handle[0]))
            sim.set_state(_dev(handle[0]), _dev(handle[1]), None)
        rc, outs = call(sim, ctrl, qpos0, qvel0, **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)
    return run


@pytest.fixture(scope="module")
def run(sims):
    return _caller(sims, abi_call)


@pytest.fixture(scope="module")
def run_fb(sims):
    return _caller(sims, fb_abi_call)


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


@pytest.mark.parametrize("model,long", SETS)
def test_without_noise_it_is_the_closed_loop_rollout(run, run_fb, model, long):
    cb.case_degenerate(run, run_fb, model, long)


@pytest.mark.parametrize("model,long", SETS)
def test_noise_is_one_fp32_add(run, run_open, model, long):
    cb.case_noise(run, run_open, model, long)


@pytest.mark.parametrize("model,long,goal_per_knot,gains,hold", COST_CASES)
def test_cost_matches_the_fp64_formula(run, model, long, goal_per_knot, gains, hold):
    eJ, eT, cap = cb.case_cost(run, model, long, goal_per_knot, gains, hold)
    print("MEASURE cost %s%s goal_per_knot %d gains %d hold %d: cost %.3g terms %.3g (cap %.3g)" % (model, " 50 x 1" if long else "", goal_per_knot, gains, hold, eJ, eT, cap))
    assert eJ <= cap and eT <= cap, (eJ, eT, cap)
    assert eJ <= COST_BOUND and eT <= TERMS_BOUND, (eJ, eT)


@pytest.mark.parametrize("model,long", SETS)
def test_cost_does_not_depend_on_the_outputs_asked_for_and_is_deterministic(run, model, long):
    cb.case_independence(run, model, long)


def test_fan_out_through_the_indices(run):
    cb.case_fan_out(run)


def test_bad_indices_write_the_status_word_alone(run):
    cb.case_bad_index(run)


def test_a_non_finite_rollout_costs_infinity_and_its_neighbours_nothing(run):
    cb.case_non_finite(run)


@pytest.mark.parametrize("case", sorted(cb.REFUSALS))
def test_refusals_leave_the_outputs_untouched(case, sims):
    k = cb.refusal_args(case)
    handle = k.pop("handle", None)
    sim = sims(cb.REFUSAL_MODEL, rb.REFUSAL_ENVS if handle is not None else 2)
    rc, outs = abi_call(sim, **k)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_rollout_cost: " + cb.REFUSALS[case]   # (the emulator's text: test_rollout_cost_emu.py)
    for name, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if name == "status" else rb.SENTINEL)).all(), name


def test_nothing_is_written_and_one_launch(sims):
    """After a few real steps: one launch per call, whatever is asked for; the snapshot of every env, flags, sensordata and state_version
    bitwise unchanged; the NULL state = get_state()'s tensors handed in; n == 0 is OK with zero launches."""
    g = cb.shared(rb.MODEL)
    sim = sims(rb.MODEL, rb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (rb.B, 9))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    w = g["weights"]
    k = dict(noise=_dev(g["noise"]), gain=_dev(g["gain"]), x_ref=_dev(g["xref"]), dofs=g["dofs"], hold=rb.HOLD, frame=g["ee"], x_goal=_dev(g["xgoal"]),
             p_goal=_dev(g["pgoal"]), wx=w["wx"], wx_final=w["wxT"], wu=w["wu"], wp=w["wp"], wp_final=w["wpT"])
    c = _dev(g["c"])
    sim.launch_count()   # (reading the counter resets it)
    a = sim.rollout_cost(c, **k)
    assert sim.launch_count() == 1 and set(a) == {"cost", "terms", "status"} and a["cost"].shape == (rb.B,) and a["terms"].shape == (rb.B, 3)
    b = sim.rollout_cost(c, qh, vh, want=cb.OUTS, **k)
    assert sim.launch_count() == 1 and set(b) == set(cb.OUTS) and all(torch.equal(a[key], b[key]) for key in a)
    assert torch.isfinite(a["cost"]).all() and (a["status"] == 0).all()
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    sim.launch_count()
    rc, outs = abi_call(sim, g["c"][:3], g["q"], g["v"], n=0, want=("qpos", "status", "cost", "terms"))
    assert rc == 0 and sim.launch_count() == 0
    assert (outs["qpos"] == rb.SENTINEL).all() and (outs["cost"] == rb.SENTINEL).all() and (outs["status"] == rb.STATUS_SENTINEL).all()
    r = sim.rollout_cost(c[:0], hold=rb.HOLD, wu=1.0)
    assert r["cost"].shape == (0,) and r["terms"].shape == (0, 3) and sim.launch_count() == 0


def test_gpu_agrees_with_the_emulator(run):
    g = cb.shared(rb.MODEL)
    r = cb.costed(run, rb.MODEL, False, 1, True, g["hold"])
    e = cb.costed(cb.rollout_cost, rb.MODEL, False, 1, True, g["hold"])
    m = float((np.abs(r["cost"].astype(np.float64) - e["cost"]) / e["cost"]).max())
    print("MEASURE gpu - emulator: cost %.3g" % m)
    assert (r["status"] == e["status"]).all()
    assert m <= EMU_BOUND, m


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_robot_config_cost_matches_the_fp64_formula(make_sim, model):
    e, cap = cb.case_config_cost(make_sim, model)
    print("MEASURE robot_config.rollout_cost %s: cost %.3g (cap %.3g)" % (model, e, cap))
    assert e <= cap and e <= CONFIG_BOUND, (e, cap)


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_greedy_mppi_never_increases_the_cost(make_sim, model):
    h = cb.case_mppi(make_sim, model, None)
    print("MEASURE greedy MPPI %s: cost ratios %s" % (model, np.array2string(h[-1] / h[0], precision=3)))
    assert (np.diff(h, axis=0) <= 0).all() and (h[-1] < h[0]).all()


@pytest.mark.parametrize("model", sorted(cb.MPPI_MODELS))
def test_mppi_at_a_finite_temperature_lowers_the_cost(make_sim, model):
    h = cb.case_mppi(make_sim, model, cb.MPPI_TEMPERATURE)
    print("MEASURE MPPI %s temperature %g: cost ratios %s" % (model, cb.MPPI_TEMPERATURE, np.array2string(h[-1] / h[0], precision=3)))
    assert (h[-1] < h[0]).all(), h
