"""GPU tier: jaco_cost_quad (mujoco_jaco_amd/csrc/cost_quad.h) on the MI355X against the fp64 reference on jaco_query's words, against
jaco_rollout_cost, bit for bit where the interface says so, and through robot_config.ilqr_expand / ilqr on one handle
(tests/cost_quad_binding.py holds the inputs, the cases and the references; tests/test_cost_quad_emu.py is the CPU-tier twin, whose
docstring states the shapes, the references and the derived bounds).

Against the reference, largest measured / derived bound on the MI355X: lx, Vx 0.85; lxx, Vxx 0.45; l 0.14 -- inside the bound that allows
nothing for a difference between the kernel's pos / Jp and jaco_query's.  Against jaco_rollout_cost: |sum_k l - cost| / cost 1.4e-7 (cap
4.8e-6 .. 6.9e-6).
ilqr on jaco2_reaching_torque, lqr_binding.ILQR_B envs x 20 knots x hold 3, an end-effector goal with w_ee_final = 400, w_dq = 0.02,
w_u = 1e-3, four iterations: 21 launches (five per iteration and the one rollout_feedback that materialises the result); cost over the
nominal's 0.341 .. 0.427 after one iteration, 0.128 .. 0.242 after two, 0.126 .. 0.241 after four; the loop runs under
torch.cuda.set_sync_debug_mode("error") in a test of its own, after a first call that puts its index tensors on the device.
"""
import numpy as np
import pytest
import torch

import cost_quad_binding as qc
import lqr_binding as lb
import rollout_binding as rb
from mujoco_jaco_amd.physics import JacoError
from test_gpu_rollout_cost import _caller, abi_call as cost_abi_call
from test_gpu_rollout import GPU, _dev
from test_gpu_rollout_fb import _host

pytestmark = pytest.mark.gpu
EVERY_MODELS = (rb.MODEL, "jaco2_dual_torque")
ILQR_T, ILQR_HOLD, ILQR_ITERATIONS = 20, 3, 4


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


def abi_call(sim, qpos, qvel, ctrl, dofs, acts, frame=None, xgoal=None, pgoal=None, goal_idx=None, weights=None, goal_per_knot=0, want=qc.OUTS, R=None,
             nknots=None, ngoals=None, no_opt=False, no_out=False, no_goal=False, patch=None):
    """jaco_cost_quad straight through the C ABI on device tensors, the arguments of cost_quad_binding.cost_quad: (return code, {output:
    device tensor handed in filled with the sentinels}); for R <= 0 the outputs have one trajectory's rows, so that no pointer is NULL."""
    q, v, c, xg, pg = [GPU.f32(a) for a in (qpos, qvel, ctrl, xgoal, pgoal)]
    gi = GPU.i32(goal_idx)
    R, T, outs = qc.prelude(GPU, q, v, c, dofs, acts, want, R, nknots)
    opt, goal, rec = qc.records(GPU, outs, dofs, acts, T, xg, pg, gi, weights, goal_per_knot, ngoals, patch)
    rc = sim.L.jaco_cost_quad(sim.h, rb.ref(opt, no_opt), rb.ref(frame), R, GPU.ptr(q), GPU.ptr(v), GPU.ptr(c), rb.ref(goal, no_goal), rb.ref(rec, no_out),
                              sim._stream())
    return rc, outs


@pytest.fixture(scope="module")
def run(sims):
    def call(model, **k):
        sim = sims(model, 2)   # (R is not tied to num_envs: any handle of the model serves)
        rc, outs = abi_call(sim, k.pop("qpos"), k.pop("qvel"), k.pop("ctrl"), k.pop("dofs"), k.pop("acts"), **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)
    return call


@pytest.fixture(scope="module")
def query(sims):
    def call(model, qpos, qvel, frame):
        r = sims(model, len(qpos)).query([frame], _dev(qpos), _dev(qvel), xmat=False, qM=False, qfrc_bias=False)
        return r["xpos"][:, 0].cpu().numpy(), r["jac"][:, 0].cpu().numpy()
    return call


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


@pytest.mark.parametrize("goal_per_knot", (1, 0))
@pytest.mark.parametrize("model", qc.MODELS)
def test_against_the_fp64_reference(run, query, model, goal_per_knot):
    qc.case_reference(run, query, model, "small", goal_per_knot)


@pytest.mark.parametrize("model", EVERY_MODELS)
def test_every_hinge_dof_against_the_fp64_reference(run, query, model):
    qc.case_reference(run, query, model, "every")


@pytest.mark.parametrize("model", qc.MODELS)
def test_the_sum_of_l_is_jaco_rollout_costs_cost(run, sims, model):
    qc.case_rollout_cost(run, _caller(sims, cost_abi_call), model)


@pytest.mark.parametrize("model,which", [(m, "small") for m in qc.MODELS] + [("jaco2_dual_torque", "every")])
def test_what_holds_bit_for_bit(run, model, which):
    qc.case_exact(run, model, which)


def test_a_bad_goal_index_writes_only_its_status_word(run):
    qc.case_bad_index(run)


def test_a_non_finite_input_word_is_flagged_in_its_item(run):
    qc.case_non_finite(run)


def test_state_weights_behind_the_chosen_dofs_are_not_used(run):
    qc.case_stray_weights(run)


def test_the_library_accepts_no_trajectories_and_launches_nothing(run, sims):
    """jaco_cost_quad itself with R = 0 (BatchedMujoco.cost_quad returns before the call): JACO_OK, no launch, every output word untouched."""
    sim = sims(rb.MODEL, 2)
    sim.launch_count()   # (reading the counter resets it)
    qc.case_empty(run)
    assert sim.launch_count() == 0


def test_one_launch_none_for_no_trajectories_and_nothing_written(sims):
    g = qc.inputs(rb.MODEL)
    sim = sims(rb.MODEL, qc.R)
    sim.set_state(_dev(g["q"][:, 0]), _dev(g["v"][:, 0]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (qc.R, 9))), nsub=3)
    version, before, flags = sim.state_version, sim.save_envs().clone(), sim.flags().clone()
    w = g["weights"]
    k = dict(dofs=g["dofs"], acts=g["acts"], frame=g["frame"], x_goal=_dev(g["xgoal"]), p_goal=_dev(g["pgoal"]), wx=w["wx"], wx_final=w["wxT"], wu=w["wu"],
             wp=w["wp"], wp_final=w["wpT"])
    sim.launch_count()   # (reading the counter resets it)
    r = sim.cost_quad(_dev(g["q"]), _dev(g["v"]), _dev(g["c"]), **k)
    assert sim.launch_count() == 1 and set(r) == set(qc.OUTS)
    none = sim.cost_quad(_dev(g["q"][:0]), _dev(g["v"][:0]), _dev(g["c"][:0]), **k)
    assert sim.launch_count() == 0 and none["lxx"].shape == (0, qc.T, 6, 6)
    assert sim.state_version == version and torch.equal(before, sim.save_envs()) and torch.equal(flags, sim.flags())
    with pytest.raises(JacoError, match="jaco_cost_quad: dof 9 belongs to a free joint"):
        sim.cost_quad(_dev(g["q"]), _dev(g["v"]), dofs=[9], want=("lx",))


@pytest.mark.parametrize("case", sorted(qc.REFUSALS))
def test_refusals_leave_the_outputs_untouched(case, sims):
    k = qc.refusal_args(case)
    sim = sims(qc.REFUSAL_MODEL, 2)
    rc, outs = abi_call(sim, k.pop("qpos"), k.pop("qvel"), k.pop("ctrl"), k.pop("dofs"), k.pop("acts"), **k)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_cost_quad: " + qc.REFUSALS[case]   # (the emulator's text: test_cost_quad_emu.py)
    for name, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if name == "status" else rb.SENTINEL)).all(), name


def _launches(make_sim):
    made = []

    def make(model, q, v):
        made.append(make_sim(model, q, v))
        return made[-1]
    return make, lambda: made[-1].launch_count()


def test_ilqr_expand_is_three_launches_and_the_hand_built_expansion(make_sim):
    qc.case_ilqr_expand(*_launches(make_sim), lb.ILQR_B, ILQR_T, ILQR_HOLD)


def test_ilqr_lowers_the_cost_of_an_end_effector_goal(make_sim):
    qc.case_ilqr(*_launches(make_sim), lb.ILQR_B, ILQR_T, ILQR_HOLD, ILQR_ITERATIONS)


def test_the_ilqr_loop_does_not_synchronise(make_sim):
    """The whole of ilqr() under torch's synchronisation check, once its index tensors are on the device (a first call uploads them)."""
    cfg, u, ubar, goal, _ = qc.ilqr_problem(make_sim, lb.ILQR_B, ILQR_T)
    cost = dict(ee_goal=cfg.Tx("EE", q=goal).clone(), dq_goal=torch.zeros_like(goal), **qc.ILQR_COST)
    first = cfg.ilqr(u, 1, ctrl=ubar, hold=ILQR_HOLD, **cost)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = cfg.ilqr(u, 2, ctrl=ubar, hold=ILQR_HOLD, **cost)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again["cost"][:2], first["cost"])
