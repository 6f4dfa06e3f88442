"""CPU tier: the cost-expansion kernel (mujoco_jaco_amd/csrc/cost_quad.h, jaco_cost_quad) under the wavefront emulator
(tests/cost_quad_binding.py holds the emulated call, the inputs, the references and the cases; tests/test_gpu_cost_quad.py is the
GPU-tier twin).  R = 3 trajectories x T = 4 knots per model from rollout_binding.inputs' states; the small set (dofs 0, 3, 5 and two
motor words) on all four models, every hinge dof with every ctrl word on the default and the two-arm model (there dofs of BOTH arms
with the frame on arm 1: arm 2's columns of Jp are exact zeros).

Against the reference -- the header's formulas in fp64 on jaco_query's fp32 xpos / jac at the same states and frame (point = 0) -- every
entry of lx, lxx, Vx, Vxx and l within c * 2^-24 * sum |terms|, c counted from the kernel's chain (cost_quad_binding.reference: 5 for a
gradient word, 4 for a block entry, 12 for l); pos and Jp are jaco_query's words bit for bit on the emulator (the same expressions
compiled without contraction).  Largest measured / bound on the emulator: lx, Vx 0.85; lxx, Vxx 0.37; l 0.21.
Against jaco_rollout_cost: sum_k l = cost and each of the three parts = terms within rollout_cost_binding.cap.
Bit for bit: everything cost_quad_binding.case_exact lists; the refusals' texts (the library's: tests/test_gpu_cost_quad.py).
The Python layer on EmuCostQuadSim: ilqr_expand against linearize_rollout and the hand-built joint-space expansion, three launches;
ilqr on 2 envs x 6 knots x 2 iterations with an end-effector goal.
"""
import numpy as np
import pytest

import cost_quad_binding as qc
import rollout_binding as rb
import rollout_cost_binding as cb

EVERY_MODELS = (rb.MODEL, "jaco2_dual_torque")


def run(model, **k):
    return qc.cost_quad(model, k.pop("qpos"), k.pop("qvel"), k.pop("ctrl"), k.pop("dofs"), k.pop("acts"), **k)


@pytest.mark.parametrize("goal_per_knot", (1, 0))
@pytest.mark.parametrize("model", qc.MODELS)
def test_against_the_fp64_reference(model, goal_per_knot):
    qc.case_reference(run, qc.emu_query, model, "small", goal_per_knot)


@pytest.mark.parametrize("model", EVERY_MODELS)
def test_every_hinge_dof_against_the_fp64_reference(model):
    qc.case_reference(run, qc.emu_query, model, "every")


@pytest.mark.parametrize("model", qc.MODELS)
def test_the_sum_of_l_is_jaco_rollout_costs_cost(model):
    qc.case_rollout_cost(run, cb.rollout_cost, model)


@pytest.mark.parametrize("model,which", [(m, "small") for m in qc.MODELS] + [("jaco2_dual_torque", "every")])
def test_what_holds_bit_for_bit(model, which):
    qc.case_exact(run, model, which)


def test_a_bad_goal_index_writes_only_its_status_word():
    qc.case_bad_index(run)


def test_a_non_finite_input_word_is_flagged_in_its_item():
    qc.case_non_finite(run)


def test_no_trajectories_launch_nothing():
    qc.case_empty(run)


def test_state_weights_behind_the_chosen_dofs_are_not_used():
    qc.case_stray_weights(run)


@pytest.mark.parametrize("case", sorted(qc.REFUSALS))
def test_refusals(case):
    k = qc.refusal_args(case)
    with pytest.raises(ValueError) as e:
        run(qc.REFUSAL_MODEL, **k)
    assert str(e.value) == "emu_cost_quad returned -1: jaco_cost_quad: " + qc.REFUSALS[case]
    for name, a in e.value.outputs.items():   # a refusal writes nothing
        assert (a == (rb.STATUS_SENTINEL if name == "status" else rb.SENTINEL)).all(), name


def test_cost_quad_shapes_and_messages():
    import torch
    g = qc.inputs(rb.MODEL)
    sim = qc.EmuCostQuadSim(rb.MODEL, g["q"][:, 0], g["v"][:, 0])
    t = torch.tensor
    w = g["weights"]
    r = sim.cost_quad(t(g["q"]), t(g["v"]), t(g["c"]), dofs=g["dofs"], acts=g["acts"], frame=g["frame"], x_goal=t(g["xgoal"]), p_goal=t(g["pgoal"]),
                      wx=w["wx"], wx_final=w["wxT"], wu=w["wu"], wp=w["wp"], wp_final=w["wpT"])
    assert sim.launches["jaco_cost_quad"] == 1 and set(r) == set(qc.OUTS)
    direct = run(rb.MODEL, **qc.call_args(g, 1))
    for k in qc.OUTS:
        assert r[k].shape == direct[k].shape and (qc.bits(r[k].numpy()) == qc.bits(direct[k])).all(), k
    one = sim.cost_quad(t(g["q"]), t(g["v"]), None, dofs=g["dofs"], acts=g["acts"], x_goal=t(g["xgoal"][:, 0]), wx=2.0, want=("lx", "Vx"))
    assert set(one) == {"lx", "Vx"} and one["lx"].shape == (qc.R, qc.T, 6)
    assert sim.cost_quad(t(g["q"][:0]), t(g["v"][:0]), dofs=g["dofs"], acts=g["acts"], want=("lxx",))["lxx"].shape == (0, qc.T, 6, 6)
    with pytest.raises(ValueError, match="names none or not only outputs"):
        sim.cost_quad(t(g["q"]), t(g["v"]), dofs=g["dofs"], want=("lx", "luu"))
    with pytest.raises(ValueError, match="qvel has shape"):
        sim.cost_quad(t(g["q"]), t(g["v"][:2]), dofs=g["dofs"], want=("lx",))
    with pytest.raises(ValueError, match="x_goal has shape"):
        sim.cost_quad(t(g["q"]), t(g["v"]), dofs=g["dofs"], x_goal=t(g["xgoal"][:, :2]), wx=1.0, want=("lx",))
    with pytest.raises(ValueError, match="jaco_cost_quad: dof 9 belongs to a free joint"):
        sim.cost_quad(t(g["q"]), t(g["v"]), dofs=[9], want=("lx",))


def _tier():
    sims = []

    def make_sim(model, q, v):
        sims.append(qc.EmuCostQuadSim(model, q, v))
        return sims[-1]
    seen = [0]

    def launches():
        total = sum(sims[-1].launches.values())
        since, seen[0] = total - seen[0], total
        return since
    return make_sim, launches


def test_ilqr_expand_is_three_launches_and_the_hand_built_expansion():
    qc.case_ilqr_expand(*_tier(), 2, 6, 3)


@pytest.mark.parametrize("model,ee", (("jaco2_dual_torque", "EE_1"),))
def test_ilqr_expand_on_one_arm_of_two(model, ee):
    """n_robots = 2: arm 1's joints and motor words, an end-effector goal: the expansion is the sim tier's call on the same rows."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    g = qc.inputs(model)
    B, T = 2, 3
    sim = qc.EmuCostQuadSim(model, g["q"][:B, 0], g["v"][:B, 0])
    cfg = BatchedMujocoConfig(sim, ee=ee)
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    u = torch.tensor(g["c"][:B, :T][..., acts])
    ee_goal = torch.tensor(g["pgoal"][:B, 0])
    e = cfg.ilqr_expand(u, ctrl=torch.tensor(g["c"][:B, 0]), hold=2, ee_goal=ee_goal, w_ee=3.0, w_ee_final=30.0, w_u=0.01)
    assert sum(sim.launches.values()) == 3 and sim.launches["jaco_cost_quad"] == 1
    n, m = len(dofs), len(acts)
    assert e["lx"].shape == (B, T, 2 * n) and e["lxx"].shape == (B, T, 2 * n, 2 * n) and e["lu"].shape == (B, T, m) and e["luu"].shape == (m, m)
    assert e["Vx"].shape == (B, 2 * n) and e["Vxx"].shape == (B, 2 * n, 2 * n) and e["l"].shape == (B, T)
    assert e["lx"][:, 1:, :n].abs().max() > 0 and not e["lx"][..., n:].any() and torch.equal(e["lxx"], e["lxx"].transpose(-1, -2))
    assert torch.equal(e["lu"], np.float32(0.01) * e["u"])


def test_ilqr_lowers_the_cost_of_an_end_effector_goal():
    qc.case_ilqr(*_tier(), 2, 6, 3, 2)


def test_ilqr_on_one_arm_of_two():
    """n_robots = 2: the loop on arm 1's joints and motor words of the two-arm model, an end-effector goal: five launches per iteration
    and one at the end, cost never rising, the returned plan re-costed bit for bit."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    model = "jaco2_dual_torque"
    g = qc.inputs(model)
    B, T, iterations = 2, 4, 2
    sim = qc.EmuCostQuadSim(model, g["q"][:B, 1], np.zeros_like(g["v"][:B, 1]))
    cfg = BatchedMujocoConfig(sim, ee="EE_1")
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    ubar = cfg.joint(joints=None).gravity_compensation()
    u = ubar[:, None, acts].expand(-1, T, -1).contiguous()
    q0 = sim.get_state()[0][:, qadr]
    cost = dict(ee_goal=cfg.Tx("EE_1", q=q0 + 0.1).clone(), dq_goal=torch.zeros_like(q0), **qc.ILQR_COST)
    before = sum(sim.launches.values())
    r = cfg.ilqr(u, iterations, ctrl=ubar, hold=2, **cost)
    assert sum(sim.launches.values()) - before == 5 * iterations + 1
    c = r["cost"].numpy()
    assert np.isfinite(c).all() and (c[1:] <= c[:-1]).all() and ((c[1:] < c[:-1]) == r["accepted"].numpy()).all(), c
    assert r["u"].shape == (B, T, len(acts)) and r["x"].shape == (B, T + 1, 2 * len(dofs)) and not r["status"].any()
    assert torch.equal(cfg.rollout_cost(r["u"], ctrl=ubar, hold=2, **cost)["cost"], r["cost"][-1])
    print("MEASURE ilqr two arms: cost / nominal's %s, accepted %s" % (c / c[0], r["accepted"].numpy().sum(0)))
