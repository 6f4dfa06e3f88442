"""CPU tier: BatchedMujoco's own query / ik / osc / joint / rollout_cost / rollout_osc on the emulator (emu_sim.EmuSim replaces the launch
under each, nothing else): the product's output selection, result dictionary, single-frame convenience, choice between jaco_osc and
jaco_osc_task, and defaults, against the emulated entries called directly.  jaco2_curtain_torque, two or three envs."""
import numpy as np
import pytest
import torch

import ik_binding as ib
import joint_binding as jb
import osc_binding as ob
import osc_task_binding as tb
import query_binding as qb
import rollout_cost_binding as cb
import rollout_osc_binding as rob
from emu_sim import EmuSim, _tensors

MODEL = "jaco2_curtain_torque"


def same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def sim():
    return EmuSim(MODEL, *ob.states(MODEL, 3))


def test_query_flags_select_exactly_their_outputs():
    s = EmuSim(MODEL, *ob.states(MODEL, 2))
    fr = [s.frames.jaco_frame("EE")]
    full = s.query(fr)
    assert tuple(full) == qb.OUTS
    for k in qb.OUTS:
        r = s.query(fr, **{o: o == k for o in qb.OUTS})
        assert set(r) == {k} and same_bits(r[k], full[k]), k
    r = s.query([], xpos=False, xmat=False, jac=False)
    assert set(r) == {"qM", "qfrc_bias"} and r["qM"].shape == (2, s.nv, s.nv) and r["qfrc_bias"].shape == (2, s.nv)
    assert s.launches["jaco_query"] == 7 and sum(s.launches.values()) == 7


def test_ik_result_dictionary():
    seeds = ib.picking_seeds(MODEL, 3)
    s = EmuSim(MODEL, seeds, np.zeros((3, 21), np.float32))
    fr = s.frames.jaco_frame("EE", point=np.zeros(3))
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], seeds, 0.3)
    r = s.ik(fr, P, Qt)
    assert set(r) == {"qpos", "converged", "iters", "err_pos", "err_rot"}
    assert r["converged"].dtype == torch.bool and r["iters"].dtype == torch.int32
    raw = ib.ik(MODEL, fr, seeds, P, Qt)
    assert same_bits(r["qpos"], raw["qpos"])
    assert (r["converged"].numpy() == (raw["converged"] != 0)).all() and (r["iters"].numpy() == raw["iters"]).all()
    assert same_bits(r["err_pos"], raw["resid"][:, 0].copy()) and same_bits(r["err_rot"], raw["resid"][:, 1].copy())
    with pytest.raises(ValueError, match="ik: target_pos is required"):
        s.ik(fr, None)


def test_osc_takes_one_frame_and_chooses_its_entry(sim):
    fr = sim.frames.jaco_frame("EE")
    tp, tq = ob.kernel_targets(ob.targets6(MODEL, "EE", sim.qpos.numpy())[:, None, :])
    listed, bare = sim.osc([fr], tp, tq), sim.osc(fr, tp, tq)
    assert set(bare) == {"ctrl", "singular"} and bare["singular"].dtype == torch.bool and bare["singular"].shape == (3, 1)
    assert same_bits(bare["ctrl"], listed["ctrl"]) and same_bits(bare["singular"], listed["singular"])
    assert same_bits(bare["ctrl"], ob.osc(MODEL, [fr], sim.qpos.numpy(), sim.qvel.numpy(), tp, tq)["ctrl"])

    def reached(**task):
        before = dict(sim.launches)
        sim.osc(fr, tp, tq, **task)
        return {k: n - before[k] for k, n in sim.launches.items() if n != before[k]}
    rest = torch.from_numpy(tb.rest_rows(MODEL, "EE", sim.qpos.numpy()))
    moved = dict(axes=tb.POS, null_kv=10.0, rest_qpos=rest, rest_kp=20.0, rest_kv=5.0, rest_mask=0b111000)
    for k, value in moved.items():
        assert reached(**{k: value}) == {"jaco_osc_task": 1}, k
    assert reached(axes=None, null_kv=0.0, rest_qpos=None, rest_kp=0.0, rest_kv=0.0, rest_mask=0) == {"jaco_osc": 1}
    assert reached() == {"jaco_osc": 1}


def test_joint_defaults(sim):
    q, v = sim.qpos.numpy(), sim.qvel.numpy()
    t, tv, ff = jb.targets(MODEL, q), jb.rates(MODEL, 3, 14, 0.5), jb.rates(MODEL, 3, 15, 2.0)
    u = sim.joint(torch.from_numpy(t), torch.from_numpy(tv), torch.from_numpy(ff))
    assert same_bits(u, jb.joint(MODEL, q, v, t, tv, ff))
    assert same_bits(u, sim.joint(t, tv, ff, ctrl=torch.zeros(3, sim.nu)))
    assert sim.calls[-2:] == [{}, {}]


def launched(s):
    return {k: n for k, n in s.launches.items() if n}


def test_rollout_cost_is_the_emulated_entry():
    """2 rollouts x 2 knots x hold 1 of rollout_cost_binding.shared: every output bit for bit the entry's called directly, one launch."""
    g = cb.shared(MODEL)
    c, q, v, w = g["c"][:2, :2], g["q"][:2], g["v"][:2], g["weights"]
    plan = {k: np.ascontiguousarray(g[k][:2, :2]) for k in ("noise", "gain", "xref", "xgoal", "pgoal")}
    s = EmuSim(MODEL, q, v)
    r = s.rollout_cost(c, q, v, noise=plan["noise"], gain=plan["gain"], x_ref=plan["xref"], dofs=g["dofs"], frame=g["ee"], x_goal=plan["xgoal"],
                       p_goal=plan["pgoal"], wx=w["wx"], wx_final=w["wxT"], wu=w["wu"], wp=w["wp"], wp_final=w["wpT"], want=cb.OUTS)
    raw = _tensors(cb.rollout_cost(MODEL, c, q, v, plan["noise"], plan["xgoal"], plan["pgoal"], w, 1, gain=plan["gain"], xref=plan["xref"], dofs=g["dofs"],
                                   frame=g["ee"]))
    assert set(r) == set(cb.OUTS) and all(same_bits(r[k], raw[k]) for k in cb.OUTS)
    assert (r["status"] == 0).all() and torch.isfinite(r["cost"]).all() and launched(s) == {"jaco_rollout_cost": 1}


def test_rollout_osc_is_the_emulated_entry():
    """2 rollouts x 2 knots x hold 1 of rollout_osc_binding.shared: every output bit for bit the entry's called directly, one launch."""
    g = rob.shared(MODEL)
    q, v = g["q"][:2], g["v"][:2]
    tp, tq, c = [np.ascontiguousarray(g[k][:2, :2]) for k in ("tp", "tq", "c")]
    s = EmuSim(MODEL, q, v)
    r = s.rollout_osc(g["frames"], tp, tq, q, v, ctrl=c, frame=g["ee"])
    raw = _tensors(rob.rollout_osc(MODEL, g["frames"], tp, tq, c, q, v, frame=g["ee"]))
    assert set(r) == set(rob.OUTS) and all(same_bits(r[k], raw[k]) for k in rob.OUTS)
    assert (r["status"] == 0).all() and launched(s) == {"jaco_rollout_osc": 1}
