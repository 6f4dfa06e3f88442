"""Device time of the cost expansion along a batch of trajectories (jaco_cost_quad) next to the path it replaces and next to the other
launches of an iLQR iteration.

4 096 plans x 50 knots on the default model: the plans and states of tools/gpu_rollout_fb_bench.py are rolled out once, and the 204 800
(state after a knot, commanded ctrl of the knot) rows are the input as jaco_rollout_fb wrote them.  9 hinge dofs, 9 ctrl words, the EE
frame, a goal per plan and knot.
  (p) cost_quad, every output, pose weights on            (n) pose weights off (no model tables, no tree walk)
  (l) want = ("l",) with the pose weights on: the walk and the reductions without the lx / lxx stores
  (q) the replaced path: set_state of the 204 800 states into a second handle of that many envs, query for the frame's position and
      Jacobian there, and the same arrays (lx, lxx, lu, Vx, Vxx) assembled in fp32 torch
  (i) one robot_config.ilqr iteration on a 4 096-env handle of jaco2_reaching_torque (the arm's joints and motor words, an end-effector
      goal): ilqr(iterations=2) minus ilqr(iterations=1), and its five launches one by one at the same shapes
  (d) the two-arm model: 18 hinge dofs, 18 ctrl words, the frame on arm 1, --dual-items work items (R x 64 knots)
Everything is MEASURED in this run: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per
repetition; the legs alternate --repeats times and every repeat is reported (min / median / max).  Bytes: what a call must write (its
outputs) and read (its input rows), from the shapes; over the median time that is the call's achieved rate, next to the MI355X's HBM3E
peak of 8 TB/s (the data sheet's figure).  One JSON line, also written to --out (default profiles/cost_quad_bench.txt), with the commit it was
measured on.
usage: python tools/gpu_cost_quad_bench.py [--plans 4096] [--knots 50] [--iters 5] [--repeats 3] [--dual-items 65536] [--commit ID] [--out ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_jaco_amd import _lib, workload  # noqa: E402
from mujoco_jaco_amd.modelc import blob  # noqa: E402
from mujoco_jaco_amd.physics import BatchedMujoco  # noqa: E402
from mujoco_jaco_amd.robot_config import BatchedMujocoConfig  # noqa: E402
from tools.gpu_lqr_bench import commit  # noqa: E402
from tools.gpu_rollout_bench import stats, timed  # noqa: E402
from tools.gpu_rollout_fb_bench import problem  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X, HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dual-items", type=int, default=65536)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_quad_bench.txt"))
    args = ap.parse_args()
    P, T, dev, model = args.plans, args.knots, "cuda:0", "jaco2_curtain_torque"
    n = P * T
    sim = BatchedMujoco(2, robot_file=model)
    qpos, qvel, plan, qadr = problem(model, sim, P, T, dev, 7)
    dofs = plan["dofs"]
    acts = list(range(sim.nu))
    nd, nx, na = len(dofs), 2 * len(dofs), len(acts)
    r = sim.rollout_feedback(plan["ctrl"], qpos, qvel, **{k: v for k, v in plan.items() if k != "ctrl"})
    Q, V, C = r["qpos"], r["qvel"], r["ctrl"]                                  # [P, T, ..]: as the rollout wrote them
    frame = sim.frames.jaco_frame("EE", point=np.zeros(3))
    gen = torch.Generator(device=dev).manual_seed(11)
    X = torch.cat([Q[..., qadr], V[..., dofs]], -1)
    xgoal = X + 0.3 * (2 * torch.rand(P, T, nx, device=dev, generator=gen) - 1)
    pgoal = torch.tensor([0.3, 0.0, 0.5], device=dev) + 0.25 * (2 * torch.rand(P, T, 3, device=dev, generator=gen) - 1)
    wx = np.concatenate([np.linspace(1.0, 3.0, nd), np.linspace(0.02, 0.06, nd)])
    wu = np.linspace(0.01, 0.03, na)
    W = dict(wx=wx, wx_final=10 * wx, wu=wu)
    call = lambda want=("lx", "lxx", "lu", "Vx", "Vxx", "l", "status"), wp=4.0, wpT=40.0: sim.cost_quad(
        Q, V, C, dofs=dofs, acts=acts, frame=frame, x_goal=xgoal, p_goal=pgoal, wp=wp, wp_final=wpT, want=want, **W)
    a = call()
    res = {"plans": P, "knots": T, "items": n, "dofs": nd, "ctrl_words": na, "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "commit": args.commit or commit(), "measured": "every *_ms entry and every ratio below: HIP events, this run",
           "status_or": int(a["status"].cpu().numpy().view("uint32").max()), "hbm_peak_GBs_data_sheet": HBM_PEAK_GBS}
    # the replaced path: a second handle holding the knot states
    big = BatchedMujoco(n, robot_file=model)
    ws = torch.zeros(n, sim.nv, device=dev)
    wxt, wxTt, wut = [torch.tensor(w, dtype=torch.float32, device=dev) for w in (wx, 10 * wx, wu)]
    last = torch.arange(T, device=dev) == T - 1
    Wk = torch.where(last[:, None], wxTt, wxt)                                # [T, nx]
    Wpk = torch.where(last, torch.tensor(40.0, device=dev), torch.tensor(4.0, device=dev))[None, :, None]
    eye = torch.eye(nx, device=dev)

    def replaced():
        big.set_state(Q.reshape(n, -1), V.reshape(n, -1), ws)
        q = big.query([frame], xmat=False, qM=False, qfrc_bias=False)
        Jp = q["jac"][:, 0, :3][:, :, dofs].reshape(P, T, 3, nd)
        e = q["xpos"][:, 0].reshape(P, T, 3) - pgoal
        x = torch.cat([Q[..., qadr], V[..., dofs]], -1)
        g = Wk * (x - xgoal)
        g[..., :nd] += Wpk * (Jp * e[..., None]).sum(2)
        H = (Wk[:, :, None] * eye).expand(P, T, nx, nx).clone()
        H[..., :nd, :nd] += Wpk[..., None] * (Jp.transpose(2, 3) @ Jp)
        z1, z2 = torch.zeros(P, 1, nx, device=dev), torch.zeros(P, 1, nx, nx, device=dev)
        return dict(lx=torch.cat([z1, g[:, :-1]], 1), lxx=torch.cat([z2, H[:, :-1]], 1), lu=wut * C[..., acts], Vx=g[:, -1].contiguous(), Vxx=H[:, -1].contiguous())
    b = replaced()
    for k in ("lx", "lxx", "Vx", "Vxx", "lu"):
        res["%s_vs_replaced_path_max_abs" % k] = float((a[k] - b[k]).abs().max())
    del a, b
    legs = {
        "p_cost_quad_pose_on_ms": lambda: call(),
        "n_cost_quad_pose_off_ms": lambda: call(wp=0.0, wpT=0.0),
        "l_cost_quad_l_alone_ms": lambda: call(("l",)),
        "q_replaced_set_state_query_assembly_ms": replaced,
    }
    # one ilqr iteration on a P-env handle, and its launches one by one
    arm = BatchedMujoco(P, robot_file="jaco2_reaching_torque")
    cfg = BatchedMujocoConfig(arm, ee="EE")
    adofs, aqadr, aacts = cfg._joint_subset(None, "bench")
    ubar = cfg.joint(joints=None).gravity_compensation()
    u0 = ubar[:, None, aacts].expand(-1, T, -1).contiguous()
    q0 = arm.get_state()[0][:, aqadr]
    cost = dict(ee_goal=cfg.Tx("EE", q=q0 + 0.1).clone(), dq_goal=torch.zeros_like(q0), w_ee_final=400.0, w_dq=0.02, w_u=1e-3)
    e = cfg.ilqr_expand(u0, ctrl=ubar, **cost)
    gains, kff, _, st = cfg.ilqr_backward(e["A"], e["B"], e["lxx"], e["luu"], lx=e["lx"], lu=e["lu"], Vxx=e["Vxx"], Vx=e["Vx"], mu=1e-3)
    res.update(ilqr_envs=P, ilqr_knots=T, ilqr_dofs=len(adofs), ilqr_ctrl_words=len(aacts), ilqr_backward_status_or=int(st.cpu().numpy().view("uint32").max()))
    xr = e["x"][:, :-1].contiguous()
    alphas = torch.tensor(BatchedMujocoConfig.ILQR_ALPHAS, device=dev)
    p = cfg._closed_loop("bench", u0, None, None, None, None, None, ubar, None, None, 1)
    rr = p["r"]
    legs.update({
        "i1_ilqr_one_iteration_ms": lambda: cfg.ilqr(u0, 1, ctrl=ubar, **cost),
        "i2_ilqr_two_iterations_ms": lambda: cfg.ilqr(u0, 2, ctrl=ubar, **cost),
        "ia_rollout_feedback_ms": lambda: cfg._closed_loop("bench", u0, None, None, None, None, None, ubar, None, None, 1),
        "ib_transition_fd_ms": lambda: cfg._linearized(p, 1, {}),
        "ic_cost_quad_ms": lambda: arm.cost_quad(rr["qpos"], rr["qvel"], rr["ctrl"], dofs=adofs, acts=aacts, frame=cfg._frames[0], p_goal=cost["ee_goal"],
                                                 x_goal=torch.zeros(P, 2 * len(adofs), device=dev), wx=[0.0] * len(adofs) + [0.02] * len(adofs), wu=1e-3, wp_final=400.0,
                                                 want=("lx", "lxx", "lu", "Vx", "Vxx", "l")),
        "id_ilqr_backward_ms": lambda: cfg.ilqr_backward(e["A"], e["B"], e["lxx"], e["luu"], lx=e["lx"], lu=e["lu"], Vxx=e["Vxx"], Vx=e["Vx"], mu=1e-3),
        "ie_rollout_cost_ladder_ms": lambda: cfg.rollout_cost(e["u"], K=gains, x_ref=xr, k=kff, alphas=alphas, ctrl=ubar, **cost),
    })
    # the two-arm model
    dual = BatchedMujoco(2, robot_file="jaco2_dual_torque")
    Md = blob.load(_lib.model_path("jaco2_dual_torque"))
    Td = 64
    Rd = max(args.dual_items // Td, 1)
    qd = torch.tensor(workload.reset_states_dual(Md["qpos0"], Rd * Td, seed=3), dtype=torch.float32, device=dev).reshape(Rd, Td, -1)
    vd = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (Rd, Td, dual.nv)), dtype=torch.float32, device=dev)
    cd = torch.tensor(np.random.default_rng(7).uniform(-5, 5, (Rd, Td, dual.nu)), dtype=torch.float32, device=dev)
    hinge = [j for j in range(int(Md["njnt"][0])) if int(Md["jnt_type"][j]) == 3]
    ddofs = [int(Md["jnt_dofadr"][j]) for j in hinge][:_lib.JACO_ROLLOUT_FB_MAX_DOFS]
    dframe = dual.frames.jaco_frame("EE_1", point=np.zeros(3))
    xgd = torch.zeros(Rd, Td, 2 * len(ddofs), device=dev)
    pgd = torch.tensor([0.3, 0.0, 0.5], device=dev).expand(Rd, Td, 3).contiguous()
    res.update(dual_items=Rd * Td, dual_dofs=len(ddofs), dual_ctrl_words=dual.nu)
    legs["d_cost_quad_two_arms_ms"] = lambda: dual.cost_quad(qd, vd, cd, dofs=ddofs, acts=list(range(dual.nu)), frame=dframe, x_goal=xgd, p_goal=pgd, wx=1.0,
                                                             wx_final=10.0, wu=0.01, wp=4.0, wp_final=40.0)
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, fn in legs.items():
            runs[k].append(timed(fn, args.iters, warmup=1))
    for k in legs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    out_bytes = 4 * (n * nx + n * nx * nx + n * na + P * nx + P * nx * nx + 2 * n)
    in_bytes = 4 * n * (sim.nq + sim.nv + sim.nu + nx + 3)
    res["bytes_written_every_output"], res["bytes_read"] = out_bytes, in_bytes
    res["pose_on_GBs"] = (out_bytes + in_bytes) / med("p_cost_quad_pose_on_ms") / 1e6
    res["pose_off_GBs"] = (out_bytes + in_bytes) / med("n_cost_quad_pose_off_ms") / 1e6
    res["pose_on_share_of_hbm_peak"] = res["pose_on_GBs"] / HBM_PEAK_GBS
    res["replaced_over_cost_quad_pose_on"] = med("q_replaced_set_state_query_assembly_ms") / med("p_cost_quad_pose_on_ms")
    res["ilqr_iteration_ms_two_minus_one"] = med("i2_ilqr_two_iterations_ms") - med("i1_ilqr_one_iteration_ms")
    five = [med(k) for k in ("ia_rollout_feedback_ms", "ib_transition_fd_ms", "ic_cost_quad_ms", "id_ilqr_backward_ms", "ie_rollout_cost_ladder_ms")]
    res["ilqr_launch_shares"] = dict(zip(("rollout_feedback", "transition_fd", "cost_quad", "ilqr_backward", "rollout_cost_ladder"), [x / sum(five) for x in five]))
    res["ns_per_item_pose_on"] = 1e6 * med("p_cost_quad_pose_on_ms") / n
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_cost_quad_bench.py --plans %d --knots %d --iters %d --repeats %d --dual-items %d\n" % (P, T, args.iters, args.repeats, Rd * Td))
        f.write(json.dumps(res) + "\n")
    for s in (sim, big, arm, dual):
        s.close()


if __name__ == "__main__":
    main()
