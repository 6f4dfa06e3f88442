"""Device time of one batched closed-loop rollout call (jaco_rollout_fb) at 65 536 rollouts, next to the open-loop kernel on the same
commands and the loop it replaces.

Default model; 4 096 picking reset states (qvel uniform in +-0.5), one plan each -- 50 knots x hold 1: motor commands uniform in +-5,
finger servo commands = the finger angle, a feed-forward step uniform in +-0.3 on the motor words, gains over the 9 hinge dofs (PD
-20 / -2 on the motor-driven pairs, dense +-0.5 on the motor rows, zero servo rows) about x_ref = the start state displaced by 0.02 rad /
0.05 rad/s -- x 16 line-search steps alpha each = 65 536 rollouts, fanned out through plan_index, state_index and alpha.
  (c) closed loop: ONE rollout_feedback call on a 2-env handle; every knot's qpos, qvel, EE pose and applied ctrl
  (o) jaco_rollout on the materialised applied ctrl of (c) ([65 536, 50, 9]), the states fanned out through state_index
  (l) the loop it replaces, on a 65 536-env handle under option disable_contact with the fanned-out states set:
      50 x { get_state(), the law in torch (gather the knot's rows by plan, one batched mat-vec), send_forces(u, 1) }
  (h) (c) with hold 5 (250 substeps), zero-order hold          (p) (h) with per_substep: the law before every substep
  (d) (c) on the two-arm model, gains over its 18 hinge dofs   (e) jaco_rollout on (d)'s applied ctrl
Each timed repetition of (l) starts with the set_state that puts the start states back.  The final state of (c) is compared with
the final state of (o) and of (l) in the same run.
Times: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per repetition; the legs alternate
--repeats times and every repeat is reported (min / median / max).  One JSON line, also written to --out (default
profiles/rollout_fb_bench.txt).
usage: python tools/gpu_rollout_fb_bench.py [--plans 4096] [--alphas 16] [--knots 50] [--iters 10] [--loop-iters 3] [--repeats 3] [--out ...]
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
from tools.gpu_rollout_bench import stats, timed  # noqa: E402


def problem(model, sim, P, T, dev, seed):
    """(qpos, qvel, plan keywords of rollout_feedback, dofs, qpos addresses) of P plans on `model`."""
    M = blob.load(_lib.model_path(model))
    g = torch.Generator(device=dev).manual_seed(seed)
    uni = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g, device=dev)
    qpos = torch.tensor(workload.reset_states(M["qpos0"], P, seed=3, f32_draws=True), dtype=torch.float32, device=dev) if model == "jaco2_curtain_torque" else \
        torch.tensor(np.asarray(M["qpos0"], np.float32), device=dev).repeat(P, 1)
    qvel = uni(-0.5, 0.5, P, sim.nv)
    hinge = [j for j in range(int(M["njnt"][0])) if int(M["jnt_type"][j]) == 3]
    dofs, qadr = [int(M["jnt_dofadr"][j]) for j in hinge], [int(M["jnt_qposadr"][j]) for j in hinge]
    nd = len(dofs)
    ctrl, kff = uni(-5, 5, P, T, sim.nu), uni(-0.3, 0.3, P, T, sim.nu)
    gain = uni(-0.5, 0.5, P, T, sim.nu, 2 * nd)
    for a in range(sim.nu):
        j = int(M["actuator_jntid"][a])
        if M["actuator_position"][a]:
            ctrl[:, :, a] = qpos[:, int(M["jnt_qposadr"][j])][:, None]   # the servos hold their joints
            kff[:, :, a] = 0.0
            gain[:, :, a] = 0.0
        else:
            c = dofs.index(int(M["jnt_dofadr"][j]))
            gain[:, :, a, c] -= 20.0
            gain[:, :, a, nd + c] -= 2.0
    sign = lambda *shape: torch.where(torch.rand(*shape, generator=g, device=dev) < 0.5, -1.0, 1.0)
    xref = torch.cat([qpos[:, qadr] + 0.02 * sign(P, nd), qvel[:, dofs] + 0.05 * sign(P, nd)], 1)[:, None].repeat(1, T, 1).contiguous()
    return qpos, qvel, dict(ctrl=ctrl, gain=gain, x_ref=xref, dofs=dofs, feedforward=kff), qadr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--alphas", type=int, default=16)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)        # rollout calls per timed window
    ap.add_argument("--loop-iters", type=int, default=3)    # repetitions of the 50-step loop per timed window
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_fb_bench.txt"))
    args = ap.parse_args()
    P, A, T, dev, model, dual = args.plans, args.alphas, args.knots, "cuda:0", "jaco2_curtain_torque", "jaco2_dual_torque"
    n = P * A
    small, big, two = BatchedMujoco(2, robot_file=model), BatchedMujoco(n, robot_file=model), BatchedMujoco(2, robot_file=dual)
    big.set_option("disable_contact", 1)
    index = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(A)
    alpha = torch.linspace(0.0, 1.0, A, device=dev).repeat(P).contiguous()
    fan = dict(alpha=alpha, plan_index=index, state_index=index)
    qpos, qvel, plan, qadr = problem(model, small, P, T, dev, 7)
    qpos2, qvel2, plan2, _ = problem(dual, two, P, T, dev, 9)
    frame, frame2 = small.frames.jaco_frame("EE"), two.frames.jaco_frame("EE_1")
    closed = lambda **k: small.rollout_feedback(plan["ctrl"], qpos, qvel, **{k_: v for k_, v in plan.items() if k_ != "ctrl"}, frame=frame, **fan, **k)
    closed2 = lambda: two.rollout_feedback(plan2["ctrl"], qpos2, qvel2, **{k_: v for k_, v in plan2.items() if k_ != "ctrl"}, frame=frame2, **fan)
    r = closed()
    applied = r["ctrl"].contiguous()
    r2 = closed2()
    applied2 = r2["ctrl"].contiguous()
    o = small.rollout(applied, qpos, qvel, state_index=index, frame=frame)
    il = index.long()
    q_all, v_all, ws = qpos[il].contiguous(), qvel[il].contiguous(), torch.zeros(n, small.nv, device=dev)
    dofs = plan["dofs"]

    def loop():
        big.set_state(q_all, v_all, ws)
        for k in range(T):
            q, v, _ = big.get_state()
            d = torch.cat([q[:, qadr], v[:, dofs]], 1) - plan["x_ref"][il, k]
            u = plan["ctrl"][il, k] + alpha[:, None] * plan["feedforward"][il, k] + (plan["gain"][il, k] @ d[:, :, None])[:, :, 0]
            big.send_forces(u.contiguous(), 1)
        return big.get_state()

    lq, lv, _ = loop()
    res = {"model": model, "plans": P, "alphas": A, "rollouts": n, "knots": T, "hold": 1, "dofs": len(dofs), "iters": args.iters, "loop_iters": args.loop_iters,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "status_or": int(r["status"].cpu().numpy().view(np.uint32).max()), "status_or_two_arm": int(r2["status"].cpu().numpy().view(np.uint32).max()),
           "final_qpos_max_abs_diff_vs_open_loop_on_applied_ctrl": float((r["qpos"][:, -1] - o["qpos"][:, -1]).abs().max()),
           "final_qpos_max_abs_diff_vs_loop": float((r["qpos"][:, -1] - lq).abs().max()), "final_qvel_max_abs_diff_vs_loop": float((r["qvel"][:, -1] - lv).abs().max())}
    del r, r2, o, lq, lv
    legs = {
        "c_closed_loop_ms": (closed, args.iters),
        "o_open_loop_on_applied_ctrl_ms": (lambda: small.rollout(applied, qpos, qvel, state_index=index, frame=frame), args.iters),
        "l_loop_ms": (loop, args.loop_iters),
        "h_closed_loop_hold5_ms": (lambda: closed(hold=5), max(args.iters // 3, 1)),
        "p_closed_loop_hold5_per_substep_ms": (lambda: closed(hold=5, per_substep=True), max(args.iters // 3, 1)),
        "d_two_arm_closed_loop_ms": (closed2, args.iters),
        "e_two_arm_open_loop_on_applied_ctrl_ms": (lambda: two.rollout(applied2, qpos2, qvel2, state_index=index, frame=frame2), args.iters),
    }
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, (fn, iters) in legs.items():
            runs[k].append(timed(fn, iters))
    for k in legs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    res["closed_over_open"] = med("c_closed_loop_ms") / med("o_open_loop_on_applied_ctrl_ms")
    res["loop_over_closed"] = med("l_loop_ms") / med("c_closed_loop_ms")
    res["per_substep_over_hold"] = med("p_closed_loop_hold5_per_substep_ms") / med("h_closed_loop_hold5_ms")
    res["two_arm_closed_over_open"] = med("d_two_arm_closed_loop_ms") / med("e_two_arm_open_loop_on_applied_ctrl_ms")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_rollout_fb_bench.py --plans %d --alphas %d --knots %d --iters %d --loop-iters %d --repeats %d\n" % (P, A, T, args.iters, args.loop_iters, args.repeats))
        f.write(json.dumps(res) + "\n")
    for s in (small, big, two):
        s.close()


if __name__ == "__main__":
    main()
