"""Device time and peak memory of one costed rollout call (jaco_rollout_cost, cost and status only) at 65 536 rollouts, next to what it
replaces: jaco_rollout / jaco_rollout_fb with every knot's outputs followed by the same quadratic cost in fp32 torch.

Three shapes, 50 knots x hold 1 each, the states and plans of tools/gpu_rollout_fb_bench.py (`problem`):
  (s) sampling, profiles/rollout_bench.txt's: 64 states with one nominal each x 1 024 noise samples (motor words +-0.5), no gains
        s_cost     one rollout_cost call, want = cost + status
        s_replaced nominal + noise in torch, jaco_rollout with every knot's qpos, qvel and EE pose, the cost in torch
        s_open     jaco_rollout alone on the materialised ctrl (every knot)    s_open_final: the same, final_only
  (l) line search, profiles/rollout_fb_bench.txt's: 4 096 plans x 16 step sizes, gains over the 9 hinge dofs
        l_cost / l_replaced (rollout_feedback with every knot + the cost in torch) / l_closed (rollout_feedback alone)
  (d) (l) on the two-arm model, gains over its 18 hinge dofs: d_cost / d_replaced / d_closed
The cost: state weights on every hinge dof (angles 2, velocities 0.05; last knot x 10), ctrl weights 0.02, pose weight 4 (last knot 40),
one goal per plan.  The torch cost and the kernel's are compared in the same run (largest relative difference).
Times: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per repetition; the legs alternate
--repeats times and every repeat is reported (min / median / max).  Peak memory: torch.cuda.max_memory_allocated over one call of each
way, above what the inputs hold.  One JSON line, also written to --out (default profiles/rollout_cost_bench.txt) under what is
already there (the resource remarks are kept by hand).
usage: python tools/gpu_rollout_cost_bench.py [--states 64] [--samples 1024] [--plans 4096] [--alphas 16] [--knots 50] [--iters 10] [--repeats 3] [--out ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_jaco_amd.physics import BatchedMujoco  # noqa: E402
from tools.gpu_rollout_bench import stats, timed  # noqa: E402
from tools.gpu_rollout_fb_bench import problem  # noqa: E402

WQ, WV, WU, WP, LAST = 2.0, 0.05, 0.02, 4.0, 10.0


def torch_cost(r, u, dofs, qadr, plan_of, xgoal, pgoal, nu):
    """The cost of jaco_rollout_cost in fp32 torch on every knot's outputs r and the applied ctrl u [n, T, nu]."""
    nd, T = len(dofs), u.shape[1]
    x = torch.cat([r["qpos"][..., qadr], r["qvel"][..., dofs]], 2)
    wx = torch.cat([torch.full((nd,), WQ), torch.full((nd,), WV)]).to(u.device)
    knot = torch.ones(T, device=u.device)
    knot[-1] = LAST
    sx = 0.5 * ((x - xgoal[plan_of][:, None]) ** 2 * wx).sum(2)
    sp = 0.5 * WP * ((r["xpos"] - pgoal[plan_of][:, None]) ** 2).sum(2)
    return 0.5 * WU * (u * u).sum((1, 2)) + ((sx + sp) * knot).sum(1)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--alphas", type=int, default=16)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_cost_bench.txt"))
    args = ap.parse_args()
    S, K, P, A, T, dev = args.states, args.samples, args.plans, args.alphas, args.knots, "cuda:0"
    model, dual = "jaco2_curtain_torque", "jaco2_dual_torque"
    one, two = BatchedMujoco(2, robot_file=model), BatchedMujoco(2, robot_file=dual)
    g = torch.Generator(device=dev).manual_seed(11)
    legs, checks, peaks = {}, {}, {}

    def goals(sim, qpos, qvel, dofs, qadr, n):
        nd = len(dofs)
        xgoal = torch.cat([qpos[:, qadr], qvel[:, dofs]], 1) + 0.3 * (2 * torch.rand(n, 2 * nd, generator=g, device=dev) - 1)
        pgoal = torch.tensor([0.3, 0.0, 0.5], device=dev) + 0.25 * (2 * torch.rand(n, 3, generator=g, device=dev) - 1)
        w = dict(wx=[WQ] * nd + [WV] * nd, wx_final=[LAST * WQ] * nd + [LAST * WV] * nd, wu=WU, wp=WP, wp_final=LAST * WP)
        return xgoal.contiguous(), pgoal.contiguous(), w

    # (s) sampling: S states with one nominal each x K noise samples, no gains
    qpos, qvel, plan, qadr = problem(model, one, S, T, dev, 7)
    dofs, frame = plan["dofs"], one.frames.jaco_frame("EE")
    xg, pg, w = goals(one, qpos, qvel, dofs, qadr, S)
    index = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(K)
    il = index.long()
    servo = (plan["gain"].abs().sum((0, 1, 3)) == 0)   # (`problem` zeroes the servo rows)
    noise = (torch.rand(S * K, T, one.nu, generator=g, device=dev) - 0.5) * torch.where(servo, 0.0, 1.0)
    s_cost = lambda: one.rollout_cost(plan["ctrl"], qpos, qvel, noise=noise, dofs=dofs, plan_index=index, state_index=index, frame=frame, x_goal=xg, p_goal=pg,
                                      want=("cost", "status"), **w)

    def s_replaced():
        u = plan["ctrl"][il] + noise
        return torch_cost(one.rollout(u, qpos, qvel, state_index=index, frame=frame), u, dofs, qadr, il, xg, pg, one.nu)
    applied = (plan["ctrl"][il] + noise).contiguous()
    legs.update(s_cost_ms=s_cost, s_replaced_ms=s_replaced, s_open_ms=lambda: one.rollout(applied, qpos, qvel, state_index=index, frame=frame),
                s_open_final_ms=lambda: one.rollout(applied, qpos, qvel, state_index=index, frame=frame, final_only=True))
    a, b = s_cost(), s_replaced()
    checks["s"] = (float(((a["cost"] - b).abs() / b).max()), int(a["status"].cpu().numpy().view(np.uint32).max()))
    del a, b
    peaks.update(s_cost_MiB=peak(s_cost), s_replaced_MiB=peak(s_replaced))

    # (l), (d) line search: P plans x A step sizes, gains over every hinge dof
    fan_index = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(A)
    alpha = torch.linspace(0.0, 1.0, A, device=dev).repeat(P).contiguous()
    fan = dict(alpha=alpha, plan_index=fan_index, state_index=fan_index)
    fl = fan_index.long()
    for tag, sim, name, ee, seed in (("l", one, model, "EE", 7), ("d", two, dual, "EE_1", 9)):
        q2, v2, pl, qa = problem(name, sim, P, T, dev, seed)
        fr, df = sim.frames.jaco_frame(ee), pl["dofs"]
        xg2, pg2, w2 = goals(sim, q2, v2, df, qa, P)
        rest = {k_: v_ for k_, v_ in pl.items() if k_ != "ctrl"}
        cost = lambda sim=sim, pl=pl, q2=q2, v2=v2, rest=rest, fr=fr, xg2=xg2, pg2=pg2, w2=w2: sim.rollout_cost(
            pl["ctrl"], q2, v2, **rest, frame=fr, x_goal=xg2, p_goal=pg2, want=("cost", "status"), **fan, **w2)
        closed = lambda sim=sim, pl=pl, q2=q2, v2=v2, rest=rest, fr=fr: sim.rollout_feedback(pl["ctrl"], q2, v2, **rest, frame=fr, **fan)

        def replaced(sim=sim, closed=closed, df=df, qa=qa, xg2=xg2, pg2=pg2):
            r = closed()
            return torch_cost(r, r["ctrl"], df, qa, fl, xg2, pg2, sim.nu)
        legs.update({tag + "_cost_ms": cost, tag + "_replaced_ms": replaced, tag + "_closed_ms": closed})
        a, b = cost(), replaced()
        checks[tag] = (float(((a["cost"] - b).abs() / b).max()), int(a["status"].cpu().numpy().view(np.uint32).max()))
        del a, b
        peaks.update({tag + "_cost_MiB": peak(cost), tag + "_replaced_MiB": peak(replaced)})

    res = {"states": S, "samples": K, "plans": P, "alphas": A, "rollouts": [S * K, P * A], "knots": T, "hold": 1, "iters": args.iters, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "cost_max_rel_diff_vs_torch": {k: v[0] for k, v in checks.items()},
           "status_or": {k: v[1] for k, v in checks.items()}, "peak_MiB_above_inputs": peaks}
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, fn in legs.items():
            runs[k].append(timed(fn, args.iters))
    for k in legs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    res["replaced_over_cost"] = {t: med(t + "_replaced_ms") / med(t + "_cost_ms") for t in ("s", "l", "d")}
    res["cost_over_rollout_alone"] = {"s": med("s_cost_ms") / med("s_open_ms"), "l": med("l_cost_ms") / med("l_closed_ms"), "d": med("d_cost_ms") / med("d_closed_ms")}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("== python tools/gpu_rollout_cost_bench.py --states %d --samples %d --plans %d --alphas %d --knots %d --iters %d --repeats %d\n"
                % (S, K, P, A, T, args.iters, args.repeats))
        f.write(json.dumps(res) + "\n")
    for s in (one, two):
        s.close()


if __name__ == "__main__":
    main()
