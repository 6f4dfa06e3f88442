"""Device time of one batched backward pass (jaco_lqr) next to the torch loop it replaces, and next to the forward pass it feeds.

4 096 problems x 50 knots at (nx, nu) = (18, 6) and (36, 12), drawn on the device with the [q, dq] structure of one substep that
tests/lqr_binding.py uses (h = 0.002; S, D, G uniform as there; lxx = diag(100 .., 1 ..), luu = 1e-3 I, Vxx = 10 lxx, gradients uniform).
Per shape:
  (k) jaco_lqr, every output: ONE lqr_backward call with lx, lu, Vx                (K, k, dV, Vxx0, Vx0)
  (K) jaco_lqr, gains only: robot_config.lqr's call (no gradients, gain alone)
  (g) robot_config.lqr_gains in fp32 on the device: the torch loop that (K) replaces
  (f) the same loop extended with the k / dV / Vx terms: the torch loop that (k) replaces
and once, at the same plan count:
  (r) jaco_rollout_fb: 4 096 plans x 50 knots x hold 1 on the default model, gains over its 9 hinge dofs (tools/gpu_rollout_fb_bench.py's
      plans, one rollout per plan) -- the forward pass of the same iLQR iteration.
(k)'s K is compared with (f)'s in the same run.  Everything below is MEASURED in this run: HIP events on the current stream around N
back-to-back repetitions after warm-up, mean per repetition; the legs alternate --repeats times and every repeat is reported (min /
median / max).  One JSON line, also written to --out (default profiles/lqr_bench.txt), with the commit it was measured on.
usage: python tools/gpu_lqr_bench.py [--problems 4096] [--knots 50] [--iters 10] [--loop-iters 2] [--repeats 3] [--commit ID] [--out ...]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mujoco_jaco_amd.physics import BatchedMujoco  # noqa: E402
from mujoco_jaco_amd.robot_config import lqr_gains  # noqa: E402
from tools.gpu_rollout_bench import stats, timed  # noqa: E402
from tools.gpu_rollout_fb_bench import problem  # noqa: E402

H = 0.002


def draw(P, T, nx, nu, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    U = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g, device=dev)
    nd = nx // 2
    I = torch.eye(nd, device=dev)
    S = U(-5, 5, P, T, nd, nd) - U(0, 50, P, T, nd)[..., None] * I
    D = U(-0.2, 0.2, P, T, nd, nd) - U(0.5, 5, P, T, nd)[..., None] * I
    G = U(-1, 1, P, T, nd, nu)
    G[..., :nu, :] += U(2, 20, P, T, nu)[..., None] * torch.eye(nu, device=dev)
    A = torch.cat([torch.cat([I + H * H * S, H * (I + H * D)], -1), torch.cat([H * S, I + H * D], -1)], -2).contiguous()
    B = torch.cat([H * H * G, H * G], -2).contiguous()
    w = torch.tensor([100.0] * nd + [1.0] * nd, device=dev)
    return dict(A=A, B=B, lxx=torch.diag(w), luu=1e-3 * torch.eye(nu, device=dev), lx=U(-1, 1, P, T, nx), lu=1e-3 * U(-1, 1, P, T, nu), Vxx=10 * torch.diag(w),
                Vx=U(-1, 1, P, nx))


def full_loop(A, B, Q, R, Qf, lx, lu, Vx):
    """lqr_gains' loop with the feed-forward, the expected cost change and the value gradient: what jaco_lqr computes, in batched torch."""
    T = A.shape[1]
    P_, p = Qf, Vx
    Ks, ks = [], []
    dV = torch.zeros(A.shape[0], 2, dtype=A.dtype, device=A.device)
    for t in range(T - 1, -1, -1):
        At, Bt = A[:, t], B[:, t]
        BtP = Bt.transpose(-1, -2) @ P_
        Quu, Qux = R + BtP @ Bt, BtP @ At
        Qu = lu[:, t] + (Bt.transpose(-1, -2) @ p[:, :, None])[:, :, 0]
        Qx = lx[:, t] + (At.transpose(-1, -2) @ p[:, :, None])[:, :, 0]
        sol = -torch.linalg.solve(Quu, torch.cat([Qux, Qu[:, :, None]], 2))
        Kt, kt = sol[:, :, :-1], sol[:, :, -1]
        dV[:, 0] += (kt * Qu).sum(1)
        dV[:, 1] += 0.5 * (kt * (Quu @ kt[:, :, None])[:, :, 0]).sum(1)
        p = Qx + (Kt.transpose(-1, -2) @ ((Quu @ kt[:, :, None])[:, :, 0] + Qu)[:, :, None])[:, :, 0] + (Qux.transpose(-1, -2) @ kt[:, :, None])[:, :, 0]
        P_ = Q + At.transpose(-1, -2) @ P_ @ (At + Bt @ Kt)
        P_ = 0.5 * (P_ + P_.transpose(-1, -2))
        Ks.append(Kt)
        ks.append(kt)
    return torch.stack(Ks[::-1], 1), torch.stack(ks[::-1], 1), dV


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (no git metadata next to the sources)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)        # kernel calls per timed window
    ap.add_argument("--loop-iters", type=int, default=2)    # repetitions of the torch loop per timed window
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lqr_bench.txt"))
    args = ap.parse_args()
    P, T, dev, model = args.problems, args.knots, "cuda:0", "jaco2_curtain_torque"
    sim = BatchedMujoco(2, robot_file=model)
    res = {"problems": P, "knots": T, "iters": args.iters, "loop_iters": args.loop_iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "commit": args.commit or commit(), "measured": "every *_ms entry and every ratio below: HIP events, this run"}
    legs = {}
    for nx, nu in ((18, 6), (36, 12)):
        g = draw(P, T, nx, nu, dev, 100 + nx)
        tag = "%dx%d" % (nx, nu)
        outs = {k: torch.empty(s, device=dev) for k, s in (("gain", (P, T, nu, nx)), ("kff", (P, T, nu)), ("dV", (P, 2)), ("Vxx0", (P, nx, nx)), ("Vx0", (P, nx)))}
        outs["status"] = torch.zeros(P, dtype=torch.int32, device=dev)
        gains_only = dict(gain=outs["gain"], kff=None, dV=None, Vxx0=None, Vx0=None, status=outs["status"])
        every = lambda g=g, outs=outs: sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], lx=g["lx"], lu=g["lu"], Vxx=g["Vxx"], Vx=g["Vx"], out=outs)
        only = lambda g=g, o=gains_only: sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], Vxx=g["Vxx"], out=o)
        loop_g = lambda g=g: lqr_gains(g["A"], g["B"], g["lxx"], g["luu"], g["Vxx"])
        loop_f = lambda g=g: full_loop(g["A"], g["B"], g["lxx"], g["luu"], g["Vxx"], g["lx"], g["lu"], g["Vx"])
        r = every()
        Kl, kl, dVl = loop_f()
        rel = lambda a, b: float((a - b).abs().amax() / b.abs().amax())
        res[tag] = {"status_or": int(r["status"].cpu().numpy().view("uint32").max()), "K_vs_torch_loop": rel(r["gain"], Kl), "k_vs_torch_loop": rel(r["kff"], kl),
                    "dV_vs_torch_loop": rel(r["dV"], dVl)}
        del Kl, kl, dVl
        legs.update({tag + "_k_jaco_lqr_ms": (every, args.iters), tag + "_K_jaco_lqr_gains_only_ms": (only, args.iters),
                     tag + "_g_lqr_gains_torch_ms": (loop_g, args.loop_iters), tag + "_f_full_torch_loop_ms": (loop_f, args.loop_iters)})
    qpos, qvel, plan, _ = problem(model, sim, P, T, dev, 7)
    frame = sim.frames.jaco_frame("EE")
    legs["r_jaco_rollout_fb_ms"] = (lambda: sim.rollout_feedback(plan["ctrl"], qpos, qvel, **{k: v for k, v in plan.items() if k != "ctrl"}, frame=frame), args.iters)
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, (fn, iters) in legs.items():
            runs[k].append(timed(fn, iters))
    for k in legs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    for tag in ("18x6", "36x12"):
        res[tag + "_torch_loop_over_jaco_lqr"] = med(tag + "_f_full_torch_loop_ms") / med(tag + "_k_jaco_lqr_ms")
        res[tag + "_lqr_gains_over_jaco_lqr_gains_only"] = med(tag + "_g_lqr_gains_torch_ms") / med(tag + "_K_jaco_lqr_gains_only_ms")
        res[tag + "_backward_over_forward"] = med(tag + "_k_jaco_lqr_ms") / med("r_jaco_rollout_fb_ms")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_lqr_bench.py --problems %d --knots %d --iters %d --loop-iters %d --repeats %d\n" % (P, T, args.iters, args.loop_iters, args.repeats))
        f.write(json.dumps(res) + "\n")
    sim.close()


if __name__ == "__main__":
    main()
