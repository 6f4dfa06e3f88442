"""Device time of the batched inverse kinematics (jaco_ik) at 65 536 envs on the default model, next to what a user had before it.

Seeds: picking reset states.  Targets: the EE pose (query kernel) of the seed with the six arm angles moved by uniform +-s and clamped to
their ranges; near set s = 0.3, far set s = 1.0; pose targets (position + orientation).
  (a) jaco_ik per call, and its mean iteration count
  (b) the mean iteration count (and that + 1: the kernel evaluates the pose once more than it steps) times one sim.query call for xpos,
      xmat, jac only -- the same tree walk per iteration with the Jacobian's trip through HBM
  (c) the same algorithm in torch on sim.query + torch.linalg.solve, stopping when every env has converged or at max_iters: what a user
      did before jaco_ik
Times: HIP events on the current stream around N back-to-back calls (after warm-up), mean per call.  One JSON line per target set, also
appended to --out (default profiles/ik_bench.txt).
usage: python tools/gpu_ik_bench.py [--envs 65536] [--iters 50] [--torch-iters 5] [--out profiles/ik_bench.txt]
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
from mujoco_jaco_amd.robot_config import mat2quat  # noqa: E402

OPT = _lib.JacoIkOptions.DEFAULTS


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def quat2mat(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1).reshape(-1, 3, 3)


def torch_ik(sim, frame, arm, dofs, lo, hi, limited, seed, tp, tq):
    """The algorithm of include/jaco_env.h ("inverse kinematics") on sim.query: (qpos, converged, iterations run)."""
    q = seed.clone()
    Rt = quat2mat(tq)
    eye = (OPT["damping"] ** 2) * torch.eye(6, device=q.device)
    k = 0
    while True:
        r = sim.query([frame], qpos=q, qM=False, qfrc_bias=False)
        R = r["xmat"][:, 0].reshape(-1, 3, 3)
        ep = tp - r["xpos"][:, 0]
        E = Rt @ R.transpose(1, 2)
        a = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
        sn = a.norm(dim=1)
        ang = torch.atan2(sn, 0.5 * (E.diagonal(dim1=1, dim2=2).sum(1) - 1.0))
        er = a * (ang / sn.clamp_min(1e-20))[:, None]
        done = (ep.norm(dim=1) < OPT["tol_pos"]) & (er.norm(dim=1) < OPT["tol_rot"])
        if k == OPT["max_iters"] or bool(done.all()):
            return q, done, k
        J = r["jac"][:, 0][:, :, dofs]
        y = torch.linalg.solve(J @ J.transpose(1, 2) + eye, torch.cat([ep, er], 1)[:, :, None])
        dq = (J.transpose(1, 2) @ y)[:, :, 0]
        mx = dq.abs().max(dim=1, keepdim=True).values
        dq = dq * torch.where(mx > OPT["max_step"], OPT["max_step"] / mx, torch.ones_like(mx))
        qa = q[:, arm] + torch.where(done[:, None], torch.zeros_like(dq), dq)
        q[:, arm] = torch.where(limited, torch.minimum(torch.maximum(qa, lo), hi), qa)
        k += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_bench.txt"))
    args = ap.parse_args()
    B, dev = args.envs, "cuda:0"
    sim = BatchedMujoco(B)
    M = blob.load(_lib.model_path("jaco2_curtain_torque"))
    seed = torch.tensor(workload.reset_states(M["qpos0"], B, seed=3, f32_draws=True), dtype=torch.float32, device=dev)
    frame = sim.frames.jaco_frame("EE", point=[0.0, 0.0, 0.0])
    arm, dofs = sim.frames.chain("EE")   # qpos and dof addresses of the six arm joints
    rng_ = torch.tensor(M["f_range"].reshape(-1, 2)[:6], dtype=torch.float32, device=dev)
    limited = torch.tensor(M["f_limited"][:6] != 0, device=dev)[None, :]
    lo, hi = rng_[None, :, 0], rng_[None, :, 1]
    lines = ["== python tools/gpu_ik_bench.py --envs %d --iters %d --torch-iters %d" % (B, args.iters, args.torch_iters)]
    for name, s in (("near", 0.3), ("far", 1.0)):
        g = seed.clone()
        ga = g[:, arm] + torch.tensor(np.random.default_rng(11).uniform(-s, s, (B, 6)), dtype=torch.float32, device=dev)
        g[:, arm] = torch.where(limited, torch.minimum(torch.maximum(ga, lo), hi), ga)
        t = sim.query([frame], qpos=g, jac=False, qM=False, qfrc_bias=False)
        tp, tq = t["xpos"][:, 0].contiguous(), mat2quat(t["xmat"][:, 0]).contiguous()
        r = sim.ik(frame, tp, tq, seed)
        it = r["iters"].float()
        res = {"set": name, "s": s, "envs": B, "calls": args.iters, "device": torch.cuda.get_device_name(0),
               "converged": int(r["converged"].sum()), "mean_iters": float(it.mean()), "max_iters_taken": int(it.max())}
        res["a_jaco_ik_ms"] = timed(lambda: sim.ik(frame, tp, tq, seed), args.iters)
        q_ms = timed(lambda: sim.query([frame], qpos=seed, qM=False, qfrc_bias=False), args.iters)
        res["query_xpos_xmat_jac_ms"] = q_ms
        res["b_mean_iters_x_query_ms"] = res["mean_iters"] * q_ms
        res["b_mean_iters_plus_1_x_query_ms"] = (res["mean_iters"] + 1.0) * q_ms
        qt, ct, kt = torch_ik(sim, frame, arm, dofs, lo, hi, limited, seed, tp, tq)
        res["c_torch_iterations_run"], res["c_torch_converged"] = kt, int(ct.sum())
        res["c_torch_calls"] = args.torch_iters
        res["c_torch_ik_ms"] = timed(lambda: torch_ik(sim, frame, arm, dofs, lo, hi, limited, seed, tp, tq), args.torch_iters, warmup=1)
        res["a_over_b"] = res["a_jaco_ik_ms"] / res["b_mean_iters_x_query_ms"]
        res["c_over_a"] = res["c_torch_ik_ms"] / res["a_jaco_ik_ms"]
        res["max_dq_vs_torch_on_common_converged"] = float((r["qpos"] - qt).abs()[(r["converged"] & ct)].max())
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
