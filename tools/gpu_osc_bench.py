"""Device time of the batched operational-space controller (jaco_osc) at 65 536 envs, next to what a user had before it.

States: picking reset states with qvel uniform in +-0.5.  Targets: each controlled frame's pose (query kernel) of the state with the
arm angles moved by uniform +-0.3.  Two configurations: the default model with one frame (EE), the two-arm model with two (EE_1 + EE_2).
  (a) jaco_osc per call (one launch)
  (b) the same formula in torch on sim.query outputs (xpos, xmat, jac, qM, qfrc_bias): what a user wrote before jaco_osc -- abr_control's
      plain-inverse branch only (no determinant test, no pseudo-inverse), so (b) does less than (a)
Times: HIP events on the current stream around N back-to-back calls (after warm-up), mean per call.  One JSON line per configuration,
also written to --out (default profiles/osc_bench.txt).
usage: python tools/gpu_osc_bench.py [--envs 65536] [--iters 50] [--torch-iters 10] [--out profiles/osc_bench.txt]
--task: the same two yardsticks for jaco_osc_task on the default model, position only with Damping(10) and RestingConfig(20, 5) on every
arm joint: (a) jaco_osc_task per call, next to jaco_osc in the same run; (b) the same formula in torch on sim.query outputs (the plain
inverse of the 3 x 3 matrix, the null-space terms and the n x n filter).  Written to profiles/osc_task_bench.txt.
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

OPT = _lib.JacoOscOptions.DEFAULTS


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


def torch_osc(sim, frames, dofs, qpos, qvel, tp, tq):
    """u [B, nf, 6] of the formula of include/jaco_env.h ("operational-space controller"), regular branch, on one sim.query call."""
    r = sim.query(frames, qpos=qpos, qvel=qvel)
    out = []
    for f, d in enumerate(dofs):
        J = r["jac"][:, f][:, :, d]
        M = r["qM"][:, d][:, :, d]
        Mx = torch.linalg.inv(J @ torch.linalg.solve(M, J.transpose(1, 2)))
        qe = mat2quat(r["xmat"][:, f])
        qd = tq[:, f]
        w = qd[:, 0] * qe[:, 0] + (qd[:, 1:] * qe[:, 1:]).sum(1)
        vec = -qd[:, :1] * qe[:, 1:] + qe[:, :1] * qd[:, 1:] - torch.linalg.cross(qd[:, 1:], qe[:, 1:])
        ut = torch.cat([r["xpos"][:, f] - tp[:, f], -vec * torch.sign(w)[:, None]], 1)
        sat = (OPT["vmax_xyz"] / OPT["kp"] * OPT["kv"], OPT["vmax_abg"] / OPT["ko"] * OPT["kv"])
        nx, na = ut[:, :3].norm(dim=1, keepdim=True), ut[:, 3:].norm(dim=1, keepdim=True)
        sx = torch.where(nx > sat[0], sat[0] / nx, torch.ones_like(nx)) * OPT["kp"]
        sa = torch.where(na > sat[1], sat[1] / na, torch.ones_like(na)) * OPT["ko"]
        ut = torch.cat([ut[:, :3] * sx, ut[:, 3:] * sa], 1)
        u = -OPT["kv"] * (M @ qvel[:, d, None])[:, :, 0] - (J.transpose(1, 2) @ (Mx @ ut[:, :, None]))[:, :, 0] + r["qfrc_bias"][:, d]
        out.append(u)
    return torch.stack(out, 1)


def torch_osc_task(sim, frame, d, qa, qpos, qvel, tp, rest, null_kv=10.0, rest_kp=20.0, rest_kv=5.0):
    """u [B, n] of the formula of include/jaco_env.h (jaco_osc_task), position only, both null-space terms, regular branch."""
    r = sim.query([frame], qpos=qpos, qvel=qvel)
    J = r["jac"][:, 0][:, :3, d]
    M = r["qM"][:, d][:, :, d]
    dq = qvel[:, d, None]
    MiJt = torch.linalg.solve(M, J.transpose(1, 2))
    Mx = torch.linalg.inv(J @ MiJt)
    ut = r["xpos"][:, 0] - tp[:, 0]
    sat = OPT["vmax_xyz"] / OPT["kp"] * OPT["kv"]
    nx = ut.norm(dim=1, keepdim=True)
    ut = ut * torch.where(nx > sat, sat / nx, torch.ones_like(nx)) * OPT["kp"]
    u = -OPT["kv"] * (M @ dq) - J.transpose(1, 2) @ (Mx @ ut[:, :, None]) + r["qfrc_bias"][:, d, None]
    e = torch.remainder(rest[:, qa] - qpos[:, qa] + np.pi, 2 * np.pi) - np.pi
    un = -null_kv * (M @ dq) + M @ (rest_kp * e[:, :, None] - rest_kv * dq)
    Jbar = MiJt @ Mx
    return (u + un - J.transpose(1, 2) @ (Jbar.transpose(1, 2) @ un))[:, :, 0]


def task_leg(args):
    """jaco_osc_task (position only, both null-space terms) against jaco_osc and against torch on sim.query, default model."""
    B, dev, model = args.envs, "cuda:0", "jaco2_curtain_torque"
    sim = BatchedMujoco(B, robot_file=model)
    M = blob.load(_lib.model_path(model))
    qpos = torch.tensor(workload.reset_states(M["qpos0"], B, seed=3, f32_draws=True), dtype=torch.float32, device=dev)
    qvel = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (B, sim.nv)), dtype=torch.float32, device=dev)
    frame = sim.frames.jaco_frame("EE")
    qa, d = sim.frames.chain("EE")
    g = qpos.clone()
    g[:, qa] += torch.tensor(np.random.default_rng(11).uniform(-0.3, 0.3, (B, len(qa))), dtype=torch.float32, device=dev)
    t = sim.query([frame], qpos=g, qM=False, qfrc_bias=False)
    tp = (t["xpos"] + (t["xmat"].reshape(B, -1, 3, 3) @ torch.tensor(frame.point[:], device=dev)[None, None, :, None])[..., 0]).contiguous()
    tq = mat2quat(t["xmat"]).contiguous()
    rest = qpos.clone()
    rest[:, qa] += torch.tensor(np.random.default_rng(17).uniform(-1, 1, (B, len(qa))), dtype=torch.float32, device=dev)
    task = dict(axes=0b000111, null_kv=10.0, rest_qpos=rest, rest_kp=20.0, rest_kv=5.0)
    r = sim.osc([frame], tp, None, qpos, qvel, **task)
    ut = torch_osc_task(sim, frame, d, qa, qpos, qvel, tp, rest)
    reg = ~r["singular"].any(1)
    diff = (r["ctrl"][:, d] - ut).abs() / (1.0 + ut.abs())   # (this model: the motor of arm dof d is actuator d)
    res = {"model": model, "frames": ["EE"], "task": "axes 0b000111, null_kv 10, rest_kp 20, rest_kv 5, rest_mask 0", "envs": B, "calls": args.iters,
           "device": torch.cuda.get_device_name(0), "pseudo_inverse_envs": int((~reg).sum()), "max_rel_diff_vs_torch_on_regular_envs": float(diff[reg].max())}
    res["a_jaco_osc_task_ms"] = timed(lambda: sim.osc([frame], tp, None, qpos, qvel, **task), args.iters)
    res["jaco_osc_ms"] = timed(lambda: sim.osc([frame], tp, tq, qpos, qvel), args.iters)
    res["a_jaco_osc_task_ms_again"] = timed(lambda: sim.osc([frame], tp, None, qpos, qvel, **task), args.iters)
    res["task_over_jaco_osc"] = res["a_jaco_osc_task_ms"] / res["jaco_osc_ms"]
    res["query_all_outputs_ms"] = timed(lambda: sim.query([frame], qpos=qpos, qvel=qvel), args.iters)
    res["b_torch_calls"] = args.torch_iters
    res["b_torch_osc_task_ms"] = timed(lambda: torch_osc_task(sim, frame, d, qa, qpos, qvel, tp, rest), args.torch_iters, warmup=2)
    res["b_over_a"] = res["b_torch_osc_task_ms"] / res["a_jaco_osc_task_ms"]
    print(json.dumps(res), flush=True)
    sim.close()
    out = args.out or os.path.join(ROOT, "profiles", "osc_task_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("== python tools/gpu_osc_bench.py --task --envs %d --iters %d --torch-iters %d\n%s\n" % (B, args.iters, args.torch_iters, json.dumps(res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--torch-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--task", action="store_true")
    args = ap.parse_args()
    if args.task:
        return task_leg(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "osc_bench.txt")
    B, dev = args.envs, "cuda:0"
    lines = ["== python tools/gpu_osc_bench.py --envs %d --iters %d --torch-iters %d" % (B, args.iters, args.torch_iters)]
    for model, names in (("jaco2_curtain_torque", ("EE",)), ("jaco2_dual_torque", ("EE_1", "EE_2"))):
        sim = BatchedMujoco(B, robot_file=model)
        M = blob.load(_lib.model_path(model))
        reset = workload.reset_states_dual if len(names) == 2 else (lambda q0, n, seed: workload.reset_states(q0, n, seed=seed, f32_draws=True))
        qpos = torch.tensor(reset(M["qpos0"], B, seed=3), dtype=torch.float32, device=dev)
        qvel = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (B, sim.nv)), dtype=torch.float32, device=dev)
        frames = [sim.frames.jaco_frame(n) for n in names]
        chains = [sim.frames.chain(n) for n in names]
        g = qpos.clone()
        for qa, _ in chains:
            g[:, qa] += torch.tensor(np.random.default_rng(11).uniform(-0.3, 0.3, (B, len(qa))), dtype=torch.float32, device=dev)
        t = sim.query(frames, qpos=g, qM=False, qfrc_bias=False)
        tp = (t["xpos"] + (t["xmat"].reshape(B, -1, 3, 3) @ torch.stack([torch.tensor(f.point[:], device=dev) for f in frames])[None, :, :, None])[..., 0]).contiguous()
        tq = mat2quat(t["xmat"]).contiguous()
        dofs = [c[1] for c in chains]
        r = sim.osc(frames, tp, tq, qpos, qvel)
        ut = torch_osc(sim, frames, dofs, qpos, qvel, tp, tq)
        reg = ~r["singular"].any(1)
        motors = torch.tensor([d for c in dofs for d in c], device=dev)   # (these models: the motor of arm dof d is actuator d)
        diff = (r["ctrl"][:, motors] - ut.reshape(B, -1)).abs() / (1.0 + ut.reshape(B, -1).abs())
        res = {"model": model, "frames": list(names), "envs": B, "calls": args.iters, "device": torch.cuda.get_device_name(0),
               "pseudo_inverse_envs": int((~reg).sum()), "max_rel_diff_vs_torch_on_regular_envs": float(diff[reg].max())}
        res["a_jaco_osc_ms"] = timed(lambda: sim.osc(frames, tp, tq, qpos, qvel), args.iters)
        res["query_all_outputs_ms"] = timed(lambda: sim.query(frames, qpos=qpos, qvel=qvel), args.iters)
        res["b_torch_calls"] = args.torch_iters
        res["b_torch_osc_ms"] = timed(lambda: torch_osc(sim, frames, dofs, qpos, qvel, tp, tq), args.torch_iters, warmup=2)
        res["b_over_a"] = res["b_torch_osc_ms"] / res["a_jaco_osc_ms"]
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        sim.close()
        del sim
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
