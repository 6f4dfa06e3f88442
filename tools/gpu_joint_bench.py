"""Device time of the batched joint-space controller (jaco_joint) at 65 536 envs, next to jaco_osc and to what a user had before it.

States: picking reset states with qvel uniform in +-0.5.  Joint targets: the state's motor-driven joints moved by uniform +-1 rad, target
velocities +-0.5, feed-forward accelerations +-2; gains kp 50, kv 20, vmax 0.5 (so the wave reduction of the velocity limit runs).  Two
configurations: the default model (6 active dofs), the two-arm model (12 active dofs in one call).
  (a) jaco_joint per call (one launch)
  (o) jaco_osc per call in the same run (one frame; two on the two-arm model): the same forward pass plus the 6 x 6 solves
  (b) the same formula in torch on sim.query's qM and qfrc_bias (no frames asked for): what a user wrote before jaco_joint
Times: HIP events on the current stream around N back-to-back calls after warm-up, mean per call; the three legs alternate --repeats times
and every repeat is reported (min / median / max), so that the spread is seen next to the differences.  One JSON line per configuration,
also written to --out (default profiles/joint_bench.txt).
usage: python tools/gpu_joint_bench.py [--envs 65536] [--iters 200] [--torch-iters 20] [--repeats 3] [--out profiles/joint_bench.txt]
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
from mujoco_jaco_amd.robot_config import BatchedJoint, BatchedMujocoConfig, mat2quat  # noqa: E402

GAINS = dict(kp=50.0, kv=20.0, vmax=0.5)


def timed(fn, iters, warmup=5):
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


def torch_joint(sim, d, qa, wrap, qpos, qvel, t, tv, ff):
    """u [B, n] of the formula of include/jaco_env.h ("joint-space controller") on one sim.query call (qM and qfrc_bias only)."""
    r = sim.query([], qpos=qpos, qvel=qvel, xpos=False, xmat=False, jac=False)
    M = r["qM"][:, d][:, :, d]
    x = t[:, qa] - qpos[:, qa]
    e = torch.where(wrap, torch.remainder(x + np.pi, 2 * np.pi) - np.pi, x)
    sat = GAINS["vmax"] * GAINS["kv"] / GAINS["kp"]
    s = torch.clamp(sat / e.abs().amax(1, keepdim=True), max=1.0)
    a = ff[:, d] + GAINS["kp"] * s * e + GAINS["kv"] * (tv[:, d] - qvel[:, d])
    return (M @ a[:, :, None])[:, :, 0] + r["qfrc_bias"][:, d]


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_bench.txt"))
    args = ap.parse_args()
    B, dev = args.envs, "cuda:0"
    lines = ["== python tools/gpu_joint_bench.py --envs %d --iters %d --torch-iters %d --repeats %d" % (B, args.iters, args.torch_iters, args.repeats)]
    for model, names in (("jaco2_curtain_torque", ("EE",)), ("jaco2_dual_torque", ("EE_1", "EE_2"))):
        sim = BatchedMujoco(B, robot_file=model)
        M = blob.load(_lib.model_path(model))
        reset = workload.reset_states_dual if len(names) == 2 else (lambda q0, n, seed: workload.reset_states(q0, n, seed=seed, f32_draws=True))
        qpos = torch.tensor(reset(M["qpos0"], B, seed=3), dtype=torch.float32, device=dev)
        rnd = lambda seed, s, n: torch.tensor(np.random.default_rng(seed).uniform(-s, s, (B, n)), dtype=torch.float32, device=dev)
        qvel = rnd(5, 0.5, sim.nv)
        ctl = BatchedJoint(BatchedMujocoConfig(sim, ee=names[0]))   # (the joint tables: every motor-driven hinge, in dof order)
        qa, d = ctl.qadr, ctl.dadr
        limited = {int(M["jnt_dofadr"][j]): bool(M["jnt_limited"][j]) for j in range(len(M["jnt_dofadr"]))}
        wrap = torch.tensor([not limited[k] for k in d], device=dev)[None, :]
        t = qpos.clone()
        t[:, qa] += rnd(13, 1.0, len(qa))
        tv, ff = rnd(14, 0.5, sim.nv), rnd(15, 2.0, sim.nv)
        # the operational-space controller's inputs, as tools/gpu_osc_bench.py draws them
        frames = [sim.frames.jaco_frame(n) for n in names]
        g = qpos.clone()
        for n in names:
            ca = sim.frames.chain(n)[0]
            g[:, ca] += rnd(11, 0.3, len(ca))
        p = sim.query(frames, qpos=g, qM=False, qfrc_bias=False)
        tp = (p["xpos"] + (p["xmat"].reshape(B, -1, 3, 3) @ torch.stack([torch.tensor(f.point[:], device=dev) for f in frames])[None, :, :, None])[..., 0]).contiguous()
        tq = mat2quat(p["xmat"]).contiguous()
        legs = {
            "a_jaco_joint_ms": (lambda: sim.joint(t, tv, ff, qpos, qvel, **GAINS), args.iters),
            "o_jaco_osc_ms": (lambda: sim.osc(frames, tp, tq, qpos, qvel), args.iters),
            "query_qM_bias_ms": (lambda: sim.query([], qpos=qpos, qvel=qvel, xpos=False, xmat=False, jac=False), args.iters),
            "b_torch_joint_ms": (lambda: torch_joint(sim, d, qa, wrap, qpos, qvel, t, tv, ff), args.torch_iters),
        }
        u = sim.joint(t, tv, ff, qpos, qvel, **GAINS)
        ut = torch_joint(sim, d, qa, wrap, qpos, qvel, t, tv, ff)
        motors = torch.tensor(d, device=dev)   # (these models: the motor of arm dof d is actuator d)
        diff = (u[:, motors] - ut).abs() / (1.0 + ut.abs())
        res = {"model": model, "active_dofs": len(d), "osc_frames": list(names), "envs": B, "calls": args.iters, "torch_calls": args.torch_iters,
               "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "max_rel_diff_vs_torch": float(diff.max())}
        runs = {k: [] for k in legs}
        for _ in range(args.repeats):   # the legs alternate
            for k, (fn, n) in legs.items():
                runs[k].append(timed(fn, n))
        for k in legs:
            res[k] = stats(runs[k])
        res["joint_over_osc"] = res["a_jaco_joint_ms"]["median"] / res["o_jaco_osc_ms"]["median"]
        res["b_over_a"] = res["b_torch_joint_ms"]["median"] / res["a_jaco_joint_ms"]["median"]
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
