"""Device time of batched forward dynamics and its linearisation (jaco_fd) at 65 536 envs, next to jaco_joint and to what a user had before it.

States: picking reset states with qvel uniform in +-0.5; ctrl: motor commands uniform in +-5, finger servo commands = the finger angle.
Two configurations: the default model (9 hinge dofs perturbed: 37 forward passes per env in the full linearisation), the two-arm model
(18 hinge dofs: 73 passes).
  (a) jaco_fd, qacc only, per call (one launch)
  (j) jaco_joint per call in the same run: the same forward pass and no solve
  (l) jaco_fd, the full linearisation (qacc, dqacc_dqpos, dqacc_dqvel, dqacc_dctrl; default steps, implicit damping) per call
  (b) qacc only in torch on sim.query's qM and qfrc_bias (torch.linalg.solve; motors only, no actuator model): what a user wrote before
The condition of DESIGN.md section 6: (l) must take less time than the 1 + 2 * 2 * (selected dofs) qacc-only calls it replaces, (a) times
that count, measured in the same run.
Times: HIP events on the current stream around N back-to-back calls after warm-up, mean per call; the legs alternate --repeats times and
every repeat is reported (min / median / max).  One JSON line per configuration, also written to --out (default profiles/fd_bench.txt).
usage: python tools/gpu_fd_bench.py [--envs 65536] [--iters 200] [--lin-iters 20] [--torch-iters 20] [--repeats 3] [--out profiles/fd_bench.txt]
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


def torch_qacc(sim, qpos, qvel, frc):
    """qacc [B, nv] = qM^-1 (frc - qfrc_bias) on one sim.query call (qM and qfrc_bias only); frc [B, nv]: the applied joint forces."""
    r = sim.query([], qpos=qpos, qvel=qvel, xpos=False, xmat=False, jac=False)
    return torch.linalg.solve(r["qM"], (frc - r["qfrc_bias"])[:, :, None])[:, :, 0]


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lin-iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fd_bench.txt"))
    args = ap.parse_args()
    B, dev = args.envs, "cuda:0"
    lines = ["== python tools/gpu_fd_bench.py --envs %d --iters %d --lin-iters %d --torch-iters %d --repeats %d" % (B, args.iters, args.lin_iters, args.torch_iters, args.repeats)]
    for model in ("jaco2_curtain_torque", "jaco2_dual_torque"):
        sim = BatchedMujoco(B, robot_file=model)
        M = blob.load(_lib.model_path(model))
        dual = int(M["nq"][0]) >= 32
        reset = workload.reset_states_dual if dual else (lambda q0, n, seed: workload.reset_states(q0, n, seed=seed, f32_draws=True))
        qpos = torch.tensor(reset(M["qpos0"], B, seed=3), dtype=torch.float32, device=dev)
        rnd = lambda seed, s, n: torch.tensor(np.random.default_rng(seed).uniform(-s, s, (B, n)), dtype=torch.float32, device=dev)
        qvel = rnd(5, 0.5, sim.nv)
        ctrl = rnd(7, 5.0, sim.nu)
        servo = [a for a in range(sim.nu) if M["actuator_position"][a]]
        motor = [a for a in range(sim.nu) if not M["actuator_position"][a]]
        adof = [int(M["jnt_dofadr"][int(j)]) for j in M["actuator_jntid"]]
        aqadr = [int(M["jnt_qposadr"][int(j)]) for j in M["actuator_jntid"]]
        ctrl[:, servo] = qpos[:, [aqadr[a] for a in servo]]   # the servos hold their joints: no actuator force there
        hinge = [int(M["jnt_dofadr"][j]) for j in range(int(M["njnt"][0])) if int(M["jnt_type"][j]) == 3]
        calls_replaced = 1 + 2 * 2 * len(hinge)
        frc = torch.zeros(B, sim.nv, device=dev)
        frc[:, [adof[a] for a in motor]] = ctrl[:, motor]
        damp = torch.tensor(np.asarray(M["dof_damping"], np.float32), device=dev)
        frc = frc - damp * qvel                                # the passive term, so that (b) computes the same number
        t = qpos.clone()
        legs = {
            "a_fd_qacc_ms": (lambda: sim.forward_dynamics(ctrl, qpos, qvel), args.iters),
            "j_jaco_joint_ms": (lambda: sim.joint(t, None, None, qpos, qvel), args.iters),
            "l_fd_linearize_ms": (lambda: sim.linearize(ctrl, qpos, qvel), args.lin_iters),
            "b_torch_qacc_ms": (lambda: torch_qacc(sim, qpos, qvel, frc), args.torch_iters),
        }
        a = sim.forward_dynamics(ctrl, qpos, qvel)
        bt = torch_qacc(sim, qpos, qvel, frc)
        diff = ((a - bt).abs() / (1.0 + bt.abs()))[:, hinge[:6]]   # (the arm's dofs: no clamp is active on them at these commands)
        res = {"model": model, "hinge_dofs": len(hinge), "envs": B, "calls": args.iters, "lin_calls": args.lin_iters, "torch_calls": args.torch_iters,
               "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "max_rel_diff_vs_torch_arm": float(diff.max())}
        runs = {k: [] for k in legs}
        for _ in range(args.repeats):   # the legs alternate
            for k, (fn, n) in legs.items():
                runs[k].append(timed(fn, n))
        for k in legs:
            res[k] = stats(runs[k])
        res["qacc_calls_replaced"] = calls_replaced
        res["replaced_calls_ms"] = calls_replaced * res["a_fd_qacc_ms"]["median"]
        res["linearize_pays"] = res["l_fd_linearize_ms"]["median"] < res["replaced_calls_ms"]
        res["fd_over_joint"] = res["a_fd_qacc_ms"]["median"] / res["j_jaco_joint_ms"]["median"]
        res["b_over_a"] = res["b_torch_qacc_ms"]["median"] / res["a_fd_qacc_ms"]["median"]
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
