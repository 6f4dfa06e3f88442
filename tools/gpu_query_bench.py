"""Device time of the robot-configuration query (jaco_query) at 65 536 envs on the default model, next to the physics step it serves.

  (a) one query: the EE frame (pose + Jacobian) plus qM and qfrc_bias -- what an OSC reads per substep
  (b) the same with 16 frames
  (c) send_forces(nsub=1): one contact substep of the same envs
  (d) a whole custom-controller substep: query, the OSC of the step kernel restated in torch (Mx = (J M^-1 J^T)^-1 by two batched
      solves, u = bias - J^T Mx (kp e_x, ko e_r) - kv M dq), send_forces(nsub=1) -- as env-substeps/s
Times: HIP events on the current stream around N back-to-back calls (after warm-up), mean per call.
usage: python tools/gpu_query_bench.py [--envs 65536] [--iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_jaco_amd import workload  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    B = args.envs
    sim = BatchedMujoco(B)
    M = blob.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
    q0 = torch.tensor(workload.reset_states(M["qpos0"], B, seed=1, f32_draws=True), dtype=torch.float32, device="cuda:0")
    sim.set_state(q0, None, None)
    ctrl = torch.tensor(workload.random_ctrl(B, seed=2, scale=0.3), dtype=torch.float32, device="cuda:0")
    for _ in range(20):   # off the exact reset poses: moving arm, falling object
        sim.send_forces(ctrl, nsub=1)
    T = sim.frames
    ee = T.jaco_frame("EE", point=[0.0, 0.0, 0.0])   # the OSC's point: the EE frame origin
    names = [n for n in T.bodies if n and n != "world"]
    many = []
    for n in names:
        try:
            many.append(T.jaco_frame(n))
        except ValueError:   # mocap bodies
            continue
        if len(many) == 16:
            break
    res = {"envs": B, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    res["a_query_ee_qM_bias_ms"] = timed(lambda: sim.query([ee]), args.iters)
    res["b_query_16_frames_ms"] = timed(lambda: sim.query(many), args.iters)
    res["c_send_forces_nsub1_ms"] = timed(lambda: sim.send_forces(ctrl, nsub=1), args.iters)
    res["a_over_c"] = res["a_query_ee_qM_bias_ms"] / res["c_send_forces_nsub1_ms"]
    target = sim.query([ee], jac=False, qM=False, qfrc_bias=False)
    xt, Rt = target["xpos"][:, 0].clone(), target["xmat"][:, 0].reshape(B, 3, 3).clone()
    u = torch.zeros(B, sim.nu, device="cuda:0")
    u[:, 6:] = 0.6
    kp, ko, kv = 100.0, 100.0, 10.0

    def substep():
        r = sim.query([ee])
        J, Mq, bias = r["jac"][:, 0, :, :6], r["qM"][:, :6, :6], r["qfrc_bias"][:, :6]
        dq = sim.get_state()[1][:, :6]
        R = r["xmat"][:, 0].reshape(B, 3, 3)
        e_r = 0.5 * torch.cross(R, Rt, dim=1).sum(-1)   # small-angle orientation error (columns)
        e = torch.cat([kp * (r["xpos"][:, 0] - xt), -ko * e_r], 1)
        MiJt = torch.linalg.solve(Mq, J.transpose(1, 2))
        w = torch.linalg.solve(J @ MiJt, e[:, :, None])   # Mx e (abr_control's plain inverse; no pseudo-inverse branch here)
        tau = bias - (J.transpose(1, 2) @ w)[:, :, 0] - kv * (Mq @ dq[:, :, None])[:, :, 0]
        u[:, :6] = tau
        sim.send_forces(u, nsub=1)
    d_ms = timed(substep, args.iters)
    res["d_custom_controller_substep_ms"] = d_ms
    res["d_env_substeps_per_s"] = B / (d_ms * 1e-3)
    res["flags_or"] = int(np.bitwise_or.reduce(sim.flags().cpu().numpy()))
    print(json.dumps(res))
    sim.close()


if __name__ == "__main__":
    main()
