"""Device time of one batched open-loop rollout call (jaco_rollout) at 65 536 rollouts, next to the loop it replaces.

Default model; 64 picking reset states (qvel uniform in +-0.5) x 1 024 ctrl sequences each = 65 536 rollouts of 50 knots x hold 1; motor
commands uniform in +-5 per knot, finger servo commands = the finger angle.
  (r) rollout: ONE call on a 64-env handle, the states fanned out through state_index; every knot's qpos, qvel and EE pose
  (f) the same call with final_only
  (l) the loop it replaces, on a 65 536-env handle under option disable_contact with the fanned-out states set:
      50 x { send_forces(ctrl_k, 1), get_state() }
  (m) that loop for a terminal cost: 50 x send_forces(ctrl_k, 1), then one get_state()
Both loop legs are the step kernel's existing code path; each timed repetition starts with the set_state that puts the start states
back (the loop advances the handle).  The final state of (r) is compared with the final state of (l) in the same run.
Times: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per repetition; the legs alternate
--repeats times and every repeat is reported (min / median / max).  One JSON line, also written to --out (default profiles/rollout_bench.txt).
usage: python tools/gpu_rollout_bench.py [--states 64] [--samples 1024] [--knots 50] [--iters 20] [--loop-iters 5] [--repeats 3] [--out profiles/rollout_bench.txt]
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


def timed(fn, iters, warmup=2):
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


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)        # rollout calls per timed window (about 0.2 s)
    ap.add_argument("--loop-iters", type=int, default=5)    # repetitions of the 50-step loop per timed window (about 0.2 s)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.txt"))
    args = ap.parse_args()
    S, K, T, dev, model = args.states, args.samples, args.knots, "cuda:0", "jaco2_curtain_torque"
    n = S * K
    M = blob.load(_lib.model_path(model))
    small, big = BatchedMujoco(S, robot_file=model), BatchedMujoco(n, robot_file=model)
    big.set_option("disable_contact", 1)
    qpos = torch.tensor(workload.reset_states(M["qpos0"], S, seed=3, f32_draws=True), dtype=torch.float32, device=dev)
    qvel = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (S, small.nv)), dtype=torch.float32, device=dev)
    index = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(K)
    ctrl = torch.tensor(np.random.default_rng(7).uniform(-5, 5, (n, T, small.nu)), dtype=torch.float32, device=dev)
    aqadr = [int(M["jnt_qposadr"][int(j)]) for j in M["actuator_jntid"]]
    for a in range(small.nu):
        if M["actuator_position"][a]:
            ctrl[:, :, a] = qpos[index.long(), aqadr[a]][:, None]   # the servos hold their joints
    by_knot = ctrl.transpose(0, 1).contiguous()                     # [T, n, nu]: the loop's ctrl rows
    q_all, v_all, ws = qpos[index.long()].contiguous(), qvel[index.long()].contiguous(), torch.zeros(n, small.nv, device=dev)
    frame = small.frames.jaco_frame("EE")

    def loop(every):
        big.set_state(q_all, v_all, ws)
        out = None
        for k in range(T):
            big.send_forces(by_knot[k], 1)
            if every or k == T - 1:
                out = big.get_state()
        return out

    legs = {
        "r_rollout_ms": (lambda: small.rollout(ctrl, qpos, qvel, state_index=index, frame=frame), args.iters),
        "f_rollout_final_only_ms": (lambda: small.rollout(ctrl, qpos, qvel, state_index=index, frame=frame, final_only=True), args.iters),
        "l_loop_ms": (lambda: loop(True), args.loop_iters),
        "m_loop_final_only_ms": (lambda: loop(False), args.loop_iters),
    }
    r = small.rollout(ctrl, qpos, qvel, state_index=index, frame=frame, final_only=True)
    lq, lv, _ = loop(True)
    res = {"model": model, "states": S, "samples": K, "rollouts": n, "knots": T, "hold": 1, "iters": args.iters, "loop_iters": args.loop_iters, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "status_or": int(r["status"].cpu().numpy().view(np.uint32).max()),
           "final_qpos_max_abs_diff_vs_loop": float((r["qpos"][:, 0] - lq).abs().max()), "final_qvel_max_abs_diff_vs_loop": float((r["qvel"][:, 0] - lv).abs().max())}
    del r, lq, lv
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, (fn, iters) in legs.items():
            runs[k].append(timed(fn, iters))
    for k in legs:
        res[k] = stats(runs[k])
    res["loop_over_rollout"] = res["l_loop_ms"]["median"] / res["r_rollout_ms"]["median"]
    res["loop_over_rollout_final_only"] = res["m_loop_final_only_ms"]["median"] / res["f_rollout_final_only_ms"]["median"]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_rollout_bench.py --states %d --samples %d --knots %d --iters %d --loop-iters %d --repeats %d\n" % (S, K, T, args.iters, args.loop_iters, args.repeats))
        f.write(json.dumps(res) + "\n")
    small.close()
    big.close()


if __name__ == "__main__":
    main()
