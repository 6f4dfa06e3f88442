"""Device time of one batched rollout under the operational-space controller (jaco_rollout_osc) at 65 536 rollouts, next to the loop it
replaces and to its two halves taken alone.

Default model; 64 picking reset states (qvel uniform in +-0.5) x 1 024 target samples each = 65 536 rollouts of 50 knots x hold 1,
per_substep, one frame (EE): every knot's target is the EE pose at the start state moved by up to +-8 cm per axis (drawn per rollout and
knot), the start orientation kept; finger servo commands = the finger angle in the base ctrl.
  (a) a_rollout_osc_ms          ONE call on a 64-env handle, the states fanned out through state_index; every knot's qpos, qvel, EE pose
                                and ctrl;   a_rollout_osc_final_only_ms: the same with final_only
  (b) b_loop_ms                 the loop it replaces on a 65 536-env handle under option disable_contact with the fanned-out states set:
                                50 x { get_state(), osc(target_k), send_forces(u, 1) }
  (c) c_rollout_ms              jaco_rollout on (a)'s materialised ctrl output (every knot's qpos, qvel, EE pose);
      c_osc_ms                  ONE jaco_osc call on the 65 536-env handle
Reported: (b) / (a); the law's cost per evaluation inside the rollout, (a - c_rollout) / 50, next to c_osc_ms -- the forward pass is
shared with the substep, so it should come in below the standalone call.
Also: d_two_arms_ms, the two-arm model with two frames (EE_1, EE_2), same shape; h_hold5_ms / p_hold5_per_substep_ms, the default model at
50 knots x hold 5 without / with per_substep.
The final state of (a) is compared with the final state of (b) in the same run (not bit for bit: the handle's option compensated is on,
tests/test_gpu_rollout_osc.py holds the difference to its bound).
Times: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per repetition; the legs alternate
--repeats times and every repeat is reported (min / median / max).  One JSON line, also written to --out (default profiles/rollout_osc_bench.txt; the commit it was taken on is added there by hand).
usage: python tools/gpu_rollout_osc_bench.py [--states 64] [--samples 1024] [--knots 50] [--iters 10] [--loop-iters 3] [--repeats 3] [--out ...]
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
from tools.gpu_rollout_bench import stats, timed  # noqa: E402

SPREAD = 0.08   # m per axis: how far a knot's target lies from the start pose


def problem(model, names, S, K, T, dev, seed):
    """(small handle, qpos [S, nq], qvel [S, nv], frames, index [S K], target_pos [S K, T, F, 3], target_quat [S K, T, F, 4], base ctrl [S K, T, nu])."""
    M = blob.load(_lib.model_path(model))
    sim = BatchedMujoco(S, robot_file=model)
    dual = int(M["nq"][0]) >= 32
    reset = workload.reset_states_dual if dual else (lambda q0, n, seed: workload.reset_states(q0, n, seed=seed, f32_draws=True))
    qpos = torch.tensor(reset(M["qpos0"], S, seed=3), dtype=torch.float32, device=dev)
    qvel = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (S, sim.nv)), dtype=torch.float32, device=dev)
    frames = [sim.frames.jaco_frame(nm) for nm in names]
    r = sim.query(frames, qpos=qpos, qvel=qvel, jac=False, qM=False, qfrc_bias=False)
    index = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(K)
    il = index.long()
    g = torch.Generator(device=dev).manual_seed(seed)
    F = len(names)
    tp = r["xpos"][il][:, None] + SPREAD * (2 * torch.rand(S * K, T, F, 3, generator=g, device=dev) - 1)
    tq = mat2quat(r["xmat"])[il][:, None].expand(S * K, T, F, 4).contiguous()
    base = torch.zeros(S * K, T, sim.nu, device=dev)
    for a in range(sim.nu):
        if M["actuator_position"][a]:
            base[:, :, a] = qpos[il, int(M["jnt_qposadr"][int(M["actuator_jntid"][a])])][:, None]   # the servos hold their joints
    return sim, qpos, qvel, frames, index, tp.contiguous(), tq, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_osc_bench.txt"))
    args = ap.parse_args()
    S, K, T, dev = args.states, args.samples, args.knots, "cuda:0"
    n = S * K
    model, dual = "jaco2_curtain_torque", "jaco2_dual_torque"
    small, qpos, qvel, frames, index, tp, tq, base = problem(model, ("EE",), S, K, T, dev, 11)
    big = BatchedMujoco(n, robot_file=model)
    big.set_option("disable_contact", 1)
    il = index.long()
    q_all, v_all, ws = qpos[il].contiguous(), qvel[il].contiguous(), torch.zeros(n, small.nv, device=dev)
    tp_k, tq_k, base_k = [t.transpose(0, 1).contiguous() for t in (tp, tq, base)]   # [T, n, ...]: the loop's rows
    ee = frames[0]
    common = dict(ctrl=base, state_index=index, frame=ee)

    def loop():
        big.set_state(q_all, v_all, ws)
        out = None
        for k in range(T):
            qk, vk, _ = big.get_state()
            u = big.osc(frames, tp_k[k], tq_k[k], qk, vk, base_k[k])["ctrl"]
            big.send_forces(u, 1)
        out = big.get_state()
        return out

    a = small.rollout_osc(frames, tp, tq, qpos, qvel, **common)
    applied = a["ctrl"].contiguous()
    lq, lv, _ = loop()
    res = {"model": model, "states": S, "samples": K, "rollouts": n, "knots": T, "iters": args.iters, "loop_iters": args.loop_iters, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "status_or": int(a["status"].cpu().numpy().view(np.uint32).max()),
           "final_qpos_max_abs_diff_vs_loop": float((a["qpos"][:, -1] - lq).abs().max()), "final_qvel_max_abs_diff_vs_loop": float((a["qvel"][:, -1] - lv).abs().max())}
    del a, lq, lv
    legs = {
        "a_rollout_osc_ms": (lambda: small.rollout_osc(frames, tp, tq, qpos, qvel, **common), args.iters),
        "a_rollout_osc_final_only_ms": (lambda: small.rollout_osc(frames, tp, tq, qpos, qvel, final_only=True, **common), args.iters),
        "b_loop_ms": (loop, args.loop_iters),
        "c_rollout_ms": (lambda: small.rollout(applied, qpos, qvel, state_index=index, frame=ee), args.iters),
        "c_osc_ms": (lambda: big.osc(frames, tp_k[0], tq_k[0], q_all, v_all, base_k[0]), 5 * args.iters),
    }
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, (fn, iters) in legs.items():
            runs[k].append(timed(fn, iters))
    big.close()
    del applied, tp_k, tq_k, base_k, q_all, v_all
    torch.cuda.empty_cache()
    # hold 5, held and per substep (the default model), and the two-arm model with two frames
    more = {
        "h_hold5_ms": (lambda: small.rollout_osc(frames, tp, tq, qpos, qvel, hold=5, per_substep=False, **common), max(1, args.iters // 3)),
        "p_hold5_per_substep_ms": (lambda: small.rollout_osc(frames, tp, tq, qpos, qvel, hold=5, per_substep=True, **common), max(1, args.iters // 3)),
    }
    two, q2, v2, fr2, idx2, tp2, tq2, base2 = problem(dual, ("EE_1", "EE_2"), S, K, T, dev, 13)
    d = two.rollout_osc(fr2, tp2, tq2, q2, v2, ctrl=base2, state_index=idx2, frame=fr2[0], final_only=True)
    res["two_arms_status_or"] = int(d["status"].cpu().numpy().view(np.uint32).max())
    del d
    more["d_two_arms_ms"] = (lambda: two.rollout_osc(fr2, tp2, tq2, q2, v2, ctrl=base2, state_index=idx2, frame=fr2[0]), args.iters)
    runs.update({k: [] for k in more})
    for _ in range(args.repeats):
        for k, (fn, iters) in more.items():
            runs[k].append(timed(fn, iters))
    for k in runs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    res["loop_over_rollout_osc"] = med("b_loop_ms") / med("a_rollout_osc_ms")
    res["law_ms_per_evaluation_in_rollout"] = (med("a_rollout_osc_ms") - med("c_rollout_ms")) / T
    res["law_in_rollout_over_osc_call"] = res["law_ms_per_evaluation_in_rollout"] / med("c_osc_ms")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_rollout_osc_bench.py --states %d --samples %d --knots %d --iters %d --loop-iters %d --repeats %d\n"
                % (S, K, T, args.iters, args.loop_iters, args.repeats))
        f.write(json.dumps(res) + "\n")
    small.close()
    two.close()


if __name__ == "__main__":
    main()
