"""Cost of env snapshots (jaco_save_envs / jaco_load_envs) on the plain bench.py workload: 65 536 envs, picking, frame_skip 50, U(-1, 1)^7
actions, auto_reset, episode counters spread over the 700-step episode.  HIP-event time of save_envs (all envs), load_envs (all, identity),
clone_envs (fan-out of env 0; a random permutation) and of plain env steps, alternating over `--rounds` rounds on one env (one handle), so
drifts of the device clock hit them alike; each round times `--reps` calls of each operation and `--steps` steps.  Reported: the medians, a
save + load pair as a share of one env step (the step path is the parent commit's: this feature touches no step kernel), and the bytes
moved divided by the time next to the device's HBM peak (`--hbm-gbs`, 8 000 GB/s for the MI355X).  The state is put back (load of the
saved rows) after the clones, so the workload of the timed steps stays the bench's.
usage: python tools/gpu_snapshot_bench.py [--envs 65536] [--steps 10] [--reps 10] [--rounds 3] [--preroll 100]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_jaco_amd.env import JacoBatchedEnv  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--preroll", type=int, default=100)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    args = ap.parse_args()
    B = args.envs
    env = JacoBatchedEnv(num_envs=B, task="picking", seed=1000, auto_reset=True)
    dev, sim = env.device, env.sim
    env.reset()
    gen = torch.Generator(device=dev); gen.manual_seed(2000)
    ts = env.task_state(); ts[:, 1] = torch.randint(0, env.task_max_steps, (B,), device=dev, generator=gen).float(); env.set_task_state(ts)
    abuf = torch.empty(B, 7, device=dev)

    def step():
        env.step(abuf.uniform_(-1.0, 1.0, generator=gen))

    for _ in range(args.preroll):
        step()
    W = sim.snapshot_words
    rows = torch.empty(B, W, dtype=torch.int32, device=dev)
    perm = torch.randperm(B, device=dev, generator=gen).to(torch.int32)
    ops = {
        "step": step,
        "save_all": lambda: sim.save_envs(out=rows),
        "load_all": lambda: sim.load_envs(rows),
        "clone_fanout": lambda: env.clone_envs(0),
        "clone_permutation": lambda: env.clone_envs(perm),
    }
    times = {k: [] for k in ops}
    for _ in range(args.rounds):
        for k, fn in ops.items():
            if k.startswith("clone"):
                keep = env.save_envs()
            fn()                                    # one untimed call first
            times[k].append(timed(fn, args.steps if k == "step" else args.reps))
            if k.startswith("clone"):
                env.load_envs(keep)
    row_bytes = 4 * W
    res = {"envs": B, "steps_per_round": args.steps, "reps_per_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "row_words": W, "row_bytes": row_bytes, "snapshot_mb_all_envs": B * row_bytes / 1e6, "hbm_peak_gbs": args.hbm_gbs}
    for k in ops:
        res["ms_" + k] = float(np.median(times[k]))
        res["ms_%s_all" % k] = times[k]
    # bytes moved: a save reads the fields and writes the row (2 x row bytes per env, padding and header aside); a load the reverse;
    # a clone is a save plus a load plus the observation rows torch moves (2 x 104 bytes per env, not counted)
    for k, passes in (("save_all", 2), ("load_all", 2), ("clone_fanout", 4), ("clone_permutation", 4)):
        res["gbs_" + k] = passes * B * row_bytes / (res["ms_" + k] * 1e-3) / 1e9
        res["hbm_share_" + k] = res["gbs_" + k] / args.hbm_gbs
    res["save_plus_load_share_of_step"] = (res["ms_save_all"] + res["ms_load_all"]) / res["ms_step"]
    res["env_steps_per_s"] = B / (res["ms_step"] * 1e-3)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
