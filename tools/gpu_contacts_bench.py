"""Cost of the contact record (jaco_set_contact_record) on the plain bench.py workload: 65 536 envs, picking, frame_skip 50, U(-1, 1)^7
actions, auto_reset, episode counters spread over the 700-step episode -- ms per env step with the record off, and on at capacity 16 and 64.
The three settings alternate over `--rounds` rounds on one env (one handle, one state trajectory), so drifts of the device clock or of the
workload hit them alike; each round times `--steps` steps with HIP events after one untimed step in the new setting.
usage: python tools/gpu_contacts_bench.py [--envs 65536] [--steps 10] [--rounds 3] [--preroll 100]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mujoco_jaco_amd.env import JacoBatchedEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--preroll", type=int, default=100)
    args = ap.parse_args()
    B = args.envs
    env = JacoBatchedEnv(num_envs=B, task="picking", seed=1000, auto_reset=True)
    dev = env.device
    env.reset()
    gen = torch.Generator(device=dev); gen.manual_seed(2000)
    ts = env.task_state(); ts[:, 1] = torch.randint(0, env.task_max_steps, (B,), device=dev, generator=gen).float(); env.set_task_state(ts)
    abuf = torch.empty(B, 7, device=dev)

    def step():
        env.step(abuf.uniform_(-1.0, 1.0, generator=gen))

    for _ in range(args.preroll):
        step()
    times = {0: [], 16: [], 64: []}
    ncon = {16: [], 64: []}
    for _ in range(args.rounds):
        for cap in (0, 16, 64):
            env.record_contacts(cap)
            step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                step()
            b.record()
            torch.cuda.synchronize()
            times[cap].append(a.elapsed_time(b) / args.steps)
            if cap:
                n = env.contacts().ncon.float()
                ncon[cap].append((float(n.clamp(max=cap).mean()), float(n.max()), float((n > cap).float().mean())))
    res = {"envs": B, "steps_per_round": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for cap in (0, 16, 64):
        res["ms_per_step_cap%d" % cap] = float(np.median(times[cap]))
        res["ms_per_step_cap%d_all" % cap] = times[cap]
    for cap in (16, 64):
        res["overhead_cap%d" % cap] = res["ms_per_step_cap%d" % cap] / res["ms_per_step_cap0"] - 1.0
        res["record_mb_written_per_step_cap%d" % cap] = float(np.mean([m for m, _, _ in ncon[cap]])) * B * 96 / 1e6   # (records kept: min(ncon, cap))
        res["kept_mean_ncon_max_overflow_share_cap%d" % cap] = ncon[cap][-1]
    res["env_steps_per_s_cap0"] = B / (res["ms_per_step_cap0"] * 1e-3)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
