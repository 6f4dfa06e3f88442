"""Device time of the transition Jacobians of every knot of a batch of plans (jaco_transition_fd) next to the path it replaces, next to
the other two launches of the same iLQR iteration, and over the number of column groups.

4 096 plans x 50 knots on the default model: the plans and states of tools/gpu_rollout_fb_bench.py are rolled out once, and the 204 800
(state at the start of a knot, applied ctrl of the knot) pairs are the input.  9 hinge dofs, 9 ctrl words (27 columns).
  (c) transition_fd, centered, hold 1                      (f) forward differences            (h) centered, hold 5
  (s) want = ("status",): the nominal evaluation alone, no A / B store -- NOT the same work as (c): 1 evaluation per pair against 54
  (l) the replaced path: set_state of the pairs into a second handle of 204 800 envs, then robot_config.linearize there (one jaco_fd
      launch of 37 forward passes per env + the torch assembly); its B has the 6 motor words' columns only
  (r) jaco_rollout_fb and (b) jaco_lqr (nx 18, nu 9, tools/gpu_lqr_bench.py's draw) on the same 4 096 plans
  (d) the two-arm model: 18 hinge dofs, 18 ctrl words (54 columns), --dual-pairs pairs drawn like tools/gpu_fd_bench.py's states
  groups: n in {64, 4 096, 204 800} x groups in {1, 3, 9, 27}, centered, hold 1, and groups = 0 (the library's rule) at each n
Everything is MEASURED in this run: HIP events on the current stream around N back-to-back repetitions after warm-up, mean per
repetition; the legs alternate --repeats times and every repeat is reported (min / median / max).  One JSON line, also written to --out
(default profiles/transition_fd_bench.txt), with the commit it was measured on.
usage: python tools/gpu_transition_bench.py [--plans 4096] [--knots 50] [--iters 3] [--repeats 3] [--dual-pairs 65536] [--commit ID] [--out ...]
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
from mujoco_jaco_amd.robot_config import BatchedMujocoConfig  # noqa: E402
from tools.gpu_lqr_bench import commit, draw  # noqa: E402
from tools.gpu_rollout_bench import stats, timed  # noqa: E402
from tools.gpu_rollout_fb_bench import problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=4096)
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dual-pairs", type=int, default=65536)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transition_fd_bench.txt"))
    args = ap.parse_args()
    P, T, dev, model = args.plans, args.knots, "cuda:0", "jaco2_curtain_torque"
    n = P * T
    sim = BatchedMujoco(2, robot_file=model)
    M = blob.load(_lib.model_path(model))
    qpos, qvel, plan, _ = problem(model, sim, P, T, dev, 7)
    dofs = plan["dofs"]
    acts = list(range(sim.nu))
    fwd = lambda: sim.rollout_feedback(plan["ctrl"], qpos, qvel, **{k: v for k, v in plan.items() if k != "ctrl"})
    r = fwd()
    Q = torch.cat([qpos[:, None], r["qpos"][:, :-1]], 1).reshape(n, sim.nq).contiguous()     # the state at the start of every knot
    V = torch.cat([qvel[:, None], r["qvel"][:, :-1]], 1).reshape(n, sim.nv).contiguous()
    C = r["ctrl"].reshape(n, sim.nu).contiguous()
    res = {"plans": P, "knots": T, "pairs": n, "dofs": len(dofs), "ctrl_words": len(acts), "iters": args.iters, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "commit": args.commit or commit(), "measured": "every *_ms entry and every ratio below: HIP events, this run",
           "rollout_status_or": int(r["status"].cpu().numpy().view("uint32").max())}
    tf = lambda want=("A", "B"), rows=slice(None), **k: sim.transition_fd(C[rows], Q[rows], V[rows], dofs=dofs, acts=acts, want=want, **k)
    a = tf(("A", "B", "status"))
    res["nominal_status_or"] = int(a["status"].cpu().numpy().view("uint32").max())
    res["A_finite_share"] = float(torch.isfinite(a["A"]).all(-1).all(-1).float().mean())
    del a
    # the replaced path: a second handle holding the pairs
    big = BatchedMujoco(n, robot_file=model)
    cfg = BatchedMujocoConfig(big)
    names = [big.frames.names["joint"][j] for j in range(int(M["njnt"][0])) if int(M["jnt_type"][j]) == 3]
    ws = torch.zeros(n, sim.nv, device=dev)

    def replaced():
        big.set_state(Q, V, ws)
        return cfg.linearize(joints=names, ctrl=C)
    A2, B2, _ = replaced()
    a = tf(("A",))
    res["A_vs_replaced_path_median_abs"] = float((a["A"] - A2).abs().median())
    del a, A2, B2
    g = draw(P, T, 18, 9, dev, 118)
    outs = {k: torch.empty(s, device=dev) for k, s in (("gain", (P, T, 9, 18)), ("kff", (P, T, 9)), ("dV", (P, 2)), ("Vxx0", (P, 18, 18)), ("Vx0", (P, 18)))}
    outs["status"] = torch.zeros(P, dtype=torch.int32, device=dev)
    legs = {
        "c_transition_centered_ms": lambda: tf(),
        "f_transition_forward_ms": lambda: tf(centered=False),
        "h_transition_centered_hold5_ms": lambda: tf(hold=5),
        "s_transition_status_only_ms": lambda: tf(("status",)),
        "l_replaced_set_state_linearize_assembly_ms": replaced,
        "r_jaco_rollout_fb_ms": fwd,
        "b_jaco_lqr_ms": lambda: sim.lqr_backward(g["A"], g["B"], g["lxx"], g["luu"], lx=g["lx"], lu=g["lu"], Vxx=g["Vxx"], Vx=g["Vx"], out=outs),
    }
    for m in (64, 4096, n):
        for groups in (0, 1, 3, 9, 27):
            legs["groups_n%d_g%d_ms" % (m, groups)] = lambda m=m, groups=groups: tf(rows=slice(0, m), groups=groups)
    # the two-arm model
    dual = BatchedMujoco(2, robot_file="jaco2_dual_torque")
    Md = blob.load(_lib.model_path("jaco2_dual_torque"))
    nd_ = args.dual_pairs
    qd = torch.tensor(workload.reset_states_dual(Md["qpos0"], nd_, seed=3), dtype=torch.float32, device=dev)
    vd = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (nd_, dual.nv)), dtype=torch.float32, device=dev)
    cd = torch.tensor(np.random.default_rng(7).uniform(-5, 5, (nd_, dual.nu)), dtype=torch.float32, device=dev)
    hinge = [j for j in range(int(Md["njnt"][0])) if int(Md["jnt_type"][j]) == 3]
    ddofs = [int(Md["jnt_dofadr"][j]) for j in hinge]
    for a_ in range(dual.nu):
        if Md["actuator_position"][a_]:
            cd[:, a_] = qd[:, int(Md["jnt_qposadr"][int(Md["actuator_jntid"][a_])])]   # the servos hold their joints
    res.update(dual_pairs=nd_, dual_dofs=len(ddofs), dual_ctrl_words=dual.nu)
    legs["d_transition_two_arms_ms"] = lambda: dual.transition_fd(cd, qd, vd, dofs=ddofs, acts=list(range(dual.nu)))
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):   # the legs alternate
        for k, fn in legs.items():
            runs[k].append(timed(fn, args.iters, warmup=1))
    for k in legs:
        res[k] = stats(runs[k])
    med = lambda k: res[k]["median"]
    res["replaced_over_transition_centered"] = med("l_replaced_set_state_linearize_assembly_ms") / med("c_transition_centered_ms")
    res["replaced_over_transition_forward"] = med("l_replaced_set_state_linearize_assembly_ms") / med("f_transition_forward_ms")
    res["transition_centered_over_rollout_fb"] = med("c_transition_centered_ms") / med("r_jaco_rollout_fb_ms")
    res["transition_centered_over_lqr"] = med("c_transition_centered_ms") / med("b_jaco_lqr_ms")
    res["ns_per_evaluation_centered"] = 1e6 * med("c_transition_centered_ms") / (n * 2 * (2 * len(dofs) + len(acts)))
    res["ns_per_evaluation_status_only"] = 1e6 * med("s_transition_status_only_ms") / n
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("== python tools/gpu_transition_bench.py --plans %d --knots %d --iters %d --repeats %d --dual-pairs %d\n" % (P, T, args.iters, args.repeats, nd_))
        f.write(json.dumps(res) + "\n")
    for s in (sim, big, dual):
        s.close()


if __name__ == "__main__":
    main()
