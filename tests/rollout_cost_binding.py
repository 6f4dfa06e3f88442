"""The costed rollout kernel (mujoco_jaco_amd/csrc/rollout_cost.h, jaco_rollout_cost) under the wavefront emulator (emu_rollout_cost of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 cost reference (the header's formula evaluated in fp64 on a call's own fp32 outputs), the input sets --
rollout_fb_binding.shared's states, plans and gains as they are, plus seeded goals distinct per plan, weights and noise -- the cases
shared by the CPU and the GPU tier and the refusals.  emu_sim.EmuSim runs BatchedMujoco.rollout_cost on the emulated call (CPU tests of
robot_config).

A tier hands the cases three calls:
  run(model, ctrl [P, T, nu], qpos0=None, qvel0=None, noise=None, xgoal=None, pgoal=None, weights=None, goal_per_knot=0, kff=None,
      gain=None, xref=None, dofs=(), alpha=None, plan_index=None, state_index=None, nstates=None, frame=None, want=OUTS, hold=1,
      final_only=0, handle=None) -> {output: array}
  run_fb: rollout_fb_binding's `run` (jaco_rollout_fb on the same tier);  run_open: its `run_open` (jaco_rollout).
Every output array is handed in filled with SENTINEL (status: STATUS_SENTINEL), so what a call leaves untouched shows.
"""
import numpy as np

import fd_binding as fb
import rollout_binding as rb
import rollout_fb_binding as fbb
from fd_binding import bits
from mujoco_jaco_amd import _lib as product_lib
from rollout_binding import SENTINEL, STATUS_SENTINEL, same

OUTS = ("qpos", "qvel", "xpos", "xmat", "status", "ctrl", "cost", "terms")
COST = ("cost", "terms", "status")
FLAG_NAN = product_lib.JACO_FLAG_NAN


def weight_options(weights):
    """{"wx", "wxT", "wu", "wp", "wpT"} (each optional) as keywords of _lib.JacoRolloutCostOptions."""
    w = dict(weights or {})
    return {k: w[k] for k in ("wx", "wxT", "wu", "wp", "wpT") if k in w}


def records(ptr, outs, ctrl, kff, gain, xref, alpha, pidx, noise, xgoal, pgoal, weights, dofs, nknots, hold, final_only, goal_per_knot, nplans, ndofs=None,
            no_ctrl=False):
    """(options, plan, goal, out) records of one call; ptr(array or tensor or None) -> c_void_p or None."""
    opt = product_lib.JacoRolloutCostOptions(nknots=nknots, hold=hold, final_only=final_only, goal_per_knot=goal_per_knot, dofs=dofs, **weight_options(weights))
    if ndofs is not None:
        opt.ndofs = ndofs
    plan = product_lib.JacoRolloutPlan(None if no_ctrl else ptr(ctrl), ptr(kff), ptr(gain), ptr(xref), ptr(alpha), ptr(pidx), nplans)
    goal = product_lib.JacoRolloutGoal(ptr(noise), ptr(xgoal), ptr(pgoal))
    out = product_lib.JacoRolloutCostOut(*[ptr(outs.get(k)) for k in OUTS])
    return opt, plan, goal, out


def rollout_cost(model, ctrl, qpos0=None, qvel0=None, noise=None, xgoal=None, pgoal=None, weights=None, goal_per_knot=0, kff=None, gain=None, xref=None,
                 dofs=(), alpha=None, plan_index=None, state_index=None, nstates=None, frame=None, want=OUTS, hold=1, final_only=0, handle=None, n=None,
                 nknots=None, nplans=None, ndofs=None, no_opt=False, no_out=False, no_ctrl=False, no_plan=False, no_goal=False):
    """Emulated jaco_rollout_cost: {output: array} in the C ABI's layout.  n / nknots / nplans / ndofs override what the arrays say
    (refusals); no_* hand NULL pointers.  Raises ValueError with the library's message when the call is refused, with the outputs it was
    handed in .outputs."""
    L, blob, dims, num_envs, hq, hv = rb.emu_model(model, handle)
    p, ref = rb.HOST.ptr, rb.ref
    ctrl, kff, gain, xref, alpha, q0, v0, noise, xgoal, pgoal = [rb.HOST.f32(a) for a in (ctrl, kff, gain, xref, alpha, qpos0, qvel0, noise, xgoal, pgoal)]
    pidx, sidx = rb.HOST.i32(plan_index), rb.HOST.i32(state_index)
    n, nknots, nstates, res = rb.prelude(rb.HOST, dims, want, ctrl.shape[0], ctrl.shape[1], q0, v0, num_envs, (noise, pidx, sidx, alpha), n, nknots, nstates, hold,
                                         final_only)
    opt, plan, goal, out = records(p, res, ctrl, kff, gain, xref, alpha, pidx, noise, xgoal, pgoal, weights, dofs, nknots, hold, final_only, goal_per_knot,
                                   ctrl.shape[0] if nplans is None else nplans, ndofs, no_ctrl)
    rc = L.emu_rollout_cost(blob, len(blob), ref(opt, no_opt), ref(frame), n, p(sidx), nstates, p(q0), p(v0), ref(plan, no_plan), ref(goal, no_goal),
                            ref(out, no_out), num_envs, p(hq), p(hv))
    return rb.checked(L, rc, "emu_rollout_cost", res)


# ---- the fp64 reference
def cost64(r, dofs, qadr, weights, xgoal=None, pgoal=None, goal_per_knot=0, plan_index=None):
    """The header's formula in fp64 on the fp32 outputs r = {"ctrl", "qpos", "qvel", "xpos"} (every knot) of a call:
    (J [n], terms [n, 3] = ctrl / state / pose, last [n] = the part of J the last knot's state and pose terms make)."""
    f64 = lambda a: np.asarray(a, np.float64)
    u = f64(r["ctrl"])
    n, T, nu = u.shape
    w = weights or {}
    pad = lambda a, m: np.concatenate([f64(np.asarray(a, np.float32)), np.zeros(m)])[:m]   # (the options hold fp32 words)
    nx = 2 * len(dofs)
    wx, wxT, wu = pad(w.get("wx", ()), nx), pad(w.get("wxT", ()), nx), pad(w.get("wu", ()), nu)
    wp, wpT = float(np.float32(w.get("wp", 0.0))), float(np.float32(w.get("wpT", 0.0)))
    p = np.arange(n) if plan_index is None else np.asarray(plan_index)
    knots = np.arange(T) if goal_per_knot else np.zeros(T, int)
    tu = 0.5 * (wu * u ** 2).sum((1, 2))
    sx, sp = np.zeros((n, T)), np.zeros((n, T))
    if nx and xgoal is not None:
        x = np.concatenate([f64(r["qpos"])[:, :, list(qadr)], f64(r["qvel"])[:, :, list(dofs)]], 2)
        W = np.where((np.arange(T) == T - 1)[:, None], wxT, wx)
        sx = 0.5 * (W * (x - f64(xgoal)[p][:, knots]) ** 2).sum(2)
    if pgoal is not None and (wp or wpT):
        W = np.where(np.arange(T) == T - 1, wpT, wp)
        sp = 0.5 * W * ((f64(r["xpos"]) - f64(pgoal)[p][:, knots]) ** 2).sum(2)
    terms = np.stack([tu, sx.sum(1), sp.sum(1)], 1)
    return terms.sum(1), terms, sx[:, -1] + sp[:, -1]


def cap(T, nx, nu):
    """Case 3's derived cap on |J - J64| / J64: every term is non-negative, so in ANY summation order each of the N = T (nx + 3 + nu)
    terms enters at most N - 1 additions that each round a partial sum no larger than J to 2^-24 relative, and forming a term (one
    subtraction, one square, the halved weight, the fused multiply-add) costs at most 4 more roundings; the three wave sums and the
    final two additions are among the N - 1.  (N + 8) 2^-24, as the issue states it."""
    return (T * (nx + 3 + nu) + 8) * 2.0 ** -24


# ---- inputs: rollout_fb_binding.shared's, plus goals, weights and noise
NOISE_MOTOR, NOISE_SERVO = 0.5, 1e-3
GOAL_DQ, GOAL_DV, GOAL_P = 0.3, 1.0, 0.25
MIN_SHARE = 0.01
_shared = {}


def shared(model, long=False):
    """rollout_fb_binding.shared(model, long) as it is, plus "noise" [n, T, nu] (uniform in +-NOISE_MOTOR on the motor words,
    +-NOISE_SERVO on the servos': a servo's force range is 0.015 rad of command wide), "xgoal" [n, T, nx] (the plan's reference states
    displaced by up to GOAL_DQ rad / GOAL_DV rad/s, drawn per plan and knot), "pgoal" [n, T, 3] (a point up to GOAL_P from
    (0.3, 0, 0.5), per plan and knot), "ee" (the EE frame with a non-zero point) and "weights": distinct per word, the last knot's ten
    times the running ones.  [:, 0] of the goals serves goal_per_knot = 0."""
    key = (model, long)
    if key not in _shared:
        g = dict(fbb.shared(model, long))
        n, T, nu = g["c"].shape
        nx = 2 * len(g["dofs"])
        rng = np.random.default_rng(91)
        servo = fb.tables(model)["position"]
        g["noise"] = (rng.uniform(-1, 1, (n, T, nu)) * np.where(servo, NOISE_SERVO, NOISE_MOTOR)).astype(np.float32)
        d = rng.uniform(-1, 1, (n, T, nx)) * np.concatenate([np.full(nx // 2, GOAL_DQ), np.full(nx // 2, GOAL_DV)])
        g["xgoal"] = (g["xref"].astype(np.float64) + d).astype(np.float32)
        g["pgoal"] = (np.array([0.3, 0.0, 0.5]) + rng.uniform(-GOAL_P, GOAL_P, (n, T, 3))).astype(np.float32)
        g["ee"] = rb.frames(model)[1]
        wx = np.concatenate([rng.uniform(1.0, 3.0, nx // 2), rng.uniform(0.02, 0.06, nx // 2)])
        g["weights"] = dict(wx=wx, wxT=10 * wx, wu=rng.uniform(0.01, 0.03, nu), wp=4.0, wpT=40.0)
        _shared[key] = g
    return _shared[key]


def goal_args(g, goal_per_knot, sl=slice(None)):
    pick = (lambda a: a[sl]) if goal_per_knot else (lambda a: np.ascontiguousarray(a[sl][:, :1]))
    return dict(xgoal=pick(g["xgoal"]), pgoal=pick(g["pgoal"]), goal_per_knot=goal_per_knot, weights=g["weights"], frame=g["ee"])


def state_args(g):
    return dict(qpos0=g["q"], qvel0=g["v"])


# ---- the cases
def case_degenerate(run, run_fb, model, long=False):
    """Case 1: without noise the six shared outputs are jaco_rollout_fb's, bit for bit -- gains, kff and alpha in, the cost's weights on."""
    g = shared(model, long)
    kff, alpha = fbb.kff_alpha(model, g["c"].shape)
    k = dict(kff=kff, alpha=alpha, hold=g["hold"], **fbb.plan_args(g))
    r = run(model, g["c"], **state_args(g), **goal_args(g, 1), **k)
    same(run_fb(model, g["c"], g["q"], g["v"], frame=g["ee"], **k), r, fbb.OUTS)
    assert np.isfinite(r["cost"]).all() and (r["cost"] > 0).all()


def case_noise(run, run_open, model, long=False):
    """Case 2: with noise and no feedback terms the outputs are jaco_rollout's on ctrl[p] + noise (the add done in fp32 on the host), bit
    for bit, and the ctrl output is that sum; cost(nominal = u + eps, no noise) equals cost(nominal = u, noise = eps), bit for bit."""
    g = shared(model, long)
    summed = g["c"] + g["noise"]
    assert summed.dtype == np.float32 and not (bits(summed) == bits(g["c"])).all(2).any()
    r = run(model, g["c"], **state_args(g), noise=g["noise"], hold=g["hold"], dofs=g["dofs"], **goal_args(g, 0))
    same(run_open(model, summed, g["q"], g["v"], frame=g["ee"], hold=g["hold"]), r, rb.OUTS)
    assert (bits(r["ctrl"]) == bits(summed)).all()
    s = run(model, summed, **state_args(g), hold=g["hold"], dofs=g["dofs"], want=COST, **goal_args(g, 0))
    same(s, r, COST)


def costed(run, model, long, goal_per_knot, gains, hold, **more):
    """One call on shared(model, long) with noise, every output asked for, kept on the tier's `run`."""
    memo = run.__dict__.setdefault("_costed", {})
    key = (model, long, goal_per_knot, gains, hold) + tuple(sorted(more.items()))
    if key not in memo:
        g = shared(model, long)
        plan = fbb.plan_args(g) if gains else dict(dofs=g["dofs"])
        memo[key] = run(model, g["c"], **state_args(g), noise=g["noise"], hold=hold, **goal_args(g, goal_per_knot), **plan, **more)
    return memo[key]


def case_cost(run, model, long, goal_per_knot, gains, hold):
    """Case 3: cost and terms against the fp64 formula on the call's own fp32 outputs.  Asserts, on the fp64 side, that in every rollout
    the ctrl, state and pose terms and the last knot's share are each at least MIN_SHARE of J.  Returns (the largest |J - J64| / J64,
    the largest |term - term64| / J64, the cap)."""
    g = shared(model, long)
    r = costed(run, model, long, goal_per_knot, gains, hold)
    assert (r["status"] == 0).all(), r["status"]
    k = goal_args(g, goal_per_knot)
    J, terms, last = cost64(r, g["dofs"], g["qadr"], g["weights"], k["xgoal"], k["pgoal"], goal_per_knot)
    share = np.concatenate([terms, last[:, None]], 1) / J[:, None]
    assert (share >= MIN_SHARE).all(), (model, share.min(0))
    eJ = float((np.abs(r["cost"].astype(np.float64) - J) / J).max())
    eT = float((np.abs(r["terms"].astype(np.float64) - terms) / J[:, None]).max())
    T, nu = r["ctrl"].shape[1:]
    return eJ, eT, cap(T, 2 * len(g["dofs"]), nu)


def case_independence(run, model, long=False):
    """Cases 4 and 5: cost and terms are bit-identical whether the call asks for all eight outputs, for cost / terms / status only, or
    sets final_only = 1; two runs agree bit for bit."""
    g = shared(model, long)
    full = costed(run, model, long, 1, True, g["hold"])
    k = dict(noise=g["noise"], hold=g["hold"], **goal_args(g, 1), **fbb.plan_args(g))
    only = run(model, g["c"], **state_args(g), want=COST, **k)
    assert set(only) == set(COST)
    same(only, full, COST)
    same(run(model, g["c"], **state_args(g), want=("cost",), **k), full, ("cost",))
    last = run(model, g["c"], **state_args(g), final_only=1, **k)
    same(last, full, COST + ("ctrl",))
    same(last, {key: full[key][:, -1:] for key in rb.OUTS[:4]}, rb.OUTS[:4])
    same(run(model, g["c"], **state_args(g), **k), full)
    # a pose weight without the pose outputs, and the last knot's alone
    w = dict(g["weights"], wp=0.0)
    k["weights"] = w
    a, b = run(model, g["c"], **state_args(g), want=COST, **k), run(model, g["c"], **state_args(g), **k)
    same(a, b, COST)
    J, terms, _ = cost64(b, g["dofs"], g["qadr"], w, k["xgoal"], k["pgoal"], 1)
    assert (terms[:, 2] > 0).all() and np.abs(a["terms"][:, 2] / terms[:, 2] - 1).max() < 1e-5


def case_fan_out(run, model=rb.MODEL):
    """Case 6: plans x alphas x states as rollout_fb_binding.case_fan_out, every combination twice with the same noise row: the indexed
    call against materialised plans, goals and states, bit for bit; the twins' costs equal bit for bit; changing only one plan's goal
    changes the cost of the rollouts on that plan and of no other."""
    g = shared(model)
    P, A, S = fbb.FAN
    kff, _ = fbb.kff_alpha(model, g["c"].shape)
    pi, ai, si = [np.tile(x.reshape(-1), 2) for x in np.meshgrid(np.arange(P), np.arange(A), np.arange(S), indexing="ij")]
    m = len(pi) // 2
    alpha = np.array([0.0, 0.25, 0.5, 1.0], np.float32)[ai]
    noise = np.tile(g["noise"][:m], (2, 1, 1))
    k = dict(hold=g["hold"], dofs=g["dofs"], alpha=alpha, noise=noise, goal_per_knot=1, weights=g["weights"], frame=g["ee"])
    plans = lambda s: dict(kff=kff[s], gain=g["gain"][s], xref=g["xref"][s], xgoal=g["xgoal"][s], pgoal=g["pgoal"][s])
    r = run(model, g["c"][:P], g["q"][:S], g["v"][:S], plan_index=pi, state_index=si, **plans(slice(0, P)), **k)
    assert (r["status"] == 0).all() and len(np.unique(bits(r["cost"][:m]))) == m
    same({key: x[:m] for key, x in r.items()}, {key: x[m:] for key, x in r.items()})
    same(run(model, g["c"][pi], g["q"][si], g["v"][si], **plans(pi), **k), r)
    moved = plans(slice(0, P))
    moved["xgoal"] = moved["xgoal"].copy()
    moved["xgoal"][1] += np.float32(0.125)
    s = run(model, g["c"][:P], g["q"][:S], g["v"][:S], plan_index=pi, state_index=si, want=COST, **moved, **k)
    assert (bits(s["cost"]) != bits(r["cost"]))[pi == 1].all() and (bits(s["cost"]) == bits(r["cost"]))[pi != 1].all()


def case_bad_index(run, model=rb.MODEL):
    """Case 7: plan_idx and state_idx entries out of range write the status word alone: the sentinels of every other output stand, cost
    and terms included, and every other rollout is bitwise what it is without the bad entries."""
    g = shared(model)
    m, P = rb.BAD_STATES, rb.BAD_PLANS
    k = dict(hold=g["hold"], gain=g["gain"][:P], xref=g["xref"][:P], dofs=g["dofs"], **goal_args(g, 1, slice(0, P)))
    rb.bad_index(lambda keep, **index: run(model, g["c"][:P], g["q"][:m], g["v"][:m], noise=g["noise"][keep], **index, **k), OUTS, plans=True)


def case_non_finite(run, model=rb.MODEL):
    """Case 8: one start row with qvel = inf in a hinge dof: that rollout has JACO_FLAG_NAN and cost = terms = +inf; its neighbours are
    unaffected, bit for bit."""
    g = shared(model)
    m, i = 5, 2
    v = g["v"][:m].copy()
    v[i, g["dofs"][1]] = np.inf
    k = dict(hold=g["hold"], noise=g["noise"][:m], want=COST, **goal_args(g, 1, slice(0, m)), **fbb.plan_args(g, slice(0, m)))
    r = run(model, g["c"][:m], g["q"][:m], v, **k)
    ok = run(model, g["c"][:m], g["q"][:m], g["v"][:m], **k)
    assert r["status"][i] & FLAG_NAN and np.isposinf(r["cost"][i]) and np.isposinf(r["terms"][i]).all()
    others = np.arange(m) != i
    same({key: x[others] for key, x in r.items()}, {key: x[others] for key, x in ok.items()})
    assert np.isfinite(ok["cost"]).all()


# ---- the refusals: one argument set per JACO_EINVAL case of include/jaco_env.h, for the emulator's entry and the library's alike
REFUSAL_MODEL = rb.REFUSAL_MODEL
REFUSALS = {k: v for k, v in fbb.REFUSALS.items() if k not in ("per_substep_2", "no_outputs")}
REFUSALS.update({
    "no_outputs": "at least one of the outputs qpos, qvel, xpos, xmat, status, ctrl, cost and terms is required",
    "goal_per_knot_2": "goal_per_knot must be 0 or 1",
    "weight_negative": "weight wx[3] is negative or not finite",
    "weight_nan": "weight wu[2] is negative or not finite",
    "weight_inf": "weight wpT is negative or not finite",
    "final_weight_negative": "weight wxT[0] is negative or not finite",
    "pose_weight_negative": "weight wp is negative or not finite",
    "state_weight_without_xgoal": "a non-zero state weight needs xgoal",
    "state_weight_null_goal": "a non-zero state weight needs xgoal",
    "state_weight_without_dofs": "a non-zero state weight needs dofs",
    "state_weight_dof_free": "dof 9 belongs to a free joint",
    "pose_weight_without_pgoal": "a non-zero pose weight needs pgoal",
    "pose_weight_without_frame": "a non-zero pose weight needs a frame",
})


def refusal_args(case):
    """Keyword arguments of one refused call of `rollout_cost` / the GPU tier's twin on REFUSAL_MODEL: REFUSAL_N plans of 2 knots."""
    if case in fbb.REFUSALS and case != "no_outputs":
        k = fbb.refusal_args(case)
        k.pop("per_substep", None)
        return dict(k, want=k["want"] + ("cost",))
    g = shared(REFUSAL_MODEL)
    n = rb.REFUSAL_N
    k = dict(ctrl=g["c"][:n, :2], qpos0=g["q"][:n], qvel0=g["v"][:n], want=("qpos", "status", "cost", "terms"), dofs=g["dofs"], frame=g["ee"],
             xgoal=g["xgoal"][:n, :1], pgoal=g["pgoal"][:n, :1], weights=g["weights"])
    W = lambda **w: dict(weights=dict(g["weights"], **w))
    wx = np.array(g["weights"]["wx"])
    k.update({"no_outputs": dict(want=()), "goal_per_knot_2": dict(goal_per_knot=2),
              "weight_negative": W(wx=np.where(np.arange(len(wx)) == 3, -1.0, wx)), "weight_nan": W(wu=[0.1, 0.1, np.nan]), "weight_inf": W(wpT=np.inf),
              "final_weight_negative": W(wxT=[-0.5]), "pose_weight_negative": W(wp=-1.0),
              "state_weight_without_xgoal": dict(xgoal=None), "state_weight_null_goal": dict(no_goal=True), "state_weight_without_dofs": dict(dofs=()),
              "state_weight_dof_free": dict(dofs=[3, 9], xgoal=np.ascontiguousarray(g["xgoal"][:n, :1, :4])),
              "pose_weight_without_pgoal": dict(pgoal=None), "pose_weight_without_frame": dict(frame=None)}[case])
    return k


# ---- case 10: the Python tiers.  make_sim(model, qpos, qvel) -> a BatchedMujoco (GPU tier) or emu_sim.EmuSim.
MPPI_MODELS = fbb.HOLD_MODELS
MPPI_B, MPPI_K, MPPI_T, MPPI_HOLD, MPPI_ITERS = 3, 16, 6, 2, 4
MPPI_SIGMA, MPPI_SEED, MPPI_TEMPERATURE = 2.0, 5, 0.05
MPPI_DQ = 0.15   # rad/s: the joint velocities asked for -- what 12 substeps of motor torque can reach
MPPI_W = dict(w_q=1.0, w_dq=100.0, w_ee=10.0, w_u=1e-3, w_q_final=10.0, w_dq_final=1000.0, w_ee_final=100.0)


def mppi_problem(make_sim, model):
    """(cfg, u0 [B, T, m] = gravity compensation held, the goals: q_goal = the posture 0.2 rad off on every arm joint, dq_goal = +-MPPI_DQ on
    alternating joints, ee_goal = the EE position at the start moved by 5 cm, the noise of every iteration [ITERS, B, K, T, m] with sample 0 noise-free)."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    q, v = fbb.hold_postures(model)
    q, v = q[:MPPI_B], v[:MPPI_B]
    sim = make_sim(model, q, v)
    cfg = BatchedMujocoConfig(sim, ee=MPPI_MODELS[model])
    Tm = fb.tables(model)
    acts = [int(np.flatnonzero(Tm["dof"] == d)[0]) for d in cfg.arm]
    u0 = cfg.joint(joints=None).gravity_compensation()[:, acts][:, None].expand(-1, MPPI_T, -1).contiguous()
    rng = np.random.default_rng(MPPI_SEED)
    noise = (MPPI_SIGMA * rng.standard_normal((MPPI_ITERS, MPPI_B, MPPI_K, MPPI_T, len(acts)))).astype(np.float32)
    noise[:, :, 0] = 0.0
    q_goal = torch.as_tensor(q[:, list(cfg.arm_qadr)] + np.float32(0.2)).to(sim.device)
    ee0 = cfg.rollout_feedback(u0[:, :1], final_only=True)["ee_pos"][:, 0]
    ee_goal = ee0 + torch.tensor([0.05, -0.03, 0.04], device=sim.device)
    dq_goal = MPPI_DQ * torch.tensor([1.0, -1.0], device=sim.device).repeat(q_goal.shape[1])[:q_goal.shape[1]].expand_as(q_goal)
    goals = dict(q_goal=q_goal, dq_goal=dq_goal.contiguous(), ee_goal=ee_goal, hold=MPPI_HOLD, **MPPI_W)
    return cfg, u0, goals, torch.as_tensor(noise).to(sim.device)


def case_config_cost(make_sim, model):
    """Case 10a: robot_config.rollout_cost against the fp64 formula on trajectories=True's own outputs (q, dq, ee_pos, u), K samples per
    env, per-knot goals.  Returns the largest |J - J64| / J64 and the cap."""
    import torch
    cfg, u0, goals, noise = mppi_problem(make_sim, model)
    N = lambda t: t.cpu().numpy()
    T, n = MPPI_T, len(cfg.arm)
    ramp = 0.01 * torch.arange(T, device=u0.device, dtype=torch.float32)[None, :, None]
    goals = dict(goals, **{key: goals[key][:, None].expand(-1, T, -1) + ramp for key in ("q_goal", "dq_goal", "ee_goal")})
    r = cfg.rollout_cost(u0, noise=noise[0], trajectories=True, **goals)
    assert r["cost"].shape == (MPPI_B, MPPI_K) and r["terms"].shape == (MPPI_B, MPPI_K, 3) and r["status"].shape == (MPPI_B, MPPI_K)
    assert r["q"].shape == (MPPI_B, MPPI_K, T, n) and r["u"].shape == (MPPI_B, MPPI_K, T, u0.shape[2]) and (N(r["status"]) == 0).all()
    assert (bits(N(r["u"])) == bits(N(u0)[:, None] + N(noise[0]))).all()
    f64 = lambda t: N(t).astype(np.float64)
    W = MPPI_W
    last = np.arange(T) == T - 1
    wq, wdq, wee = [np.where(last, W[k + "_final"], W[k]) for k in ("w_q", "w_dq", "w_ee")]
    J = 0.5 * W["w_u"] * (f64(r["u"]) ** 2).sum((2, 3))
    J += 0.5 * (wq[:, None] * (f64(r["q"]) - f64(goals["q_goal"])[:, None]) ** 2).sum((2, 3))
    J += 0.5 * (wdq[:, None] * (f64(r["dq"]) - f64(goals["dq_goal"])[:, None]) ** 2).sum((2, 3))
    J += 0.5 * (wee * ((f64(r["ee_pos"]) - f64(goals["ee_goal"])[:, None]) ** 2).sum(3)).sum(2)
    cost = f64(r["cost"])
    only = cfg.rollout_cost(u0, noise=noise[0], **goals)
    assert set(only) == {"cost", "terms", "status"} and (bits(N(only["cost"])) == bits(N(r["cost"]))).all()
    assert np.abs(f64(r["terms"]).sum(2) / cost - 1).max() < 1e-6
    return float((np.abs(cost - J) / J).max()), cap(T, 2 * n, cfg.sim.nu)


def case_mppi(make_sim, model, temperature):
    """Case 10b: MPPI_ITERS iterations of rollout_cost + mppi_update on MPPI_B envs with MPPI_K samples, sample 0 noise-free.
    temperature None: greedy (a temperature so small that the softmax is the argmin) -- the nominal's cost never increases and after
    each update it equals the chosen sample's cost, bit for bit.  Returns the nominal's cost before each iteration and after the
    last, [ITERS + 1, B]."""
    import torch
    cfg, u, goals, noise = mppi_problem(make_sim, model)
    N = lambda t: t.cpu().numpy()
    history, chosen = [], None
    for it in range(MPPI_ITERS + 1):
        r = cfg.rollout_cost(u, noise=noise[it % MPPI_ITERS], **goals)
        cost = r["cost"]
        assert (N(r["status"]) == 0).all()
        history.append(N(cost[:, 0]).copy())
        if temperature is None:
            if chosen is not None:
                assert (bits(history[-1]) == bits(chosen)).all(), (history[-1], chosen)
                assert (history[-1] <= history[-2]).all()
            if it == MPPI_ITERS:
                break
            u, w = cfg.mppi_update(u, noise[it], cost, 1e-30, status=r["status"])
            best = cost.argmin(1)
            assert torch.equal(w.argmax(1), best) and torch.equal(w.sum(1), torch.ones_like(w[:, 0])) and ((w == 0) | (w == 1)).all()
            chosen = N(cost.gather(1, best[:, None])[:, 0])
        elif it < MPPI_ITERS:
            u, w = cfg.mppi_update(u, noise[it], cost, temperature, status=r["status"])
            assert np.abs(N(w.sum(1)) - 1).max() < 1e-5
    return np.stack(history)
