"""The operational-space rollout kernel (mujoco_jaco_amd/csrc/rollout_osc.h, jaco_rollout_osc) under the wavefront emulator
(emu_rollout_osc of tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 reference (the oracle with contacts disabled, stepped by rollout_binding.oracle_rollout's substeps, the law
osc_binding.reference evaluated on the oracle's own state at each evaluation), the input sets -- rollout_binding.inputs' states and ctrl
rows (starts that open with a joint-limit row, gripper words in the base ctrl) plus seeded targets a few centimetres and tenths of a
radian from each start pose -- with the conditions they must meet asserted on the fp64 side, the cases shared by the CPU and the GPU
tier and the refusals.  emu_sim.EmuSim runs BatchedMujoco.rollout_osc and robot_config.BatchedOSC.rollout on the emulated call.

A tier hands the cases these calls:
  run(model, frames, target_pos [P, T, F, 3], target_quat [P, T, F, 4], ctrl=None, qpos0=None, qvel0=None, plan_index=None,
      state_index=None, nstates=None, frame=None, want=OUTS, hold=1, final_only=0, per_substep=1, handle=None, **gains) -> {output: array}
  run_open: rollout_fb_binding's (jaco_rollout on the same tier);
  run_osc(model, frames, qpos [B, nq], qvel [B, nv], target_pos [B, F, 3], target_quat [B, F, 4], ctrl_in [B, nu]) -> {"ctrl", "status"}:
      jaco_osc on the same tier;
  loop(model, frames, q, v, target_pos [n, T, F, 3], target_quat, base [n, T, nu]) -> {"qpos", "qvel" [n, T, ..], "ctrl" [n, T, nu]}:
      the loop the entry replaces on a contact-free handle: T x (get_state, jaco_osc, a one-substep step).
Every output array is handed in filled with SENTINEL (status: STATUS_SENTINEL), so what a call leaves untouched shows.
"""
import ctypes

import numpy as np

import fd_binding as fb
import ik_binding as ib
import osc_binding as ob
import rollout_binding as rb
import rollout_fb_binding as fbb
from fd_binding import bits, verr
from mujoco_jaco_amd import _lib as product_lib
from rollout_binding import same

OUTS = fbb.OUTS
STATE = fbb.STATE
SING0, SING1 = product_lib.JACO_ROLLOUT_OSC_SINGULAR0, product_lib.JACO_ROLLOUT_OSC_SINGULAR1
SING = SING0 | SING1
FLAG_NAN = product_lib.JACO_FLAG_NAN


def records(ptr, outs, frames, ctrl, tp, tq, pidx, nknots, hold, final_only, per_substep, nplans, nframes=None, opt_nframes=None, **gains):
    """(options, frame array or None, plan, out) records of one call; ptr(array or tensor or None) -> c_void_p or None."""
    nf = 0 if frames is None else len(frames)
    opt = product_lib.JacoRolloutOscOptions(nknots=nknots, hold=hold, final_only=final_only, per_substep=per_substep,
                                            nframes=(nf if nframes is None else nframes) if opt_nframes is None else opt_nframes, **gains)
    arr = None if frames is None else (product_lib.JacoFrame * max(nf, 1))(*frames)
    plan = product_lib.JacoRolloutOscPlan(ptr(ctrl), ptr(tp), ptr(tq), ptr(pidx), nplans)
    out = product_lib.JacoRolloutFbOut(*[ptr(outs.get(k)) for k in OUTS])
    return opt, arr, plan, out


def rollout_osc(model, frames, target_pos, target_quat, ctrl=None, qpos0=None, qvel0=None, plan_index=None, state_index=None, nstates=None, frame=None,
                want=OUTS, hold=1, final_only=0, per_substep=1, handle=None, n=None, nknots=None, nplans=None, nframes=None, opt_nframes=None, no_opt=False,
                no_out=False, no_plan=False, no_pos=False, no_quat=False, **gains):
    """Emulated jaco_rollout_osc: {output: array} in the C ABI's layout.  n / nknots / nplans / nframes override what the arrays say
    (refusals); no_* hand NULL pointers.  Raises ValueError with the library's message when the call is refused, with the outputs it was
    handed in .outputs."""
    L, blob, dims, num_envs, hq, hv = rb.emu_model(model, handle)
    p, ref = rb.HOST.ptr, rb.ref
    tp, tq, ctrl, q0, v0 = [rb.HOST.f32(a) for a in (target_pos, target_quat, ctrl, qpos0, qvel0)]
    pidx, sidx = rb.HOST.i32(plan_index), rb.HOST.i32(state_index)
    n, nknots, nstates, res = rb.prelude(rb.HOST, dims, want, tp.shape[0], tp.shape[1], q0, v0, num_envs, (pidx, sidx), n, nknots, nstates, hold, final_only,
                                         per_substep)
    opt, arr, plan, out = records(p, res, frames, ctrl, None if no_pos else tp, None if no_quat else tq, pidx, nknots, hold, final_only, per_substep,
                                  tp.shape[0] if nplans is None else nplans, nframes, opt_nframes, **gains)
    nf = (0 if frames is None else len(frames)) if nframes is None else nframes
    rc = L.emu_rollout_osc(blob, len(blob), ref(opt, no_opt), None if arr is None else ctypes.cast(arr, ctypes.c_void_p), nf, ref(frame), n, p(sidx), nstates,
                           p(q0), p(v0), ref(plan, no_plan), ref(out, no_out), num_envs, p(hq), p(hv))
    return rb.checked(L, rc, "emu_rollout_osc", res)


# ---- the models and their controlled frames
MODELS = (rb.MODEL,) + rb.SMALL
NAMES = {"jaco2_dual_torque": ("EE_1", "EE_2")}
N = rb.SMALL_B   # 9 rollouts on every model
DET_LO, DET_HI = 0.5e-3, 2e-3


def names_of(model):
    return NAMES.get(model, ("EE",))


def frames_of(model):
    """The controlled frames: each body with its COM as the point, so that the point is the fp64 reference's (mj_jacBodyCom)."""
    return [ib.table_of(model).jaco_frame(n) for n in names_of(model)]


def motors(model):
    """(the motor actuators of the active dofs of every frame, flat, in frame and dof order; the same per frame)."""
    mot = ob.motor_of(model)
    per = [[mot[d] for d in ob.active_dofs(model, n)] for n in names_of(model)]
    return [a for f in per for a in f], per


# ---- the fp64 reference
def oracle_closed_loop(model, q, v, base, target6, plan_index=None, state_index=None, hold=1, per_substep=1):
    """fp64, contacts disabled: rollout_binding.oracle_rollout's substeps with the ctrl of each evaluation = the base row with
    osc_binding.reference's u -- on the oracle's own state, its forward pass fresh -- at the motors of the active dofs.  {"qpos" [n, T, nq],
    "qvel" [n, T, nv]: the state after each knot; "u" [n, E, nu]: the commanded row of every evaluation; "det" [n, E, F]: |det(J M^-1 J^T)|
    there; "xpos" [n, T, 3]: the first frame's point after each knot}."""
    from oracle_binding import Oracle
    o = Oracle(model)
    o.option("disable_contact", 1)
    names = names_of(model)
    _, per = motors(model)
    P, T, F = target6.shape[:3]
    n = rb.count(P, (plan_index, state_index))
    E = T * (hold if per_substep else 1)
    r = dict(qpos=np.zeros((n, T, o.nq)), qvel=np.zeros((n, T, o.nv)), u=np.zeros((n, E, o.nu)), det=np.zeros((n, E, F)), xpos=np.zeros((n, T, 3)))
    tab = ib.table_of(model)
    for i in range(n):
        p = i if plan_index is None else int(plan_index[i])
        s = i if state_index is None else int(state_index[i])
        o.set("qpos", np.asarray(q[s], np.float64)); o.set("qvel", np.asarray(v[s], np.float64)); o.set("qacc_warmstart", np.zeros(o.nv))
        u = None
        for k in range(T):
            for sub in range(hold):
                if per_substep or sub == 0:
                    U, D, _ = ob.reference(model, names, o.get("qpos")[None], o.get("qvel")[None], target6[p, k][None])
                    u = np.zeros(o.nu) if base is None else np.asarray(base[p, k], np.float64).copy()
                    for f in range(F):
                        u[per[f]] = U[0, f, :len(per[f])]
                    e = k * hold + sub if per_substep else k
                    r["u"][i, e], r["det"][i, e] = u, D[0]
                o.step(u)
            r["qpos"][i, k], r["qvel"][i, k] = o.get("qpos"), o.get("qvel")
        r["xpos"][i] = ib.oracle_pose(model, names[0], tab.com(names[0]), r["qpos"][i])[0]
    return r


def check_reference(ref, singular=False):
    """The conditions on an input set, on the fp64 reference, over all rollouts and evaluations: the determinant outside [DET_LO, DET_HI]
    so that the fp32 and the fp64 branch cannot differ -- above DET_HI throughout in the regular sets, where the singular bit must stay
    clear, below DET_LO throughout in the singular set, where it must be set -- and a finite rollout."""
    d = ref["det"]
    if singular:
        assert (d < DET_LO).all(), d.max()
    else:
        assert (d > DET_HI).all(), d.min()
    assert np.isfinite(ref["qpos"]).all() and np.isfinite(ref["qvel"]).all() and (np.abs(ref["qvel"]) < 1e10).all()


# ---- inputs
TARGET_DIST, TARGET_ANG = (0.03, 0.08), (0.1, 0.3)   # m, rad from the start pose: a few centimetres, as a planner samples them
_shared = {}


def targets(model, q, T, seed=81):
    """[n, T, F, 6] targets (position + 'rxyz' Euler angles): per knot and frame a fresh draw of osc_binding.offset_targets about the START
    pose of the frame's body."""
    names = names_of(model)
    return np.stack([np.stack([ob.offset_targets(model, nm, q, TARGET_DIST, TARGET_ANG, seed + 10 * k + f) for f, nm in enumerate(names)], 1) for k in range(T)], 1)


def regular_inputs(model, n, T, spare=3):
    """The first n of rollout_binding.inputs(model, n + spare, T) whose START has fp64 |det(J M^-1 J^T)| > DET_HI for every controlled
    frame (rollout 3 of that draw starts with a straight elbow: 3.7e-5); at least two of them open with a joint-limit row."""
    q, v, c = rb.inputs(model, n + spare, T)
    D = ob.reference(model, names_of(model), q, v, np.zeros((len(q), len(names_of(model)), 6)))[1]
    keep = np.flatnonzero((D > DET_HI).all(1))[:n]
    assert len(keep) == n and (keep % 3 == 0).sum() >= 2, keep
    return q[keep], v[keep], c[keep]


def shared(model, long=False):
    """The inputs of a model -- regular_inputs(model, 9, 6) at hold 3 (long: LONG_B rollouts of LONG_KNOTS x 1 on the arm-only
    model), targets, the kernel's fp32 targets -- and the fp64 reference in both modes; computed once per process, conditions asserted."""
    key = (model, long)
    if key not in _shared:
        n, T, hold = (rb.LONG_B, rb.LONG_KNOTS, 1) if long else (N, rb.KNOTS, rb.HOLD)
        q, v, c = regular_inputs(model, n, T)
        t6 = targets(model, q, T)
        tp, tq = ob.kernel_targets(t6)
        g = dict(q=q, v=v, c=c, hold=hold, t6=t6, tp=tp, tq=tq, frames=frames_of(model), ee=rb.frames(model)[1], ref={})
        for mode in ((1,) if long else (0, 1)):
            g["ref"][mode] = oracle_closed_loop(model, q, v, c, t6, hold=hold, per_substep=mode)
            check_reference(g["ref"][mode])
        servo = fb.tables(model)["position"]
        assert servo.any() and (c[:, :, servo] != 0).all()   # (gripper words in the base ctrl)
        _shared[key] = g
    return _shared[key]


SINGULAR_MODEL, SINGULAR_B, SINGULAR_KNOTS = "jaco2_curtain_torque", 4, 2


def singular():
    """The singular set: osc_binding.singular_states with zero velocities, 2 knots x hold 1, targets at the start pose's distance draws."""
    if "singular" not in _shared:
        q, v = ob.singular_states(SINGULAR_MODEL, "EE", want=SINGULAR_B)
        v = np.zeros_like(v)
        t6 = targets(SINGULAR_MODEL, q, SINGULAR_KNOTS, seed=83)
        tp, tq = ob.kernel_targets(t6)
        g = dict(q=q, v=v, t6=t6, tp=tp, tq=tq, frames=frames_of(SINGULAR_MODEL))
        g["ref"] = oracle_closed_loop(SINGULAR_MODEL, q, v, None, t6)
        check_reference(g["ref"], singular=True)
        _shared["singular"] = g
    return _shared["singular"]


def args(g, sl=slice(None)):
    return dict(target_pos=g["tp"][sl], target_quat=g["tq"][sl], ctrl=g["c"][sl])


def call(run, model, per_substep=1, long=False):
    """The call on shared(model, long) in one mode with every output, made once per tier (kept on the tier's `run`)."""
    memo = run.__dict__.setdefault("_osc_calls", {})
    key = (model, per_substep, long)
    if key not in memo:
        g = shared(model, long)
        memo[key] = run(model, g["frames"], qpos0=g["q"], qvel0=g["v"], frame=g["ee"], hold=g["hold"], per_substep=per_substep, **args(g))
    return memo[key]


# ---- the cases
def case_own_commands(run, run_open, model, per_substep, long=False):
    """Case 1: an OSC rollout is an open loop on its own commands -- the ctrl output fed to jaco_rollout from the same states reproduces
    qpos, qvel, xpos, xmat and (the singular bits masked) status bit for bit; the regular sets leave the singular bits clear."""
    g = shared(model, long)
    hold = g["hold"]
    r = call(run, model, per_substep, long)
    assert (r["status"] == 0).all(), r["status"]
    if per_substep:
        o = run_open(model, r["ctrl"], g["q"], g["v"], frame=g["ee"], hold=1)
        o = {k: (x if k == "status" else x[:, hold - 1::hold]) for k, x in o.items()}
    else:
        o = run_open(model, r["ctrl"], g["q"], g["v"], frame=g["ee"], hold=hold)
    same(o, dict(r, status=r["status"] & ~np.uint32(SING)), rb.OUTS)


def case_first_evaluation(run, run_osc, model):
    """Case 2: the first evaluation is jaco_osc on the start state with the base row as ctrl_in, bit for bit, in both modes; the
    singular bits of a one-evaluation call equal jaco_osc's status, and no other bit but JACO_FLAG_NAN / _SOLVER_MAXITER can be set."""
    g = shared(model)
    o = run_osc(model, g["frames"], g["q"], g["v"], g["tp"][:, 0], g["tq"][:, 0], g["c"][:, 0])
    for mode in (0, 1):
        r = call(run, model, mode)
        assert (bits(r["ctrl"][:, 0]) == bits(o["ctrl"])).all()
    one = run(model, g["frames"], g["tp"][:, :1], g["tq"][:, :1], g["c"][:, :1], g["q"], g["v"], want=("status", "ctrl"))
    assert (bits(one["ctrl"][:, 0]) == bits(o["ctrl"])).all()
    sing = sum((o["status"][:, f] != 0).astype(np.uint32) * np.uint32(SING0 << f) for f in range(o["status"].shape[1]))
    assert ((one["status"] & SING) == sing).all() and (one["status"] & ~np.uint32(SING | 24) == 0).all()


def case_singular(run, run_osc):
    """The singular set: the determinant of the fp64 reference is below DET_LO at every evaluation, so frame 0's singular bit must be
    set (and frame 1's clear); the first evaluation is still jaco_osc's, status included.  Returns the ctrl measure against fp64."""
    g = singular()
    r = run(SINGULAR_MODEL, g["frames"], g["tp"], g["tq"], None, g["q"], g["v"], want=STATE + ("ctrl",))
    assert ((r["status"] & SING) == SING0).all(), r["status"]
    o = run_osc(SINGULAR_MODEL, g["frames"], g["q"], g["v"], g["tp"][:, 0], g["tq"][:, 0], None)
    assert (o["status"] != 0).all() and (bits(r["ctrl"][:, 0]) == bits(o["ctrl"])).all()
    mot, _ = motors(SINGULAR_MODEL)
    return float(ob.error(r["ctrl"][..., mot], g["ref"]["u"][..., mot]).max())


def case_loop(run, loop, model, bitwise):
    """Case 3: hold 1 per_substep against the loop the entry replaces (get_state, jaco_osc, a one-substep contact-free step) on the same
    tier; run and loop work on the same handle.  bitwise (a handle with option compensated = 0: the walk reads no low words, so every
    evaluation is jaco_osc): states and commands bit for bit.  Otherwise (compensated on: jaco_osc sees the high words only) returns the (qpos, qvel, ctrl) measures."""
    g = shared(model)
    T = g["tp"].shape[1]
    r = run(model, g["frames"], qpos0=g["q"], qvel0=g["v"], hold=1, per_substep=1, want=STATE + ("ctrl",), **args(g))
    o = loop(model, g["frames"], g["q"], g["v"], g["tp"], g["tq"], g["c"])
    assert r["ctrl"].shape == o["ctrl"].shape == (len(g["q"]), T, g["c"].shape[2])
    assert (bits(r["ctrl"][:, 0]) == bits(o["ctrl"][:, 0])).all()
    if bitwise:
        same(o, r, ("qpos", "qvel", "ctrl"))
        return 0.0, 0.0, 0.0
    mot, _ = motors(model)
    return verr(r["qpos"], o["qpos"]), verr(r["qvel"], o["qvel"]), float(ob.error(r["ctrl"][..., mot], o["ctrl"][..., mot]).max())


def case_oracle(run, model, per_substep=1, long=False):
    """Against fp64: every knot's qpos, qvel and output-frame position, and the commanded ctrl on the active dofs, against the fp64
    closed loop.  Returns (qpos, qvel, ctrl, xpos) measures: rollout_fb's verr on states, osc_binding.error on ctrl."""
    g = shared(model, long)
    ref = g["ref"][per_substep]
    r = call(run, model, per_substep, long)
    assert (r["status"] == 0).all(), r["status"]
    mot, _ = motors(model)
    name = names_of(model)[0]
    # (the output frame is rollout_binding's EE frame: the body's origin, fp64, at the reference's knot states)
    xp = np.stack([ib.oracle_pose(model, name, np.zeros(3), ref["qpos"][i])[0] for i in range(len(ref["qpos"]))])
    return (verr(r["qpos"], ref["qpos"]), verr(r["qvel"], ref["qvel"]), float(ob.error(r["ctrl"][..., mot], ref["u"][..., mot]).max()), verr(r["xpos"], xp))


FAN = (3, 4)   # plans x states


def case_fan_out(run, model=rb.MODEL):
    """Case 4: 3 plans x 4 states through plan_idx and state_idx against the same rollouts with materialised plans and states, bit for
    bit; shuffling the rollouts permutes the rows.  Both modes."""
    g = shared(model)
    P, S = FAN
    pi, si = [x.reshape(-1) for x in np.meshgrid(np.arange(P), np.arange(S), indexing="ij")]
    for mode in (0, 1):
        k = dict(frame=g["ee"], hold=g["hold"], per_substep=mode)
        r = run(model, g["frames"], qpos0=g["q"][:S], qvel0=g["v"][:S], plan_index=pi, state_index=si, **args(g, slice(0, P)), **k)
        assert len(np.unique(bits(r["qpos"][:, -1]), axis=0)) == P * S
        same(run(model, g["frames"], qpos0=g["q"][si], qvel0=g["v"][si], **args(g, pi), **k), r)
        perm = np.random.default_rng(5).permutation(len(pi))
        s = run(model, g["frames"], qpos0=g["q"][:S], qvel0=g["v"][:S], plan_index=pi[perm], state_index=si[perm], **args(g, slice(0, P)), **k)
        same(s, {key: x[perm] for key, x in r.items()})


def case_independence(run, model=rb.MODEL):
    """Case 5: outputs do not depend on which other outputs are asked for or on final_only; the handle's state serves as the states; two
    calls agree.  Both modes."""
    g = shared(model)
    for mode in (0, 1):
        full = call(run, model, mode)
        k = dict(qpos0=g["q"], qvel0=g["v"], hold=g["hold"], per_substep=mode, **args(g))
        same(run(model, g["frames"], frame=g["ee"], **k), full)
        for key in OUTS:
            alone = run(model, g["frames"], frame=g["ee"] if key in ("xpos", "xmat") else None, want=(key,), **k)
            assert set(alone) == {key}
            same(alone, full, (key,))
        last = run(model, g["frames"], frame=g["ee"], final_only=1, **k)
        same(last, {key: (x if key in ("status", "ctrl") else x[:, -1:]) for key, x in full.items()})
        same(run(model, g["frames"], frame=g["ee"], handle=(g["q"], g["v"]), hold=g["hold"], per_substep=mode, **args(g)), full)


def case_pass_through(run, model):
    """Case 6: every ctrl word that is not the motor of an active dof passes through bitwise, on every evaluation; a NULL base ctrl is
    zeros there, and the first evaluation's motor words do not depend on the base row."""
    g = shared(model)
    mot, _ = motors(model)
    other = np.setdiff1d(np.arange(g["c"].shape[2]), mot)
    assert len(other) > 0
    for mode in (0, 1):
        r = call(run, model, mode)
        base = np.repeat(g["c"], g["hold"], 1) if mode else g["c"]
        assert (bits(r["ctrl"][..., other]) == bits(base[..., other])).all()
        assert not (bits(r["ctrl"][..., mot]) == bits(base[..., mot])).any(-1).all()
    z = run(model, g["frames"], g["tp"], g["tq"], None, g["q"], g["v"], hold=g["hold"], want=("ctrl",))
    assert (bits(z["ctrl"][..., other]) == 0).all()
    assert (bits(z["ctrl"][:, 0][..., mot]) == bits(call(run, model, 1)["ctrl"][:, 0][..., mot])).all()


def case_bad_index(run, model=rb.MODEL):
    """plan_idx and state_idx entries -1 and one past the end among valid ones: JACO_ROLLOUT_BAD_INDEX in their status words, their rows
    untouched (ctrl included), every other rollout bitwise what it is without the bad entries."""
    g = shared(model)
    m, P = rb.BAD_STATES, rb.BAD_PLANS
    k = dict(qpos0=g["q"][:m], qvel0=g["v"][:m], frame=g["ee"], hold=g["hold"], **args(g, slice(0, P)))
    rb.bad_index(lambda keep, **index: run(model, g["frames"], **index, **k), OUTS, plans=True)


# ---- the refusals: one argument set per JACO_EINVAL case of include/jaco_env.h, for the emulator's entry and the library's alike
REFUSAL_MODEL = rb.REFUSAL_MODEL
REFUSALS = {k: v for k, v in rb.REFUSALS.items() if k not in ("status_only", "null_ctrl")}   # (status alone is an output; a NULL ctrl is zeros)
REFUSALS.update({
    "no_outputs": "at least one of the outputs qpos, qvel, xpos, xmat, status and ctrl is required",
    "null_plan": "the plan is required",
    "per_substep_2": "per_substep must be 0 or 1",
    "nplans_0": "nplans 0: at least one plan is required",
    "n_beyond_nplans": "n 4 rollouts from 3 plans without a plan index",
    "nframes_mismatch": "nframes 1 but the options' nframes 2",
    "nframes_0": "nframes 0 outside [1, 2]",
    "nframes_3": "nframes 3 outside [1, 2]",
    "null_target_pos": "the target positions and the target quaternions are required",
    "null_target_quat": "the target positions and the target quaternions are required",
    "gain": "kp, ko, kv, vmax_xyz and vmax_abg must be positive",
    "frame_body_high": "frame 0: body 11 outside [0, 11)",
    "frame_world": "frame 0: body -1 outside [0, 11)",
    "empty": "frame 0: empty active dof set (a free body's frame, or a dof_mask that removes the whole chain)",
})


def refusal_args(case):
    """Keyword arguments of one refused call of `rollout_osc` / the GPU tier's twin on REFUSAL_MODEL: REFUSAL_N plans of 2 knots."""
    g = shared(REFUSAL_MODEL)
    n = rb.REFUSAL_N
    k = dict(frames=g["frames"], target_pos=g["tp"][:n, :2], target_quat=g["tq"][:n, :2], ctrl=g["c"][:n, :2], qpos0=g["q"][:n], qvel0=g["v"][:n],
             want=("qpos", "status", "ctrl"))
    if case in rb.REFUSALS:
        r = rb.refusal_args(case)
        r.pop("ctrl")
        if "want" in r and case != "pose_without_frame":
            r.pop("want")
        return dict(k, **r)

    def body(b):
        f = product_lib.JacoFrame()
        f.body = b
        return [f]
    k.update({"no_outputs": dict(want=()), "null_plan": dict(no_plan=True), "per_substep_2": dict(per_substep=2), "nplans_0": dict(nplans=0, plan_index=np.zeros(n, np.int32)),
              "n_beyond_nplans": dict(target_pos=g["tp"][:3, :2], target_quat=g["tq"][:3, :2], ctrl=g["c"][:3, :2], n=n), "nframes_mismatch": dict(opt_nframes=2),
              "nframes_0": dict(nframes=0), "nframes_3": dict(nframes=3), "null_target_pos": dict(no_pos=True), "null_target_quat": dict(no_quat=True),
              "gain": dict(kv=0.0), "frame_body_high": dict(frames=body(11)), "frame_world": dict(frames=body(-1)),
              "empty": dict(dof_mask=1 << 20)}[case])
    return k


# ---- the Python tiers.  make_sim(model, qpos, qvel) -> a BatchedMujoco (GPU tier) or emu_sim.EmuSim.
CONFIG_MODELS = {"jaco2_reaching_torque": ("EE",), "jaco2_dual_torque": ("EE_1", "EE_2")}
CONFIG_K, CONFIG_T, CONFIG_HOLD = 3, 4, 2


def case_config(make_sim, model):
    """BatchedOSC.rollout on K = 3 target sequences per env, every target the CURRENT pose of its frame (fp64 oracle pose at the start,
    zero start velocity): the fp64 reference holds the arm (asserted first: its joints move less than HOLD_REF), and the kernel's
    joints stay within the returned measure of the reference's.  The documented shapes; the result equals the sim-tier call bit for
    bit; a controller built with ctrlr_dof or null_controllers is refused.  Returns the q measure (verr against the fp64 reference)."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, BatchedOSC, Damping
    import glue
    from mujoco_jaco_amd.modelc import rot
    names = CONFIG_MODELS[model]
    q, v = fbb.hold_postures(model)
    v = np.zeros_like(v)
    B = len(q)
    tab = ib.table_of(model)
    t6 = np.zeros((B, len(names), 6))
    for f, nm in enumerate(names):   # (the controller's point is the body origin: point = 0)
        P, R = ib.oracle_pose(model, nm, np.zeros(3), q)
        t6[:, f, :3] = P.astype(np.float32)
        t6[:, f, 3:] = [glue.euler_from_quat(rot.mat_to_quat(R[e])) for e in range(B)]
    sim = make_sim(model, q, v)
    cfg = BatchedMujocoConfig(sim, ee=names[0])
    osc = BatchedOSC(cfg, names=names)
    target = np.broadcast_to(t6[:, None, None], (B, CONFIG_K, CONFIG_T, len(names), 6))
    if len(names) == 1:
        target = target[:, :, :, 0]
    servo = fb.tables(model)["position"]
    base = np.zeros((B, sim.nu), np.float32)
    base[:, servo] = q[:, fb.tables(model)["qadr"][servo]]   # (the grippers commanded to where they are)
    r = osc.rollout(torch.as_tensor(np.ascontiguousarray(target), dtype=torch.float32, device=sim.device), hold=CONFIG_HOLD, ctrl=torch.as_tensor(base, device=sim.device))
    nJ, E = len(cfg.arm), CONFIG_T * CONFIG_HOLD
    assert r["q"].shape == (B, CONFIG_K, CONFIG_T, nJ) and r["dq"].shape == (B, CONFIG_K, CONFIG_T, nJ) and r["status"].shape == (B, CONFIG_K)
    assert r["ee_pos"].shape == (B, CONFIG_K, CONFIG_T, 3) and r["ee_mat"].shape == (B, CONFIG_K, CONFIG_T, 9) and r["u"].shape == (B, CONFIG_K, E, sim.nu)
    A = lambda t: t.cpu().numpy()
    from mujoco_jaco_amd.robot_config import quat_from_euler_rxyz
    tt = torch.as_tensor(np.ascontiguousarray(target), dtype=torch.float32, device=sim.device).reshape(B * CONFIG_K, CONFIG_T, len(names), 6)
    raw = sim.rollout_osc(osc.frames, tt[..., :3], quat_from_euler_rxyz(tt[..., 3:]), ctrl=torch.as_tensor(np.repeat(base, CONFIG_K, 0)[:, None].repeat(CONFIG_T, 1), device=sim.device),
                          state_index=np.repeat(np.arange(B), CONFIG_K), hold=CONFIG_HOLD, frame=osc.frames[0])
    assert (bits(A(r["q"]).reshape(B * CONFIG_K, CONFIG_T, nJ)) == bits(A(raw["qpos"])[..., list(cfg.arm_qadr)])).all()
    assert (bits(A(r["u"]).reshape(B * CONFIG_K, E, -1)) == bits(A(raw["ctrl"]))).all() and (bits(A(r["ee_pos"]).reshape(-1, 3)) == bits(A(raw["xpos"]).reshape(-1, 3))).all()
    assert (A(r["status"]).reshape(-1) == A(raw["status"])).all()
    assert (bits(A(r["q"])[:, 0]) == bits(A(r["q"])[:, 1])).all()   # (the K candidates share state and targets here)
    ref = oracle_closed_loop(model, q, v, np.broadcast_to(base[:, None], (B, CONFIG_T, sim.nu)), np.broadcast_to(t6[:, None], (B, CONFIG_T, len(names), 6)),
                             hold=CONFIG_HOLD, per_substep=1)
    check_reference(ref)
    moved = np.abs(ref["qpos"][:, :, list(cfg.arm_qadr)] - q[:, None, list(cfg.arm_qadr)].astype(np.float64)).max()
    assert moved < HOLD_REF, moved
    for bad in (dict(ctrlr_dof=[True, True, True, False, False, False]), dict(null_controllers=[Damping(1.0)])):
        try:
            BatchedOSC(cfg, names=names, **bad).rollout(torch.as_tensor(np.ascontiguousarray(target), dtype=torch.float32, device=sim.device))
        except ValueError as e:
            assert "plain controller" in str(e)
        else:
            raise AssertionError("a controller with %s must be refused" % sorted(bad))
    return verr(A(r["q"])[:, 0], ref["qpos"][:, :, list(cfg.arm_qadr)])


HOLD_REF = 1e-4   # rad: what the fp64 reference's arm moves in 8 substeps of holding its own pose (fp32 targets: not exactly its pose)
