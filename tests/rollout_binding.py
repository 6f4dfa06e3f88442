"""The rollout kernel (mujoco_jaco_amd/csrc/rollout.h, jaco_rollout) under the wavefront emulator (emu_rollout of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 reference (the oracle with contacts disabled: per rollout qpos / qvel and a zero warm start, then step(ctrl_k, hold) per
knot), the input sets with the conditions they must meet asserted on the fp64 side, the cases shared by the CPU and the GPU tier, the
refusals.  emu_sim.EmuSim runs BatchedMujoco.rollout on the emulated call (CPU tests of robot_config).  And what the four entries of
the family (jaco_rollout, _fb, _cost, _osc) share on both tiers: the prelude of a call (Tier, prelude) and the bad-index case (bad_index).

A tier hands the cases its `run`:
  run(model, ctrl [n, T, nu], qpos0=None, qvel0=None, state_index=None, nstates=None, frame=None, want=OUTS, hold=1, final_only=0,
      handle=None) -> {output: array}
qpos0 / qvel0 None: the handle's state, which is handle = (qpos [num_envs, nq], qvel [num_envs, nv]).  Every output array is handed in
filled with SENTINEL (status: STATUS_SENTINEL), so what a call leaves untouched shows.
"""
import ctypes

import numpy as np

import emu_binding
import fd_binding as fb
import ik_binding as ib
import osc_binding as ob
from fd_binding import bits, verr
from mujoco_jaco_amd import _lib as product_lib

OUTS = ("qpos", "qvel", "xpos", "xmat", "status")
SENTINEL, STATUS_SENTINEL = 7.0, 0x7777
BAD_INDEX = product_lib.JACO_ROLLOUT_BAD_INDEX


# ---- what every call of the rollout family does before its one foreign call, for the four emulated entries (rollout here, rollout_fb,
# rollout_cost, rollout_osc of their *_binding.py files) and for their GPU twins (the abi_call of tests/test_gpu_rollout*.py)
class Tier:
    """What the two tiers of a call differ in.  array(a, dtype) -> a as the tier's contiguous array of that numpy dtype; full(shape,
    value, dtype) -> an array filled with value; address(array) -> where it lies, as a c_void_p; min_rows: the rollouts the outputs have
    rows for when n <= 0 (the emulator: none; the GPU: one, so that no output pointer is NULL)."""

    def __init__(self, array, full, address, min_rows):
        self.array, self.full, self.address, self.min_rows = array, full, address, min_rows

    def f32(self, a):
        return None if a is None else self.array(a, np.float32)

    def i32(self, a):
        return None if a is None else self.array(a, np.int32)

    def ptr(self, a):
        return None if a is None else self.address(a)

    def blank(self, shape, status=False):
        """An output array as a call is handed it: the sentinel in every word."""
        return self.full(shape, STATUS_SENTINEL, np.uint32) if status else self.full(shape, SENTINEL, np.float32)


HOST = Tier(np.ascontiguousarray, np.full, lambda a: ctypes.c_void_p(a.ctypes.data), 0)


def ref(record, absent=False):
    """The address of a ctypes record (or of an array of them) as the C ABI's untyped pointer; NULL for None or with `absent`."""
    return None if record is None or absent else ctypes.cast(ctypes.pointer(record), ctypes.c_void_p)


def count(nplans, per_rollout=(), n=None):
    """n of a call: given, or the length of the first per-rollout array that is there, or the number of plans."""
    if n is not None:
        return n
    for a in per_rollout:
        if a is not None:
            return len(a)
    return nplans


def shapes(n, rows, evals, nq, nv, nu):
    """The family's outputs: jaco_rollout's five, "ctrl" of the closed loops, "cost" and "terms" of the costed one."""
    return {"qpos": (n, rows, nq), "qvel": (n, rows, nv), "xpos": (n, rows, 3), "xmat": (n, rows, 9), "status": (n,), "ctrl": (n, evals, nu),
            "cost": (n,), "terms": (n, 3)}


def prelude(tier, dims, want, nplans, knots, q0, v0, num_envs, per_rollout=(), n=None, nknots=None, nstates=None, hold=1, final_only=0, per_substep=0):
    """(n, nknots, nstates, {output in `want`: the tier's array, sentinel-filled}) of one call.  dims = (nq, nv, nu); nplans, knots: what
    the plan arrays say; q0 / v0: the tier's state override arrays or None; num_envs: the handle's; per_rollout: the tier's per-rollout
    arrays in the order their length decides n; n / nknots / nstates: the overrides (refusals)."""
    n = count(nplans, per_rollout, n)
    nknots = knots if nknots is None else nknots
    if nstates is None:
        nstates = q0.shape[0] if q0 is not None else (v0.shape[0] if v0 is not None else num_envs)
    rows = 1 if final_only == 1 else max(nknots, 1)
    evals = max(nknots, 1) * (max(hold, 1) if per_substep == 1 else 1)
    sh = shapes(max(n, tier.min_rows), rows, evals, *dims)
    return n, nknots, nstates, {k: tier.blank(sh[k], k == "status") for k in want}


def emu_model(model, handle):
    """What an emulated call needs of its model and its handle: (the layout's library, the blob, (nq, nv, nu), num_envs, the handle's fp32
    qpos, qvel); handle None: no envs, NULL state."""
    blob, layout, nu = ob._model_info(model)
    M = ib.load_model(model)
    hq, hv = (None, None) if handle is None else (HOST.f32(handle[0]), HOST.f32(handle[1]))
    return emu_binding.lib(layout), blob, (int(M["nq"][0]), int(M["nv"][0]), nu), 0 if hq is None else hq.shape[0], hq, hv


def checked(L, rc, entry, res):
    """res, or the refusal's ValueError with the outputs the call was handed in .outputs."""
    try:
        emu_binding.check(L, rc, entry)
    except ValueError as e:
        e.outputs = res
        raise
    return res


def rollout(model, ctrl, qpos0=None, qvel0=None, state_index=None, nstates=None, frame=None, want=OUTS, hold=1, final_only=0, handle=None,
            n=None, nknots=None, no_opt=False, no_out=False, no_ctrl=False):
    """Emulated jaco_rollout: {output: array} in the C ABI's layout.  n / nknots: override what the ctrl array says (refusals);
    no_opt / no_out / no_ctrl hand NULL pointers.  Raises ValueError with the library's message when the call is refused, with the
    outputs it was handed in .outputs."""
    L, blob, dims, num_envs, hq, hv = emu_model(model, handle)
    p = HOST.ptr
    ctrl, q0, v0, idx = HOST.f32(ctrl), HOST.f32(qpos0), HOST.f32(qvel0), HOST.i32(state_index)
    n, nknots, nstates, res = prelude(HOST, dims, want, ctrl.shape[0], ctrl.shape[1], q0, v0, num_envs, n=n, nknots=nknots, nstates=nstates, hold=hold,
                                      final_only=final_only)
    out = product_lib.JacoRolloutOut(*[p(res.get(k)) for k in OUTS])
    opt = product_lib.JacoRolloutOptions(nknots=nknots, hold=hold, final_only=final_only)
    rc = L.emu_rollout(blob, len(blob), ref(opt, no_opt), ref(frame), n, p(idx), nstates, p(q0), p(v0), None if no_ctrl else p(ctrl), ref(out, no_out),
                       num_envs, p(hq), p(hv))
    return checked(L, rc, "emu_rollout", res)


def emu_steps(model, q, v, ctrl, hold):
    """The emulated contact-free step kernel as a handle runs it -- set_state(q, v, zeros), then send_forces(ctrl_k, hold) + get_state per
    knot, the compensated low words kept between the calls as the library keeps them: (qpos [n, T, nq], qvel [n, T, nv], flags [n])."""
    blob, layout, nu = ob._model_info(model)
    L = emu_binding.lib(layout)
    q, v = np.array(q, np.float32), np.array(v, np.float32)
    n, T = ctrl.shape[0], ctrl.shape[1]
    ws, ql, vl = np.zeros_like(v), np.zeros_like(q), np.zeros_like(v)
    flags = np.zeros(n, np.uint32)
    Q, V = np.zeros((n, T, q.shape[1]), np.float32), np.zeros((n, T, v.shape[1]), np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for k in range(T):
        c = np.ascontiguousarray(ctrl[:, k], np.float32)
        emu_binding.check(L, L.emu_step_lo(blob, len(blob), n, hold, p(q), p(v), p(ws), p(ql), p(vl), p(c), p(flags)), "emu_step_lo")
        Q[:, k], V[:, k] = q, v
    return Q, V, flags


# ---- the fp64 reference
def limit_table(model):
    """(qpos addresses, lower, upper) of the limited hinge joints."""
    M = ib.load_model(model)
    nj = int(M["njnt"][0])
    lim = [j for j in range(nj) if int(M["jnt_type"][j]) == 3 and int(M["jnt_limited"][j])]
    rng = np.asarray(M["jnt_range"], float).reshape(-1, 2)
    return np.array([int(M["jnt_qposadr"][j]) for j in lim]), rng[lim, 0], rng[lim, 1]


def oracle_rollout(model, q, v, ctrl, hold):
    """fp64, contacts disabled: {"qpos" [n, T, nq], "qvel" [n, T, nv]: the state after each knot; "before" [n, T * hold, nq]: qpos at the
    start of each substep; "nefc" [n, T * hold]: the constraint rows (= limit rows) of each substep}."""
    from oracle_binding import Oracle
    o = Oracle(model)
    o.option("disable_contact", 1)
    n, T = ctrl.shape[0], ctrl.shape[1]
    r = dict(qpos=np.zeros((n, T, o.nq)), qvel=np.zeros((n, T, o.nv)), before=np.zeros((n, T * hold, o.nq)), nefc=np.zeros((n, T * hold), int))
    for i in range(n):
        o.set("qpos", np.asarray(q[i], np.float64)); o.set("qvel", np.asarray(v[i], np.float64)); o.set("qacc_warmstart", np.zeros(o.nv))
        for k in range(T):
            for s in range(hold):
                r["before"][i, k * hold + s] = o.get("qpos")
                o.step(np.asarray(ctrl[i, k], np.float64))
                r["nefc"][i, k * hold + s] = o.nefc
            r["qpos"][i, k], r["qvel"][i, k] = o.get("qpos"), o.get("qvel")
    return r


ULP_2PI = 2.0 ** -21   # the fp32 spacing at the joint angles' magnitude (4 <= |q| < 8)


def check_inputs(model, ctrl, hold, ref):
    """What the issue asks of the inputs, on the fp64 side: limit rows active in at least a fifth of the rollouts and in none of at least
    a fifth; every substep off the actuator model's knife edges; no limit row within the margin of its threshold at any substep.  The
    margin: one fp32 spacing of a joint angle per substep taken so far (the two paths can drift apart by a rounding per substep)."""
    adr, lo, hi = limit_table(model)
    n, nsub = ref["nefc"].shape
    active = (ref["nefc"] > 0).any(1)
    assert active.mean() >= 0.2 and (~active).mean() >= 0.2, (model, active.mean())
    for t in range(nsub):
        assert fb.off_the_knife_edges(model, ref["before"][:, t], ctrl[:, t // hold]), (model, t)
        ql = ref["before"][:, t][:, adr]
        dist = np.minimum(ql - lo, hi - ql)
        assert ((dist < 0).sum(1) == ref["nefc"][:, t]).all(), (model, t)      # (the oracle's rows are the limit rows, threshold 0)
        assert np.abs(dist).min() > (t + 1) * ULP_2PI, (model, t, np.abs(dist).min())
    return active


# ---- inputs
MODEL, B = "jaco2_curtain_torque", 67
SMALL = ("jaco2_dual_torque", "jaco2_curtain_torque_old", "jaco2_reaching_torque")
SMALL_B = 9
KNOTS, HOLD = 6, 3
LONG_MODEL, LONG_B, LONG_KNOTS = "jaco2_reaching_torque", 8, 50
PUSH = 0.03     # rad beyond a limit, for the rollouts that start with a limit row
INSIDE = 0.15   # rad inside both limits, for the rollouts that must have none


def inputs(model, n, nknots, seed=61):
    """(qpos [n, nq], qvel [n, nv], ctrl [n, nknots, nu]) fp32, drawn like fd_binding.shared: its states and ctrl rows (motor commands
    uniform in +-5, the servo commands kp |delta| = 0.02 .. 0.16 away from the finger angles), then
      * the servo-driven joints moved at least 0.05 rad inside their joint range (a limit row would push the finger through the
        servo's forcerange: a knife edge), the servo commands moved with them;
      * rollout i with i % 3 == 0: one motor-driven limited arm joint PUSH beyond its lower or upper limit (a limit row from the start);
      * i % 3 == 1: every limited joint at least INSIDE from both limits (no limit row);  i % 3 == 2: as drawn;
      * the later knots: fresh motor commands; the servo commands stay (the undamped proximal finger joints of the 12-hinge model swing
        about their command: with a fixed command the servo force stays inside its first value, off the forcerange)."""
    T = fb.tables(model)
    q, v, c0 = fb.inputs(model, n)
    q, c0 = q.astype(np.float64), c0.astype(np.float64)
    adr, lo, hi = limit_table(model)
    servo = np.flatnonzero(T["position"])
    sq = T["qadr"][servo]
    delta = c0[:, servo] - q[:, sq]
    for a, j in zip(sq, [int(np.flatnonzero(adr == a)[0]) for a in sq]):
        q[:, a] = np.clip(q[:, a], lo[j] + 0.05, hi[j] - 0.05)
    arm = [j for j in range(len(adr)) if adr[j] not in sq and adr[j] in T["qadr"]]   # limited joints with a motor
    for i in range(n):
        if i % 3 == 0:
            j = arm[(i // 3) % len(arm)]
            q[i, adr[j]] = lo[j] - PUSH if (i // 3) % 2 == 0 else hi[j] + PUSH
        elif i % 3 == 1:
            q[i, adr] = np.clip(q[i, adr], lo + INSIDE, hi - INSIDE)
    q = q.astype(np.float32)
    rng = np.random.default_rng(seed)
    c = rng.uniform(-5, 5, (n, nknots, c0.shape[1]))
    c[:, 0] = c0
    c[:, :, servo] = (q[:, sq].astype(np.float64) + delta)[:, None]
    return q, v, c.astype(np.float32)


_shared = {}


def shared(model, long=False):
    """The inputs of a model (KNOTS x HOLD; long: LONG_KNOTS x 1 on LONG_B rollouts), their fp64 reference and which rollouts have a
    limit row over the horizon; computed once per process, conditions asserted."""
    key = (model, long)
    if key not in _shared:
        n, T, hold = (LONG_B, LONG_KNOTS, 1) if long else (B if model == MODEL else SMALL_B, KNOTS, HOLD)
        q, v, c = inputs(model, n, T)
        ref = oracle_rollout(model, q, v, c, hold)
        _shared[key] = dict(q=q, v=v, c=c, hold=hold, ref=ref, active=check_inputs(model, c, hold, ref))
    return _shared[key]


def ee_name(model):
    return "EE_1" if model == "jaco2_dual_torque" else "EE"


def frames(model):
    """(a world-fixed frame with a pose of its own, the EE frame with a non-zero point)."""
    w = product_lib.JacoFrame()
    w.body = -1
    w.pos[:] = [0.25, -0.5, 0.75]
    w.mat[:] = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    w.point[:] = [0.1, 0.2, 0.3]
    ee = ib.table_of(model).jaco_frame(ee_name(model), point=np.array([0.01, -0.02, 0.03]))
    assert any(abs(x) > 0 for x in ee.pos)
    return w, ee


# ---- the cases.  Each returns what it measured; the caller prints it and holds it to its bound.
def case_oracle(run, model, long=False):
    """Case 1: every knot's qpos and qvel against the fp64 oracle.  Returns (qpos measure, qvel measure, the call's result)."""
    g = shared(model, long)
    r = run(model, g["c"], g["q"], g["v"], want=("qpos", "qvel", "status"), hold=g["hold"])
    assert (r["status"] == 0).all(), r["status"]
    return verr(r["qpos"], g["ref"]["qpos"]), verr(r["qvel"], g["ref"]["qvel"]), r


def case_frames(run, query, model=MODEL):
    """Case 3: xpos / xmat rows against the query at the returned qpos rows, a world-fixed frame and the EE frame.  query(model, qpos
    [N, nq], qvel [N, nv], frame) -> (xpos [N, 3], xmat [N, 9]).  Returns (xpos measure, xmat measure) over both frames."""
    g = shared(model)
    ex = em = 0.0
    for f in frames(model):
        r = run(model, g["c"], g["q"], g["v"], frame=f, hold=g["hold"])
        n, T = r["qpos"].shape[:2]
        xp, xm = query(model, r["qpos"].reshape(n * T, -1), r["qvel"].reshape(n * T, -1), f)
        ex, em = max(ex, verr(r["xpos"].reshape(n * T, 3), xp)), max(em, verr(r["xmat"].reshape(n * T, 9), xm))
        if f.body < 0:   # a world-fixed frame is the frame record itself, bit for bit
            assert (bits(r["xpos"]) == bits(np.array(f.pos[:], np.float32))).all() and (bits(r["xmat"]) == bits(np.array(f.mat[:], np.float32))).all()
    return ex, em


def same(a, b, keys=None):
    for k in (keys or a):
        assert a[k].shape == b[k].shape and (bits(a[k]) == bits(b[k])).all(), k


def case_self_consistency(run, model=MODEL):
    """Case 4: hold = 3 against hold = 1 with every ctrl row repeated; final_only; each output alone; two identical calls; the fan-out
    through state_index against replicated states; the handle's state against get_state()'s tensors handed in.  All bit for bit."""
    g = shared(model)
    q, v, c, hold = g["q"], g["v"], g["c"], g["hold"]
    ee = frames(model)[1]
    full = run(model, c, q, v, frame=ee, hold=hold)
    assert not (bits(full["qpos"]) == bits(np.float32(SENTINEL))).all(1).any() and (full["status"] == 0).all()
    same(full, run(model, c, q, v, frame=ee, hold=hold))
    fine = run(model, np.repeat(c, hold, axis=1), q, v, frame=ee, hold=1)
    same(full, {k: (x if k == "status" else x[:, hold - 1::hold]) for k, x in fine.items()})
    last = run(model, c, q, v, frame=ee, hold=hold, final_only=1)
    same(last, {k: (x if k == "status" else x[:, -1:]) for k, x in full.items()})
    for k in OUTS[:4]:
        alone = run(model, c, q, v, frame=ee if k in ("xpos", "xmat") else None, want=(k,), hold=hold)
        assert set(alone) == {k}
        same(alone, full, (k,))
    m = 5
    idx = np.arange(3 * m) % m
    c3 = np.concatenate([c[:m], c[m:2 * m], c[2 * m:3 * m]])
    same(run(model, c3, q[:m], v[:m], state_index=idx, frame=ee, hold=hold), run(model, c3, q[idx], v[idx], frame=ee, hold=hold))
    same(run(model, c, None, None, frame=ee, hold=hold, handle=(q, v)), full)


BAD_STATES, BAD_PLANS = 7, 4   # the states and the plans the bad-index case's entries point into


def bad_index(call, outs, plans):
    """The bad-index case of the four entries: index entries -1 and one past the end among valid ones have JACO_ROLLOUT_BAD_INDEX in
    their status words and their rows of every output in `outs` untouched; every other rollout is bitwise what it is without the bad
    entries.  call(keep, **indices) -> the tier's result on BAD_STATES states (and, with `plans`, BAD_PLANS plans) with those index
    arrays -- state_index, with `plans` also plan_index --, `keep`: the rollouts of the full call it makes (rows of a per-rollout input)."""
    m, P = BAD_STATES, BAD_PLANS
    sidx = np.array([0, 3, -1, 6, m, 2, 2, 5, 1, 4], np.int32)
    pidx = np.array([0, 1, 2, P, 3, -1, 2, 0, 3, 1], np.int32)
    if plans:
        index, bad = dict(plan_index=pidx, state_index=sidx), (sidx < 0) | (sidx >= m) | (pidx < 0) | (pidx >= P)
        assert bad.sum() == 4
    else:   # (jaco_rollout: one sequence per rollout, nine of them)
        sidx = sidx[:-1]
        index, bad = dict(state_index=sidx), (sidx < 0) | (sidx >= m)
    r = call(np.arange(len(sidx)), **index)
    ok = call(np.flatnonzero(~bad), **{k: x[~bad] for k, x in index.items()})
    assert (r["status"][bad] == BAD_INDEX).all() and (r["status"][~bad] == 0).all()
    for key in outs:
        if key != "status":
            assert (bits(r[key][bad]) == bits(np.float32(SENTINEL))).all(), key
            assert (bits(r[key][~bad]) == bits(ok[key])).all(), key


def case_bad_index(run, model=MODEL):
    """Case 5: state_index entries -1 and nstates among valid ones: JACO_ROLLOUT_BAD_INDEX in their status words, their rows untouched,
    every other rollout bitwise what it is without the bad entries."""
    g = shared(model)
    m, ee = BAD_STATES, frames(model)[1]
    bad_index(lambda keep, **index: run(model, g["c"][keep], g["q"][:m], g["v"][:m], frame=ee, hold=g["hold"], **index), OUTS, plans=False)


# ---- the refusals: one argument set per JACO_EINVAL case of include/jaco_env.h, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"   # 11 fused bodies
REFUSAL_N, REFUSAL_ENVS = 4, 5
REFUSALS = {
    "null_options": "the options are required",
    "nknots_0": "nknots 0 x hold 1: both must be at least 1 and their product at most 16384",
    "hold_0": "nknots 2 x hold 0: both must be at least 1 and their product at most 16384",
    "too_long": "nknots 2 x hold 8193: both must be at least 1 and their product at most 16384",
    "final_only_2": "final_only must be 0 or 1",
    "n_negative": "n -1 is negative",
    "null_ctrl": "the ctrl sequences are required",
    "null_out": "the output record is required",
    "status_only": "at least one of the outputs qpos, qvel, xpos and xmat is required",
    "pose_without_frame": "xpos and xmat need a frame",
    "body_low": "frame body -2 outside [-1, 11)",
    "body_high": "frame body 11 outside [-1, 11)",
    "qpos0_alone": "qpos0 and qvel0 are given together or not at all",
    "qvel0_alone": "qpos0 and qvel0 are given together or not at all",
    "nstates_not_num_envs": "nstates 4 with the handle's state of 5 envs",
    "nstates_0": "nstates 0 with a state override",
    "n_beyond_nstates": "n 4 rollouts from 3 states without a state index",
}


def refusal_args(case):
    """Keyword arguments of one refused call of `rollout` / the GPU tier's twin on REFUSAL_MODEL: REFUSAL_N sequences of 2 knots."""
    g = shared(REFUSAL_MODEL)
    n = REFUSAL_N
    k = dict(ctrl=g["c"][:n, :2], qpos0=g["q"][:n], qvel0=g["v"][:n], want=("qpos", "status"))

    def body(b):
        f = product_lib.JacoFrame()
        f.body = b
        return f
    k.update({"null_options": dict(no_opt=True), "nknots_0": dict(nknots=0), "hold_0": dict(hold=0), "too_long": dict(hold=8193),
              "final_only_2": dict(final_only=2), "n_negative": dict(n=-1), "null_ctrl": dict(no_ctrl=True), "null_out": dict(no_out=True),
              "status_only": dict(want=("status",)), "pose_without_frame": dict(want=("qpos", "xpos")), "body_low": dict(frame=body(-2)),
              "body_high": dict(frame=body(11)), "qpos0_alone": dict(qvel0=None, nstates=n), "qvel0_alone": dict(qpos0=None, nstates=n),
              "nstates_not_num_envs": dict(qpos0=None, qvel0=None, nstates=n, handle=(g["q"][:REFUSAL_ENVS], g["v"][:REFUSAL_ENVS])),
              "nstates_0": dict(nstates=0, state_index=np.zeros(n, np.int32)), "n_beyond_nstates": dict(qpos0=g["q"][:3], qvel0=g["v"][:3])}[case])
    return k


# ---- case 8: robot_config.rollout.  make_sim(model, qpos, qvel) -> a BatchedMujoco (GPU tier) or emu_sim.EmuSim.
CONFIG_K, CONFIG_T = 3, 2


def case_config(make_sim, model):
    """BatchedMujocoConfig.rollout with K = 3 sequences per env, hold 1: the documented shapes; q / dq the documented columns of the
    sim-tier result, bit for bit; without K the K axis squeezed; the first knot's dq against dq + h forward_dynamics(ctrl_0,
    implicit_damping=True) on the envs the oracle reports without limit rows in the first substep.  Returns that vector measure."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    g = shared(model)
    n = len(g["q"])
    sim = make_sim(model, g["q"], g["v"])
    cfg = BatchedMujocoConfig(sim, ee=ee_name(model))
    c = np.stack([g["c"][:, :CONFIG_T], g["c"][:, 2:2 + CONFIG_T], g["c"][:, 4:4 + CONFIG_T]], 1)   # [n, K, T, nu]
    ctrl = torch.as_tensor(c, device=sim.device)
    r = cfg.rollout(ctrl)
    nJ = len(cfg.arm)
    assert r["q"].shape == (n, CONFIG_K, CONFIG_T, nJ) and r["dq"].shape == (n, CONFIG_K, CONFIG_T, nJ) and r["status"].shape == (n, CONFIG_K)
    assert r["ee_pos"].shape == (n, CONFIG_K, CONFIG_T, 3) and r["ee_mat"].shape == (n, CONFIG_K, CONFIG_T, 9)
    raw = sim.rollout(ctrl.reshape(n * CONFIG_K, CONFIG_T, -1), state_index=np.repeat(np.arange(n), CONFIG_K), frame=ib.table_of(model).jaco_frame(ee_name(model)))
    N = lambda t: t.cpu().numpy()
    assert (bits(N(r["q"]).reshape(n * CONFIG_K, CONFIG_T, nJ)) == bits(N(raw["qpos"])[..., list(cfg.arm_qadr)])).all()
    assert (bits(N(r["dq"]).reshape(n * CONFIG_K, CONFIG_T, nJ)) == bits(N(raw["qvel"])[..., list(cfg.arm)])).all()
    assert (bits(N(r["ee_pos"]).reshape(-1, 3)) == bits(N(raw["xpos"]).reshape(-1, 3))).all() and (N(r["status"]) == 0).all()
    one = cfg.rollout(ctrl[:, 1], final_only=True)
    assert one["q"].shape == (n, 1, nJ) and one["ee_mat"].shape == (n, 1, 9) and one["status"].shape == (n,)
    assert (bits(N(one["q"])) == bits(N(r["q"])[:, 1, -1:])).all()
    ok = g["ref"]["nefc"][:, 0] == 0
    assert ok.sum() >= 3
    h, worst = fb.tables(model)["h"], 0.0
    for k in range(CONFIG_K):
        a = N(cfg.forward_dynamics(ctrl[:, k, 0].contiguous(), implicit_damping=True)).astype(np.float64)
        pred = g["v"][:, list(cfg.arm)].astype(np.float64) + h * a
        worst = max(worst, verr(N(r["dq"])[:, k, 0][ok], pred[ok]))
    return worst
