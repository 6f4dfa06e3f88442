"""The task-axis / null-space controller kernel (mujoco_jaco_amd/csrc/osc_task.h, jaco_osc_task) under the wavefront emulator
(emu_osc_task of tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 restatement of abr_control's OSC.generate() with ctrlr_dof and null_controllers = [Damping, RestingConfig] on true
k x k matrices (generate / reference: the oracle's J, qM, qfrc_bias, point and quaternion, taken as osc_binding.reference takes them),
the inputs of the tests, the refusal cases and the closed loops.  emu_sim.EmuSim runs BatchedMujoco.osc on the emulated call.
"""
import ctypes

import numpy as np

import emu_binding
import ik_binding as ib
import osc_binding as ob
from mujoco_jaco_amd import _lib as product_lib
from osc_binding import glue

POS, ROT, ALL = 0b000111, 0b111000, 0b111111
NULL = dict(null_kv=10.0, rest_kp=20.0, rest_kv=5.0)   # the gains of the null-space cases


def task_record(nf, axes=None, null_kv=0.0, rest_kp=0.0, rest_kv=0.0, rest_mask=0):
    """_lib.JacoOscTask from the keywords of BatchedMujoco.osc."""
    return product_lib.JacoOscTask(axes=product_lib.osc_axes(axes, nf), null_kv=null_kv, rest_kp=rest_kp, rest_kv=rest_kv, rest_mask=rest_mask)


def osc_task(model, frames, qpos, qvel, target_pos, target_quat, ctrl_in=None, rest_qpos=None, no_task=False, raw_axes=None, **kw):
    """Emulated jaco_osc_task: {"ctrl" [B, nu], "status" [B, nf]}; arguments as osc_binding.osc, plus rest_qpos [B, nq] (None: NULL), the
    task keywords (axes, null_kv, rest_kp, rest_kv, rest_mask; raw_axes: the axes words as they are) and the options (the remaining
    keywords).  no_task=True hands a NULL task record.  Raises ValueError with the library's message when the call is refused."""
    blob, layout, nu = ob._model_info(model)
    L = emu_binding.lib(layout)
    qpos, qvel = np.ascontiguousarray(qpos, np.float32), np.ascontiguousarray(qvel, np.float32)
    B, nf = qpos.shape[0], len(frames)
    tk = {k: kw.pop(k) for k in ("axes", "null_kv", "rest_kp", "rest_kv", "rest_mask") if k in kw}
    task = task_record(nf, **tk)
    if raw_axes is not None:
        task.axes[:] = raw_axes
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    tp = None if target_pos is None else np.ascontiguousarray(target_pos, np.float32).reshape(B, -1)
    tq = None if target_quat is None else np.ascontiguousarray(target_quat, np.float32).reshape(B, -1)
    rest = None if rest_qpos is None else np.ascontiguousarray(rest_qpos, np.float32).reshape(B, qpos.shape[1])
    cin = None if ctrl_in is None else np.array(ctrl_in, np.float32).reshape(B, nu)
    out = np.full((B, nu), np.nan, np.float32)
    st = np.full((B, max(nf, 1)), -7, np.int32)
    opt = product_lib.JacoOscOptions(**kw)
    arr = (product_lib.JacoFrame * max(nf, 1))(*frames)
    rc = L.emu_osc_task(blob, len(blob), B, ctypes.cast(arr, ctypes.c_void_p), nf, ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p),
                        None if no_task else ctypes.cast(ctypes.pointer(task), ctypes.c_void_p), fp(qpos), fp(qvel), fp(tp), fp(tq), fp(rest),
                        fp(cin), fp(out), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    emu_binding.check(L, rc, "emu_osc_task")
    return {"ctrl": out, "status": st}


# ---- the fp64 restatement
def rows_of(axes):
    return [r for r in range(6) if ((axes or ALL) >> r) & 1]


def generate(J, M, bias, dq, q, pos, quat, target6, axes=0, null_kv=0.0, rest=None, held=None, rest_kp=0.0, rest_kv=0.0,
             kp=50.0, ko=180.0, kv=20.0, vmax_xyz=0.4, vmax_abg=1.0472):
    """abr_control's OSC.generate with ctrlr_dof and null_controllers = [Damping(null_kv), RestingConfig(rest, rest_kp, rest_kv)] in
    fp64: J 6 x n, M n x n, bias / dq / q n-vectors (the active dofs), pos / quat the controlled point and orientation, target6 =
    position + 'rxyz' Euler angles, rest an n-vector of rest angles (None: no resting term) held where `held` (n booleans; None: all)
    is set.  Returns (u [n], |det(Js M^-1 Js^T)| of the k x k matrix, pseudo-inverse branch taken, Js)."""
    rows = rows_of(axes)
    n, k = len(dq), len(rows)
    Js = J[rows]
    Minv = np.linalg.inv(M)
    X = Js @ Minv @ Js.T
    det = abs(np.linalg.det(X))
    sing = not (n >= k and det >= 1e-3)
    if not sing:
        Mx = np.linalg.inv(X)
    else:
        u_, s_, vh = np.linalg.svd(X)
        Mx = vh.T @ np.diag([0.0 if x < 0.005 else 1.0 / x for x in s_]) @ u_.T
    u_task = np.zeros(6)
    u_task[:3] = np.asarray(pos) - target6[:3]
    qd = glue.quat_from_euler(*target6[3:6]); qd = qd / np.linalg.norm(qd)
    qc = np.array([quat[0], -quat[1], -quat[2], -quat[3]], np.float64)
    w = qd[0] * qc[0] - qd[1:] @ qc[1:]
    u_task[3:] = -(qd[0] * qc[1:] + qc[0] * qd[1:] + np.cross(qd[1:], qc[1:])) * np.sign(w)
    sat_xyz, sat_abg = vmax_xyz / kp * kv, vmax_abg / ko * kv
    nx, na = np.linalg.norm(u_task[:3]), np.linalg.norm(u_task[3:])
    u_task[:3] *= kp * (sat_xyz / nx if nx > sat_xyz else 1.0)      # velocity limiting on the full halves and the gains ...
    u_task[3:] *= ko * (sat_abg / na if na > sat_abg else 1.0)
    u = -kv * (M @ dq) - Js.T @ (Mx @ u_task[rows]) + bias          # ... and only then u_task[ctrlr_dof]
    u_null = np.zeros(n)
    if null_kv:
        u_null += -null_kv * (M @ dq)
    if rest is not None:
        h = np.ones(n, bool) if held is None else np.asarray(held, bool)
        e = np.where(h, np.mod(rest - q + np.pi, 2 * np.pi) - np.pi, 0.0)
        u_null += M @ (rest_kp * e - rest_kv * np.where(h, dq, 0.0))
    Jbar = Minv @ Js.T @ Mx
    u += (np.eye(n) - Js.T @ Jbar.T) @ u_null
    return u, det, sing, Js


def reference(model, names, qpos, qvel, target6, axes=0, null_kv=0.0, rest_qpos=None, rest_kp=0.0, rest_kv=0.0, rest_mask=0, dof_mask=0, **gains):
    """fp64 at the fp32 states: {"u" [B, nf, 6] (the first n entries: the active dofs in dof order), "det" [B, nf], "sing" [B, nf],
    "acts" (active dof lists), "Js" / "M" (per env and frame: the k x n and n x n matrices)}.  axes: one mask, or one per name."""
    from oracle_binding import Oracle
    o = Oracle(model)
    tab = ib.table_of(model)
    B, nf = qpos.shape[0], len(names)
    target6 = np.asarray(target6, np.float64).reshape(B, nf, 6)
    axes = [axes] * nf if isinstance(axes, int) else list(axes)
    acts = [ob.active_dofs(model, n, dof_mask) for n in names]
    qadr_of = dof_qadr(model)
    out = dict(u=np.zeros((B, nf, 6)), det=np.zeros((B, nf)), sing=np.zeros((B, nf), bool), acts=acts, Js=[], M=[])
    for e in range(B):
        o.set("qpos", qpos[e].astype(np.float64)); o.set("qvel", qvel[e].astype(np.float64))
        o.forward()
        xp, xq, xm = o.get("xpos").reshape(-1, 3), o.get("xquat").reshape(-1, 4), o.get("xmat").reshape(-1, 3, 3)
        qM, bias, dq = o.get("qM").reshape(o.nv, o.nv), o.get("qfrc_bias"), o.get("qvel")
        Js_e, M_e = [], []
        for f, name in enumerate(names):
            b, a = tab.body_id(name), acts[f]
            qa = [qadr_of[d] for d in a]
            jp, jr = o.jac_body_com(b)
            J, M = np.vstack([jp[:, a], jr[:, a]]), qM[np.ix_(a, a)]
            rest = None if rest_qpos is None else np.asarray(rest_qpos[e], np.float64)[qa]
            held = [not rest_mask or bool((rest_mask >> d) & 1) for d in a]
            if rest is not None:
                rest = np.where(held, rest, 0.0)   # (entries that are not held are not read: they may hold anything)
            u, det, sing, Js = generate(J, M, bias[a], dq[a], qpos[e].astype(np.float64)[qa], xp[b] + xm[b] @ tab.com(name), xq[b], target6[e, f],
                                        axes[f], null_kv, rest, held, rest_kp, rest_kv, **gains)
            out["u"][e, f, :len(a)], out["det"][e, f], out["sing"][e, f] = u, det, sing
            Js_e.append(Js); M_e.append(M)
        out["Js"].append(Js_e); out["M"].append(M_e)
    return out


def dof_qadr(model):
    """{hinge dof: its qpos address}."""
    M = ib.load_model(model)
    return {int(d): int(q) for q, d in zip(M["jnt_qposadr"], M["jnt_dofadr"])}


# ---- inputs
def rest_rows(model, name, qpos, seed=17, mask=0):
    """[B, nq] fp32 rest rows: q + U(-1, 1) + 2 pi m, m in {-1, 0, 1} drawn per entry, at the qpos addresses of the chain's dofs (those of
    `mask` when it is non-zero); NaN everywhere else -- those words must not be read."""
    rng = np.random.default_rng(seed)
    qa = dof_qadr(model)
    rest = np.full(qpos.shape, np.nan, np.float32)
    for d in ob.active_dofs(model, name):
        draw = qpos[:, qa[d]].astype(np.float64) + rng.uniform(-1, 1, len(qpos)) + 2 * np.pi * rng.integers(-1, 2, len(qpos))
        if not mask or (mask >> d) & 1:
            rest[:, qa[d]] = draw
    return rest


# ---- the refusals jaco_osc_task adds to jaco_osc's: one argument set each, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"
REFUSALS = {
    "axes_high": "frame 0: axes 64 has bits above bit 5",
    "null_kv_negative": "null_kv, rest_kp and rest_kv must be finite and not negative",
    "rest_kp_nan": "null_kv, rest_kp and rest_kv must be finite and not negative",
    "rest_kv_inf": "null_kv, rest_kp and rest_kv must be finite and not negative",
    "rest_mask_empty": "frame 0: rest_mask leaves none of its active dofs",
    "null_quat": "frame 0: a rotational axis is selected and the target quaternions are missing",
}


def refusal_args(case, B=2):
    """(target_quat [B, 1, 4] or None, rest_qpos [B, nq] or None, task keywords) of one refused call on REFUSAL_MODEL, frame EE."""
    tq = np.tile(np.float32([1, 0, 0, 0]), (B, 1, 1))
    rest, task = None, {}
    if case == "axes_high":
        task = dict(raw_axes=(64, 0))
    elif case == "null_kv_negative":
        task = dict(null_kv=-1.0)
    elif case == "rest_kp_nan":
        task = dict(rest_kp=float("nan"))
    elif case == "rest_kv_inf":
        task = dict(rest_kv=float("inf"))
    elif case == "rest_mask_empty":
        rest, task = np.zeros((B, int(ib.load_model(REFUSAL_MODEL)["nq"][0])), np.float32), dict(rest_mask=0b111000000)
    elif case == "null_quat":
        tq, task = None, dict(axes=0b001111)
    return tq, rest, task


# ---- closed loop: 200 x { osc -> send_forces(nsub = 1) } on the arm-only model, position-only with both null-space terms
LOOP_REST_OFFSET = np.array([0, 0, 0, 0.4, -0.4, 0.4])


def loop_rest(q0):
    """[B, 9] fp32 rest rows of the loop: the start angles of the arm moved by LOOP_REST_OFFSET."""
    rest = q0.copy()
    rest[:, :6] += LOOP_REST_OFFSET.astype(np.float32)
    return rest


def closed_loop_oracle(q0, target6, rest, steps=ob.LOOP_STEPS):
    """fp64: the oracle stepped one substep per control tick with generate() on fresh quantities (contacts off); final qpos [B, 9]."""
    from oracle_binding import Oracle
    o = Oracle(ob.LOOP_MODEL)
    o.option("disable_contact", 1)
    tab = ib.table_of(ob.LOOP_MODEL)
    b, a, com = tab.body_id("EE"), ob.active_dofs(ob.LOOP_MODEL, "EE"), tab.com("EE")
    qa = [dof_qadr(ob.LOOP_MODEL)[d] for d in a]
    mot = ob.motor_of(ob.LOOP_MODEL)
    out = np.zeros((q0.shape[0], o.nq))
    for e in range(q0.shape[0]):
        o.set("qpos", q0[e].astype(np.float64)); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv))
        c0 = ob.loop_ctrl_row(q0[e:e + 1])[0].astype(np.float64)
        for _ in range(steps):
            o.forward()
            xp, xq, xm = o.get("xpos").reshape(-1, 3), o.get("xquat").reshape(-1, 4), o.get("xmat").reshape(-1, 3, 3)
            jp, jr = o.jac_body_com(b)
            qM = o.get("qM").reshape(o.nv, o.nv)
            u = generate(np.vstack([jp[:, a], jr[:, a]]), qM[np.ix_(a, a)], o.get("qfrc_bias")[a], o.get("qvel")[a], o.get("qpos")[qa],
                         xp[b] + xm[b] @ com, xq[b], target6[e], POS, NULL["null_kv"], rest[e].astype(np.float64)[qa], None, NULL["rest_kp"], NULL["rest_kv"])[0]
            c = c0.copy()
            for k, d in enumerate(a):
                c[mot[d]] = u[k]
            o.step(c)
        out[e] = o.get("qpos")
    return out


def closed_loop_emu(q0, target6, rest, steps=ob.LOOP_STEPS):
    """... on the emulated controller and step kernels: final qpos [B, 9] (fp32)."""
    from emu_binding import EmuEnv
    e = EmuEnv(ob.LOOP_MODEL, q0.shape[0])
    e.qpos[:] = q0
    fr = [ib.table_of(ob.LOOP_MODEL).jaco_frame("EE")]
    tp = ob.kernel_targets(target6)[0]
    cin = ob.loop_ctrl_row(q0)
    for _ in range(steps):
        c = osc_task(ob.LOOP_MODEL, fr, e.qpos, e.qvel, tp, None, cin, rest, axes=POS, **NULL)["ctrl"]
        e.step(c, nsub=1, disable_contact=True)
    return e.qpos.copy()
