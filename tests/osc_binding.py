"""The operational-space controller kernel (mujoco_jaco_amd/csrc/osc.h) under the wavefront emulator (emu_osc of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 reference (oracle/glue.py osc_generate on the fp64 oracle's J, M[active, active], qfrc_bias[active], point and
quaternion), the input sets of the tests (seeds, targets, near-singular configurations) and the closed loops.  emu_sim.EmuSim runs
BatchedMujoco.osc on the emulated call (CPU tests of robot_config.BatchedOSC).
"""
import ctypes
import os
import sys

import numpy as np

import emu_binding
import ik_binding as ib
import query_binding as qb
from emu_binding import ROOT
from mujoco_jaco_amd import _lib as product_lib

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import glue  # noqa: E402

DEFAULTS = dict(product_lib.JacoOscOptions.DEFAULTS)


_info = {}


def _model_info(model):
    """(blob bytes, library layout, nu) of a model, read once."""
    if model not in _info:
        from mujoco_jaco_amd.modelc import blob as blobmod
        blob = qb.blob_of(model)
        _info[model] = (blob, product_lib.variant_for(blob), int(blobmod.loads(blob)["nu"][0]))
    return _info[model]


def osc(model, frames, qpos, qvel, target_pos, target_quat, ctrl_in=None, status=True, alias=False, defaults=False, no_out=False, **options):
    """Emulated jaco_osc: {"ctrl" [B, nu], "status" [B, nf]} for a list of _lib.JacoFrame (None: a NULL table), fp32 states qpos [B, nq] /
    qvel [B, nv], targets [B, nf, 3] / [B, nf, 4] (None: NULL), ctrl_in [B, nu] (None: NULL).  alias=True: ctrl_out is the ctrl_in
    buffer.  defaults=True hands a NULL options pointer, no_out=True a NULL ctrl_out.  Raises ValueError with the library's message when
    the call is refused."""
    blob, layout, nu = _model_info(model)
    L = emu_binding.lib(layout)
    qpos, qvel = np.ascontiguousarray(qpos, np.float32), np.ascontiguousarray(qvel, np.float32)
    B, nf = qpos.shape[0], 0 if frames is None else len(frames)
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    tp = None if target_pos is None else np.ascontiguousarray(target_pos, np.float32).reshape(B, -1)
    tq = None if target_quat is None else np.ascontiguousarray(target_quat, np.float32).reshape(B, -1)
    cin = None if ctrl_in is None else np.array(ctrl_in, np.float32).reshape(B, nu)   # (a copy: alias=True overwrites it)
    out = cin if alias else np.full((B, nu), np.nan, np.float32)
    st = np.full((B, max(nf, 1)), -7, np.int32) if status else None
    opt = product_lib.JacoOscOptions(**options)
    arr = None if frames is None else (product_lib.JacoFrame * max(nf, 1))(*frames)
    rc = L.emu_osc(blob, len(blob), B, None if arr is None else ctypes.cast(arr, ctypes.c_void_p), nf if frames is not None else 1,
                   None if defaults else ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), fp(qpos), fp(qvel), fp(tp), fp(tq), fp(cin),
                   None if no_out else fp(out), None if st is None else st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    emu_binding.check(L, rc, "emu_osc")
    return {"ctrl": out, "status": st}


# ---- the fp64 reference: glue.osc_generate on the oracle's quantities
def active_dofs(model, name, dof_mask=0):
    """Dof addresses of the hinge joints on the chain of body `name`, narrowed by dof_mask: the controller's active set, in dof order."""
    _, dadr = ib.table_of(model).chain(name)
    return [d for d in sorted(dadr) if not dof_mask or (dof_mask >> d) & 1]


def motor_of(model):
    """{dof: index of its motor actuator} of the model (FrameTable.motor_of_dof)."""
    return ib.table_of(model).motor_of_dof()


def reference(model, names, qpos, qvel, target6, dof_mask=0, kp=50.0, ko=180.0, kv=20.0, vmax_xyz=0.4, vmax_abg=1.0472):
    """fp64: (u [B, nf, 6] (the first n entries: the active dofs in dof order, the rest 0), |det(J M^-1 J^T)| [B, nf], active dof lists)
    of glue.osc_generate at the fp32 states, targets target6 [B, nf, 6] = position + 'rxyz' Euler angles.  The oracle's quantities as
    query_binding.oracle_answers takes them: mj_jacBodyCom, qM, qfrc_bias, body pose.  n < 6: M padded with identity, J with zero
    columns."""
    from oracle_binding import Oracle
    o = Oracle(model)
    tab = ib.table_of(model)
    B, nf = qpos.shape[0], len(names)
    target6 = np.asarray(target6, np.float64).reshape(B, nf, 6)
    acts = [active_dofs(model, n, dof_mask) for n in names]
    U, D = np.zeros((B, nf, 6)), np.zeros((B, nf))
    for e in range(B):
        o.set("qpos", qpos[e].astype(np.float64)); o.set("qvel", qvel[e].astype(np.float64))
        o.forward()
        xp, xq, xm = o.get("xpos").reshape(-1, 3), o.get("xquat").reshape(-1, 4), o.get("xmat").reshape(-1, 3, 3)
        qM, bias, dq = o.get("qM").reshape(o.nv, o.nv), o.get("qfrc_bias"), o.get("qvel")
        for f, name in enumerate(names):
            b, a = tab.body_id(name), acts[f]
            n = len(a)
            jp, jr = o.jac_body_com(b)
            J, M, bi, v = np.zeros((6, 6)), np.eye(6), np.zeros(6), np.zeros(6)
            J[:3, :n], J[3:, :n] = jp[:, a], jr[:, a]
            M[:n, :n] = qM[np.ix_(a, a)]
            bi[:n], v[:n] = bias[a], dq[a]
            D[e, f] = abs(np.linalg.det(J @ np.linalg.inv(M) @ J.T))
            u = glue.osc_generate(v, target6[e, f], J, M, bi, xp[b] + xm[b] @ tab.com(name), xq[b], kp, ko, kv, (vmax_xyz, vmax_abg))
            U[e, f, :n] = u[:n]
    return U, D, acts


def kernel_targets(target6):
    """What the kernel is handed for targets [..., 6] (position + Euler): fp32 positions and glue.quat_from_euler quaternions rounded to fp32."""
    t = np.asarray(target6, np.float64)
    flat = t.reshape(-1, 6)
    quat = np.array([glue.quat_from_euler(*r[3:]) for r in flat]).reshape(*t.shape[:-1], 4)
    return t[..., :3].astype(np.float32), quat.astype(np.float32)


def error(u, u_ref):
    """The measure of the tests: max over the active dofs of |u - u_ref| / (1 + |u_ref|), per env."""
    u, u_ref = np.asarray(u, np.float64), np.asarray(u_ref, np.float64)
    return (np.abs(u - u_ref) / (1.0 + np.abs(u_ref))).max(axis=-1)


# ---- inputs
def states(model, B, seed=3, vseed=5):
    """fp32 (qpos, qvel): the picking reset states of the workload (ik_binding.picking_seeds) with qvel uniform in +-0.5."""
    q = ib.picking_seeds(model, B, seed=seed)
    nv = int(ib.load_model(model)["nv"][0])
    v = np.random.default_rng(vseed).uniform(-0.5, 0.5, (B, nv)).astype(np.float32)
    return q, v


def targets6(model, name, qpos, s=0.3, seed=11):
    """[B, 6] reachable targets as position + 'rxyz' Euler angles: ik_binding.targets (the body's COM as the point, so that the point is
    mj_jacBodyCom's) with the quaternion turned into Euler angles; fp32-representable positions."""
    tab = ib.table_of(model)
    P, Qt, _ = ib.targets(model, name, tab.com(name), qpos, s, seed=seed)
    E = np.array([glue.euler_from_quat(q) for q in Qt.astype(np.float64)])
    return np.concatenate([P.astype(np.float64), E], 1)


def singular_states(model="jaco2_curtain_torque", name="EE", want=8, seed=3, limit=2.5e-4):
    """`want` fp32 states with fp64 |det(J M^-1 J^T)| < limit: the elbow (dof 2) of the picking seeds scanned towards the straight arm
    (q2 near pi; a coarse grid over [2.6, 3.4], then a fine one around its minimum); seeds whose minimum stays above the limit are left
    out.  Generated, not stored."""
    q, v = states(model, 4 * want, seed=seed)
    out = []
    t6 = np.zeros((1, 1, 6))

    def det_at(e, a):
        qe = q[e:e + 1].copy()
        qe[0, 2] = np.float32(a)
        return reference(model, [name], qe, v[e:e + 1], t6)[1][0, 0]

    for e in range(q.shape[0]):
        grid = np.linspace(2.6, 3.4, 41)
        a0 = grid[np.argmin([det_at(e, a) for a in grid])]
        grid = np.linspace(a0 - 0.02, a0 + 0.02, 41)
        d = [det_at(e, a) for a in grid]
        if min(d) < limit:
            q[e, 2] = np.float32(grid[np.argmin(d)])
            out.append(e)
        if len(out) == want:
            break
    assert len(out) >= want, "the elbow scan found only %d near-singular configurations" % len(out)
    return q[out], v[out]


# ---- the refusals: one argument set per JACO_EINVAL case of include/jaco_env.h, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"
REFUSAL_CASES = ("nframes0", "nframes3", "body_low", "body_high", "empty", "seven", "overlap", "no_motor", "gain", "null_pos", "null_quat", "null_out")


def refusal_args(case, B=2):
    """(frames, target_pos [B, nf, 3] or None, target_quat [B, nf, 4] or None, no_out, options) of one refused call on REFUSAL_MODEL."""
    tab = ib.table_of(REFUSAL_MODEL)
    ee = tab.jaco_frame("EE")
    frames, opts, no_out = [ee], {}, False
    if case == "nframes0":
        frames = []
    elif case == "nframes3":
        frames = [ee, ee, ee]
    elif case in ("body_low", "body_high"):
        ee.body = -1 if case == "body_low" else 11
    elif case == "empty":
        frames = [tab.jaco_frame("object_body")]
    elif case == "seven":
        frames = [tab.jaco_frame("thumb_proximal")]
    elif case == "overlap":
        frames = [ee, tab.jaco_frame("link3")]
    elif case == "no_motor":
        frames, opts = [tab.jaco_frame("thumb_proximal")], dict(dof_mask=0b1000000)
    elif case == "gain":
        opts = dict(kv=0.0)
    nf = max(len(frames), 1)
    tp = None if case == "null_pos" else np.zeros((B, nf, 3), np.float32)
    tq = None if case == "null_quat" else np.tile(np.float32([1, 0, 0, 0]), (B, nf, 1))
    return frames, tp, tq, case == "null_out", opts


# ---- closed loop: 200 x { osc -> send_forces(nsub = 1) } on the arm-only model
LOOP_MODEL, LOOP_B, LOOP_STEPS = "jaco2_reaching_torque", 8, 200


def offset_targets(model, name, qpos, dist, ang, seed):
    """[B, 6] targets (position + 'rxyz' Euler angles): the fp64 pose of body `name` at qpos moved by a drawn offset of length
    dist = (lo, hi) m and turned about a drawn axis by ang = (lo, hi) rad; fp32-representable positions."""
    from mujoco_jaco_amd.modelc import rot
    tab = ib.table_of(model)
    P, R = ib.oracle_pose(model, name, tab.com(name), qpos)
    B = len(P)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(B, 3))
    d *= (rng.uniform(dist[0], dist[1], B) / np.linalg.norm(d, axis=1))[:, None]
    T = np.zeros((B, 6))
    for e in range(B):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        a = rng.uniform(ang[0], ang[1])
        dq = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * ax])
        T[e, :3] = (P[e] + d[e]).astype(np.float32)
        T[e, 3:] = glue.euler_from_quat(rot.mat_to_quat(rot.quat_to_mat(dq) @ R[e]))
    return T


def loop_inputs():
    """(q0 [8, 9] fp32, target6 [8, 6]): start poses qpos0 +- 0.5 rad (query_binding.hold_states) and targets 5-10 cm / 0.1-0.3 rad
    from the start pose of the EE."""
    q0 = qb.hold_states(LOOP_B, seed=21)
    return q0, offset_targets(LOOP_MODEL, "EE", q0, (0.05, 0.10), (0.1, 0.3), seed=22)


def pose_error(model, name, qpos, target6):
    """(|p - p*| [B], rotation angle between R and R* [B]) of the fp64 oracle's EE pose at qpos against the targets."""
    tab = ib.table_of(model)
    P, R = ib.oracle_pose(model, name, tab.com(name), qpos)
    ep = np.linalg.norm(P - target6[:, :3], axis=1)
    er = np.zeros(len(ep))
    for e in range(len(ep)):
        Rt = glue.quat_to_mat(glue.quat_from_euler(*target6[e, 3:]))
        er[e] = np.linalg.norm(ib.rotvec(Rt @ R[e].T))
    return ep, er


def closed_loop_oracle(q0, target6, steps=LOOP_STEPS):
    """fp64: the oracle stepped one substep per control tick with glue.osc_generate on fresh quantities (contacts off); final qpos [B, 9]."""
    from oracle_binding import Oracle
    o = Oracle(LOOP_MODEL)
    o.option("disable_contact", 1)
    tab = ib.table_of(LOOP_MODEL)
    b, a, com = tab.body_id("EE"), active_dofs(LOOP_MODEL, "EE"), tab.com("EE")
    mot = motor_of(LOOP_MODEL)
    out = np.zeros((q0.shape[0], o.nq))
    for e in range(q0.shape[0]):
        o.set("qpos", q0[e].astype(np.float64)); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv))
        hold = q0[e].astype(np.float64)
        for _ in range(steps):
            o.forward()
            xp, xq, xm = o.get("xpos").reshape(-1, 3), o.get("xquat").reshape(-1, 4), o.get("xmat").reshape(-1, 3, 3)
            jp, jr = o.jac_body_com(b)
            qM = o.get("qM").reshape(o.nv, o.nv)
            u = glue.osc_generate(o.get("qvel")[a], target6[e], np.vstack([jp[:, a], jr[:, a]]), qM[np.ix_(a, a)], o.get("qfrc_bias")[a],
                                  xp[b] + xm[b] @ com, xq[b])
            c = loop_ctrl_row(hold[None])[0].astype(np.float64)
            for k, d in enumerate(a):
                c[mot[d]] = u[k]
            o.step(c)
        out[e] = o.get("qpos")
    return out


def loop_ctrl_row(q0):
    """ctrl_in rows of the loop: arm motors 0, finger position servos commanded to their start angles."""
    c = np.zeros((q0.shape[0], 9), np.float32)
    c[:, 6:9] = q0[:, 6:9]
    return c


def closed_loop_emu(q0, target6, steps=LOOP_STEPS):
    """... on the emulated OSC and step kernels: final qpos [B, 9] (fp32)."""
    from emu_binding import EmuEnv
    e = EmuEnv(LOOP_MODEL, q0.shape[0])
    e.qpos[:] = q0
    fr = [ib.table_of(LOOP_MODEL).jaco_frame("EE")]
    tp, tq = kernel_targets(target6)
    cin = loop_ctrl_row(q0)
    for _ in range(steps):
        c = osc(LOOP_MODEL, fr, e.qpos, e.qvel, tp, tq, cin)["ctrl"]
        e.step(c, nsub=1, disable_contact=True)
    return e.qpos.copy()
