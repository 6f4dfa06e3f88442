"""The inverse-kinematics kernel (mujoco_jaco_amd/csrc/ik.h) under the wavefront emulator (emu_ik of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 numpy restatement of the algorithm on modelc.kin.fk / jac_point, the fp64 oracle's forward kinematics as the judge of a
returned configuration and the target sets of the tests.  emu_sim.EmuSim runs BatchedMujoco.ik on the emulated call (CPU tests of
robot_config.BatchedMujocoConfig.ik).
"""
import ctypes
import os

import numpy as np

import emu_binding
import query_binding as qb
from emu_binding import ASSETS
from mujoco_jaco_amd import _lib as product_lib
from mujoco_jaco_amd.modelc import blob as blobmod
from mujoco_jaco_amd.modelc import kin, rot

DEFAULTS = dict(product_lib.JacoIkOptions.DEFAULTS)


def load_model(model):
    return blobmod.load(os.path.join(ASSETS, model + ".jacomdl"))


def table_of(model):
    from mujoco_jaco_amd.robot_config import FrameTable
    return FrameTable.for_model(model)


def ik(model, frame, qpos, target_pos, target_quat=None, resid=True, status=True, defaults=False, **options):
    """Emulated jaco_ik: {"qpos", "resid" [B, 2], "iters", "converged"} for one _lib.JacoFrame (None: a NULL frame), fp32 seed rows qpos
    [B, nq], targets [B, 3] / [B, 4] (None: NULL).  defaults=True hands a NULL options pointer.  Raises ValueError with the library's
    message when the call is refused."""
    blob = qb.blob_of(model)
    L = emu_binding.lib(product_lib.variant_for(blob))
    qpos = np.ascontiguousarray(qpos, np.float32)
    B = qpos.shape[0]
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    tp = None if target_pos is None else np.ascontiguousarray(target_pos, np.float32).reshape(B, 3)
    tq = None if target_quat is None else np.ascontiguousarray(target_quat, np.float32).reshape(B, 4)
    out = np.full(qpos.shape, np.nan, np.float32)
    res = np.full((B, 2), np.nan, np.float32) if resid else None
    st = np.full((B, 2), -7, np.int32) if status else None
    opt = product_lib.JacoIkOptions(**options)
    rc = L.emu_ik(blob, len(blob), B, ctypes.cast(ctypes.pointer(frame), ctypes.c_void_p) if frame is not None else None,
                  None if defaults else ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), fp(qpos), fp(tp), fp(tq), fp(out), fp(res),
                  None if st is None else st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    emu_binding.check(L, rc, "emu_ik")
    r = {"qpos": out}
    if res is not None:
        r["resid"] = res
    if st is not None:
        r["iters"], r["converged"] = st[:, 0].copy(), st[:, 1].copy()
    return r


# ---- the algorithm in fp64 numpy (include/jaco_env.h, "inverse kinematics"), on the model compiler's own kinematics
def rotvec(E):
    """Rotation vector of a rotation matrix: axis * sin from the antisymmetric part, cos from the trace, angle by atan2."""
    a = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    cs, sn = 0.5 * (np.trace(E) - 1.0), np.linalg.norm(a)
    ang = np.arctan2(sn, cs)
    if sn < 1e-15:
        return np.array([ang, 0.0, 0.0]) if cs < 0 else a
    return a * (ang / sn)


def pose_fp64(M, body, point, q):
    """(p, R, fk tuple) of the point `point` (body frame) of MJCF body `body` at qpos q, by modelc.kin.fk."""
    f = kin.fk(M, q)
    R = rot.quat_to_mat(f[1][body])
    return f[0][body] + R @ point, R, f


def ik_fp64(M, table, name, point, qpos, target_pos, target_quat=None, tol_pos=1e-5, tol_rot=1e-4, damping=0.02, max_step=0.3, max_iters=60,
            dof_mask=0):
    """The restatement, env by env: (qpos [B, nq], iters [B], converged [B], resid [B, 2])."""
    body = table.body_id(name)
    qadr, dadr = table.chain(name)
    act = [(a, d) for a, d in zip(qadr, dadr) if not dof_mask or (dof_mask >> d) & 1]
    jq = {int(M["jnt_qposadr"][j]): j for j in range(int(M["njnt"][0]))}
    lim = M["jnt_range"].reshape(-1, 2)
    point = np.asarray(point, np.float64)
    Q = np.array(qpos, np.float64)
    B = Q.shape[0]
    iters, conv, resid = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 2))
    for e in range(B):
        q = Q[e]
        Rt = None if target_quat is None else rot.quat_to_mat(rot.quat_normalize(np.asarray(target_quat[e], np.float64)))
        k = 0
        while True:
            p, R, f = pose_fp64(M, body, point, q)
            ep = np.asarray(target_pos[e], np.float64) - p
            er = np.zeros(3) if Rt is None else rotvec(Rt @ R.T)
            resid[e] = np.linalg.norm(ep), np.linalg.norm(er)
            if resid[e, 0] < tol_pos and (Rt is None or resid[e, 1] < tol_rot):
                conv[e] = 1
                break
            if k == max_iters:
                break
            jp, jr = kin.jac_point(M, *f, body, p)
            cols = [d for _, d in act]
            J = np.vstack([jp[:, cols], jr[:, cols] if Rt is not None else np.zeros((3, len(cols)))])
            dq = J.T @ np.linalg.solve(J @ J.T + damping ** 2 * np.eye(6), np.concatenate([ep, er]))
            mx = np.abs(dq).max()
            if mx > max_step:
                dq *= max_step / mx
            for (a, _), s in zip(act, dq):
                q[a] += s
                if M["jnt_limited"][jq[a]]:
                    q[a] = min(max(q[a], lim[jq[a], 0]), lim[jq[a], 1])
            k += 1
        iters[e] = k
    return Q, iters, conv, resid


# ---- the judge: the fp64 oracle's forward kinematics at a returned configuration
def oracle_pose(model, name, point, qpos):
    """(p [B, 3], R [B, 3, 3]) of the point on MJCF body `name` by Oracle.forward (xpos / xmat) at fp32 rows qpos."""
    from oracle_binding import Oracle
    o = Oracle(model)
    b = table_of(model).body_id(name)
    qpos = np.asarray(qpos, np.float64)
    P, R = np.zeros((qpos.shape[0], 3)), np.zeros((qpos.shape[0], 3, 3))
    for e in range(qpos.shape[0]):
        o.set("qpos", qpos[e]); o.set("qvel", np.zeros(o.nv))
        o.forward()
        R[e] = o.get("xmat").reshape(-1, 3, 3)[b]
        P[e] = o.get("xpos").reshape(-1, 3)[b] + R[e] @ np.asarray(point, np.float64)
    return P, R


def oracle_errors(model, name, point, qpos, target_pos, target_quat=None):
    """(|e_p| [B], |e_r| [B]) of the configurations qpos against the targets, judged by the oracle's FK."""
    P, R = oracle_pose(model, name, point, qpos)
    ep = np.linalg.norm(np.asarray(target_pos, np.float64) - P, axis=1)
    er = np.zeros(len(ep))
    if target_quat is not None:
        for e in range(len(ep)):
            er[e] = np.linalg.norm(rotvec(rot.quat_to_mat(rot.quat_normalize(np.asarray(target_quat[e], np.float64))) @ R[e].T))
    return ep, er


# ---- seeds and targets
def picking_seeds(model, B, seed=3):
    """fp32 seed rows: the picking reset states of the workload (both arms on the two-arm model)."""
    from mujoco_jaco_amd import workload
    M = load_model(model)
    if int(M["nq"][0]) >= 32:
        return workload.reset_states_dual(M["qpos0"], B, seed=seed).astype(np.float32)
    return workload.reset_states(M["qpos0"], B, seed=seed, f32_draws=True).astype(np.float32)


def targets(model, name, point, seeds, s, seed=11, clamp=True):
    """Reachable targets: the fp64 FK (point position [B, 3], body quaternion [B, 4], fp32-rounded) of the seed with the chain's arm
    angles moved by uniform +-s and clamped to their ranges (clamp=False: left where they fall); also the configurations themselves."""
    M, table = load_model(model), table_of(model)
    body = table.body_id(name)
    qadr, _ = table.chain(name)
    jq = {int(M["jnt_qposadr"][j]): j for j in range(int(M["njnt"][0]))}
    lim = M["jnt_range"].reshape(-1, 2)
    rng = np.random.default_rng(seed)
    G = np.array(seeds, np.float64)
    G[:, qadr] += rng.uniform(-s, s, (G.shape[0], len(qadr)))
    for a in qadr:
        if clamp and M["jnt_limited"][jq[a]]:
            G[:, a] = np.clip(G[:, a], lim[jq[a], 0], lim[jq[a], 1])
    P, Qt = np.zeros((G.shape[0], 3)), np.zeros((G.shape[0], 4))
    for e in range(G.shape[0]):
        p, R, f = pose_fp64(M, body, np.asarray(point, np.float64), G[e])
        P[e], Qt[e] = p, f[1][body]
    return P.astype(np.float32), Qt.astype(np.float32), G
