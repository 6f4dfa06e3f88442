"""The robot-configuration query kernel (mujoco_jaco_amd/csrc/query.h) under the wavefront emulator (emu_query of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also the fp64 oracle's answers to the same questions.  emu_sim.EmuSim runs BatchedMujoco.query on the emulated call (CPU tests of
robot_config.BatchedMujocoConfig).
"""
import ctypes
import os

import numpy as np

import emu_binding
from emu_binding import ASSETS

OUTS = ("xpos", "xmat", "jac", "qM", "qfrc_bias")


def blob_of(model):
    return open(os.path.join(ASSETS, model + ".jacomdl"), "rb").read()


def query(model, qpos, qvel, frames, want=OUTS):
    """Emulated jaco_query: {output: array} at the fp32 states qpos [B, nq] / qvel [B, nv] for a list of _lib.JacoFrame.  Raises ValueError
    with the library's message when the call is refused."""
    from mujoco_jaco_amd import _lib as product_lib
    blob = blob_of(model)
    L = emu_binding.lib(product_lib.variant_for(blob))
    qpos = np.ascontiguousarray(qpos, np.float32)
    qvel = np.ascontiguousarray(qvel, np.float32)
    B, nv, nf = qpos.shape[0], qvel.shape[1], len(frames)
    shapes = {"xpos": (B, nf, 3), "xmat": (B, nf, 9), "jac": (B, nf, 6, nv), "qM": (B, nv, nv), "qfrc_bias": (B, nv)}
    res = {k: np.full(shapes[k], np.nan, np.float32) for k in want}
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    arr = (product_lib.JacoFrame * max(nf, 1))(*frames)
    rc = L.emu_query(blob, len(blob), B, fp(qpos), fp(qvel), ctypes.cast(arr, ctypes.c_void_p), nf,
                     *[fp(res[k]) if k in res else None for k in OUTS])
    emu_binding.check(L, rc, "emu_query")
    return res


def oracle_answers(model, qpos, qvel, bodies):
    """fp64 oracle (sim.forward()) at the same states: xpos / xmat / mj_jacBodyCom of the MJCF bodies, qM, qfrc_bias."""
    from oracle_binding import Oracle
    o = Oracle(model)
    B = qpos.shape[0]
    nb = len(bodies)
    r = {"xpos": np.zeros((B, nb, 3)), "xmat": np.zeros((B, nb, 9)), "jac": np.zeros((B, nb, 6, o.nv)), "qM": np.zeros((B, o.nv, o.nv)),
         "qfrc_bias": np.zeros((B, o.nv))}
    for e in range(B):
        o.set("qpos", qpos[e].astype(np.float64)); o.set("qvel", qvel[e].astype(np.float64))
        o.forward()
        xp, xm = o.get("xpos").reshape(-1, 3), o.get("xmat").reshape(-1, 9)
        for i, b in enumerate(bodies):
            r["xpos"][e, i], r["xmat"][e, i] = xp[b], xm[b]
            jp, jr = o.jac_body_com(b)
            r["jac"][e, i, :3], r["jac"][e, i, 3:] = jp, jr
        r["qM"][e] = o.get("qM").reshape(o.nv, o.nv)
        r["qfrc_bias"][e] = o.get("qfrc_bias")
    return r


def random_states(M, B, seed, qvel_scale=1.0):
    """fp32 states around qpos0: hinge angles +-1 rad, free bodies moved by up to 5 cm with a random orientation, random velocities."""
    rng = np.random.default_rng(seed)
    nq, nv = int(M["nq"][0]), int(M["nv"][0])
    q = np.tile(M["qpos0"], (B, 1))
    for j in range(int(M["njnt"][0])):
        a = int(M["jnt_qposadr"][j])
        if M["jnt_type"][j] == 3:
            q[:, a] += rng.uniform(-1, 1, B)
        else:
            q[:, a:a + 3] += rng.uniform(-0.05, 0.05, (B, 3))
            u = rng.normal(size=(B, 4))
            q[:, a + 3:a + 7] = u / np.linalg.norm(u, axis=1, keepdims=True)
    v = rng.normal(size=(B, nv)) * qvel_scale
    return q.astype(np.float32), v.astype(np.float32)


# ---- closed loop through the query surface: ctrl[arm] = -g + PD (gravity compensation), fingers held by their position servos
KP, KD = 50.0, 5.0


def hold_ctrl(q, dq, bias, qt, gc=True, xp=np):
    """ctrl [B, 9] of the reaching model: arm torque qfrc_bias (= -g) + PD towards qt, finger servos commanded to their start angles."""
    u = KP * (qt[:, :6] - q[:, :6]) - KD * dq[:, :6]
    if gc:
        u = u + bias[:, :6]
    return xp.concatenate([u, qt[:, 6:9]], 1) if xp is np else xp.cat([u, qt[:, 6:9]], 1)


def hold_states(B, seed):
    """Start states of the reaching model: arm angles qpos0 +- 0.5 rad, fingers at qpos0, at rest; fp32."""
    from mujoco_jaco_amd.modelc import blob
    M = blob.load(os.path.join(ASSETS, "jaco2_reaching_torque.jacomdl"))
    q = np.tile(M["qpos0"], (B, 1))
    q[:, :6] += np.random.default_rng(seed).uniform(-0.5, 0.5, (B, 6))
    return q.astype(np.float32)


def closed_loop_oracle(q0, nsub, gc=True):
    """The same loop in fp64 on the oracle (contacts off, as in the GPU / emulator runs): final qpos [B, 9]."""
    from oracle_binding import Oracle
    o = Oracle("jaco2_reaching_torque")
    o.option("disable_contact", 1)
    out = np.zeros((q0.shape[0], 9))
    for e in range(q0.shape[0]):
        qt = q0[e:e + 1].astype(np.float64)
        o.set("qpos", qt[0]); o.set("qvel", np.zeros(9)); o.set("qacc_warmstart", np.zeros(9))
        for _ in range(nsub):
            o.forward()
            q, dq, bias = o.get("qpos")[None], o.get("qvel")[None], o.get("qfrc_bias")[None]
            o.step(hold_ctrl(q, dq, bias, qt, gc)[0])
        out[e] = o.get("qpos")
    return out


def closed_loop_emu(q0, nsub, gc=True):
    """... on the emulated step and query kernels: final qpos [B, 9] (fp32)."""
    from emu_binding import EmuEnv
    e = EmuEnv("jaco2_reaching_torque", q0.shape[0])
    e.qpos[:] = q0
    qt = q0.astype(np.float32)
    for _ in range(nsub):
        bias = query("jaco2_reaching_torque", e.qpos, e.qvel, [], want=("qfrc_bias",))["qfrc_bias"]
        e.step(hold_ctrl(e.qpos, e.qvel, bias, qt, gc).astype(np.float32), nsub=1, disable_contact=True)
    return e.qpos.copy()
