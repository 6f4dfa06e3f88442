"""GPU tier: the library's refusals are the emulator driver's, word for word -- both call the same host halves (jaco_query_resolve,
jaco_contact_record_check, jaco_ik_resolve).  No physics kernel is launched: bad arguments through the C ABI, jaco_last_error against the
driver's text for the same argument, and a valid jaco_query on the same handle after each refusal.
jaco_ik with max_iters = 0 is inside the documented range [0, JACO_IK_MAX_ITERS] (include/jaco_env.h): neither side refuses it, and the
test holds the two to that same answer (no iteration taken); the IK refusal compared word for word is max_iters = 257."""
import ctypes

import numpy as np
import pytest
import torch

import ik_binding as ikb
import query_binding as qb
from emu_binding import EmuEnv
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco

pytestmark = pytest.mark.gpu
MODEL = "jaco2_curtain_torque"


def _emu_message(call):
    with pytest.raises(ValueError) as ei:
        call()
    return str(ei.value).split(": ", 1)[1]   # "emu_<entry> returned -1: <message>"


def test_refusal_messages_equal_the_emulators():
    B = 4
    sim = BatchedMujoco(B, robot_file=MODEL)
    L, h, T = sim.L, sim.h, sim.frames
    q, v, _ = [t.cpu().numpy() for t in sim.get_state()]
    ee = T.jaco_frame("EE")
    bad = _lib.JacoFrame()
    bad.body = 11   # 11 fused bodies: 0 .. 10
    frames = lambda fs: ctypes.cast((_lib.JacoFrame * len(fs))(*fs), ctypes.c_void_p)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    xpos = torch.empty(B, 1, 3, device=sim.device)
    out = _lib.JacoQueryOut(vp(xpos), None, None, None, None)
    rec = torch.zeros(B * 4 * _lib.CONTACT_WORDS + 4, device=sim.device)
    ncon = torch.zeros(B, dtype=torch.int32, device=sim.device)
    assert rec.data_ptr() % 16 == 0
    tp, qout = torch.zeros(B, 3, device=sim.device), torch.empty(B, sim.nq, device=sim.device)
    status = torch.full((B, 2), -7, dtype=torch.int32, device=sim.device)
    ik = lambda n: L.jaco_ik(h, ctypes.cast(ctypes.pointer(ee), ctypes.c_void_p), ctypes.cast(ctypes.pointer(_lib.JacoIkOptions(max_iters=n)), ctypes.c_void_p),
                             None, vp(tp), None, vp(qout), None, vp(status), None)
    emu_ik = lambda n: ikb.ik(MODEL, ee, q, np.zeros((B, 3), np.float32), max_iters=n)
    e = EmuEnv(MODEL, B)
    emu_rec, emu_n = np.zeros(B * 4 * 24 + 4, np.float32), np.zeros(B, np.int32)
    emu_rec = emu_rec[(-emu_rec.ctypes.data % 16) // 4:][:B * 4 * 24 + 1]
    step = lambda r, cap: e._physics_step(np.zeros(e.nu, np.float32), 1, False, r, emu_n, cap, -1)
    cases = [
        (lambda: L.jaco_query(h, frames([ee] * 17), 17, None, None, None, None), lambda: qb.query(MODEL, q, v, [ee] * 17)),
        (lambda: L.jaco_query(h, frames([ee, bad]), 2, None, None, None, None), lambda: qb.query(MODEL, q, v, [ee, bad])),
        (lambda: L.jaco_set_contact_record(h, vp(rec), vp(ncon), 0), lambda: step(emu_rec[:-1], 0)),
        (lambda: L.jaco_set_contact_record(h, ctypes.c_void_p(rec.data_ptr() + 4), vp(ncon), 4), lambda: step(emu_rec[1:], 4)),
        (lambda: ik(257), lambda: emu_ik(257)),
    ]
    for refused, emulated in cases:
        assert refused() == -1   # JACO_EINVAL
        message = L.jaco_last_error(h).decode()
        print(message)
        assert message == _emu_message(emulated)
        xpos.fill_(float("nan"))
        assert L.jaco_query(h, frames([ee]), 1, None, None, ctypes.cast(ctypes.pointer(out), ctypes.c_void_p), None) == 0
        assert torch.isfinite(xpos).all()
    # max_iters = 0: valid on both sides, the pose is evaluated and no step taken
    assert ik(0) == 0
    assert (status.cpu().numpy() == 0).all() and (emu_ik(0)["iters"] == 0).all()
    sim.close()
