"""ctypes binding of tests/emu/libjaco_emu*.so -- TEST INFRASTRUCTURE ONLY.

Runs the *unmodified* HIP kernel source (mujoco_jaco_amd/csrc/physics_kernel.h) compiled for the host
against a lockstep 64-lane wavefront emulator, so kernel logic can be checked against the oracle
without a GPU.  Not a product path: the product library refuses to run without a HIP device.
One library per layout / build option holds every entry: ctrl-level steps (with the contact record),
env-level calls, the ten query-style entries that read the model (tests/query_binding.py, ik_binding.py, osc_binding.py,
osc_task_binding.py, joint_binding.py, fd_binding.py, rollout_binding.py, rollout_fb_binding.py, rollout_cost_binding.py,
rollout_osc_binding.py; emu_sim.py puts them under BatchedMujoco's own public methods as one stand-in sim), and one set of option
switches.  lib() is the only
place that builds and loads such a library and declares the argument types of its emu_* entries.  The switches are process-wide
state of a library that every entry shares: whoever flips one puts it back (try / finally), so that no test depends on what ran
before it.
A refused call raises ValueError with the text the library would leave in jaco_last_error.
"""
import ctypes
import sys
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
EMU_DIR = os.path.join(ROOT, "tests", "emu")
ASSETS = os.path.join(ROOT, "mujoco_jaco_amd", "assets")
_libs = {}
# launch modes of emu_env_call, read from the kernel's own enum (physics_kernel.h JacoMode) so that the two cannot drift apart
with open(os.path.join(ROOT, "mujoco_jaco_amd", "csrc", "physics_kernel.h")) as _f:
    _MODES = {k: int(v) for k, v in re.findall(r"(JM_\w+) = (\d+)", re.search(r"enum JacoMode \{([^}]*)\}", _f.read()).group(1))}
JM_STEP, JM_FORWARD, JM_HOLD, JM_TERMINAL, JM_PREREACH = (_MODES[k] for k in ("JM_STEP", "JM_FORWARD", "JM_HOLD", "JM_TERMINAL", "JM_PREREACH"))


def lib(layout=""):
    """layout "": the default build (11 bodies / 21 dofs in blocks 9 + 6 + 6); "_d12": the build for jaco2_torque.xml (12 hinge dofs, one tree);
    "_d30": the build for jaco2_dual_torque.xml (two arms + two objects, 30 dofs; ctrl level); "_wrench" / "_nolook" / "_mprpairs": A/B builds of the default layout
    (body-space constraint rows; the Newton solver without its look-ahead stop; MPR two pairs per wave)."""
    if layout not in _libs:
        name = "libjaco_emu%s.so" % layout
        subprocess.check_call(["make", "-s", "-C", EMU_DIR, name])
        L = ctypes.CDLL(os.path.join(EMU_DIR, name))
        fp, ip, up = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.emu_physics_step.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, up, ip,
                                       ctypes.c_void_p, ip, ctypes.c_int, fp, ctypes.c_int, ip]
        L.emu_env_call.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong,
                                   fp, fp, fp, fp, up, ip, fp, fp, fp, fp, fp, fp, ctypes.POINTER(ctypes.c_ubyte), fp, ip]
        L.emu_query.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, fp, fp, ctypes.c_void_p, ctypes.c_int, fp, fp, fp, fp, fp]
        L.emu_marker_rest.argtypes = [ctypes.c_char_p, ctypes.c_long, fp]
        L.emu_ik.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, fp, fp, fp, fp, fp, ip]
        L.emu_osc.argtypes = [ctypes.c_char_p, ctypes.c_long, ci, vp, ci, vp, fp, fp, fp, fp, fp, fp, ip]
        L.emu_osc_task.argtypes = [ctypes.c_char_p, ctypes.c_long, ci, vp, ci, vp, vp, fp, fp, fp, fp, fp, fp, fp, ip]
        L.emu_joint.argtypes = [ctypes.c_char_p, ctypes.c_long, ci, vp, fp, fp, fp, fp, fp, fp, fp]
        L.emu_fd.argtypes = [ctypes.c_char_p, ctypes.c_long, ci, vp, fp, fp, fp, vp]
        L.emu_rollout.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp]
        L.emu_rollout_fb.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp]
        L.emu_rollout_cost.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp]
        L.emu_rollout_osc.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp]
        L.emu_step_lo.argtypes = [ctypes.c_char_p, ctypes.c_long, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.emu_last_error.restype = ctypes.c_char_p
        L.emu_qpos0.argtypes = [ctypes.c_char_p, ctypes.c_long, fp]
        L.emu_set_auto_reset.argtypes = [ctypes.c_int]
        L.emu_reset_env.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, fp, fp, fp, fp, fp]
        L.emu_set_init_buffer.argtypes = [fp, ctypes.c_int, ctypes.c_int]
        for switch in ("obs_mode", "hints", "sep_cache", "mpr_pairs", "pair_list", "handdown", "mpr_output", "tier_return"):
            getattr(L, "emu_set_" + switch).argtypes = [ctypes.c_int]
        L.emu_get_counter.argtypes = [ctypes.c_int, ctypes.c_int]; L.emu_get_counter.restype = ctypes.c_long
        L.emu_last_terminal.argtypes = []; L.emu_last_terminal.restype = fp
        L.emu_task_nact.argtypes = [ctypes.c_int]
        _libs[layout] = L
    return _libs[layout]


def check(L, rc, entry):
    """A refused call (argument check or model loader) raises ValueError with the driver's message."""
    if rc != 0:
        raise ValueError("%s returned %d: %s" % (entry, rc, L.emu_last_error().decode()))


class EmuEnv:
    """Batched env state (fp32, [nenv][n]) stepped by the emulated kernel."""

    def __init__(self, model="jaco2_curtain_torque", nenv=1, layout=None):
        self.blob = open(os.path.join(ASSETS, model + ".jacomdl"), "rb").read()
        from mujoco_jaco_amd.modelc import blob as blobmod
        M = blobmod.loads(self.blob)
        from mujoco_jaco_amd import _lib as product_lib
        self.L = lib(layout if layout is not None else product_lib.variant_for(self.blob))   # (the same layout choice as the product's loader)
        self.M = M
        self.nq, self.nv, self.nu, self.ns = int(M["nq"][0]), int(M["nv"][0]), int(M["nu"][0]), int(M["nsensor"][0])
        self.nenv = nenv
        self.qpos = np.tile(M["qpos0"].astype(np.float32), (nenv, 1))
        self.qvel = np.zeros((nenv, self.nv), np.float32)
        self.qacc_ws = np.zeros((nenv, self.nv), np.float32)
        self.sensordata = np.zeros((nenv, self.ns), np.float32)
        self.flags = np.zeros(nenv, np.uint32)
        self.stats = np.zeros((nenv, 4), np.int32)
        self.dbg = np.zeros(self.L.emu_dbg_size(), np.float32)

    def step(self, ctrl, nsub=1, disable_contact=False, dbg_env=-1):
        self._physics_step(ctrl, nsub, disable_contact, None, None, 0, dbg_env)

    def step_rec(self, ctrl, nsub=1, cap=16, disable_contact=False, guard=0):
        """One ctrl-level step with the record on (cap > 0) or off (cap = 0): (rec [nenv][cap][24] words, ncon [nenv]).  `guard` extra
        records after the buffer's end are passed in NaN-filled and returned as self.guard (a write past the capacity would show there)."""
        assert self.L.emu_contact_words() == 24
        buf = np.full(self.nenv * max(cap, 1) + guard, np.nan, np.float32).repeat(24).reshape(-1, 24)   # (NaN: a slot the kernel did not write stands out)
        rec = buf[:self.nenv * max(cap, 1)].reshape(self.nenv, max(cap, 1), 24)
        ncon = np.full(self.nenv, -7, np.int32)
        self._physics_step(ctrl, nsub, disable_contact, buf if cap > 0 else None, ncon if cap > 0 else None, cap, -1)
        self.guard = buf[self.nenv * max(cap, 1):]
        return (rec, ncon) if cap > 0 else (None, None)

    def _physics_step(self, ctrl, nsub, disable_contact, rec, ncon, cap, dbg_env):
        ctrl = np.ascontiguousarray(np.broadcast_to(np.asarray(ctrl, np.float32), (self.nenv, self.nu)))
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        hv = ctypes.c_int(0)
        rc = self.L.emu_physics_step(self.blob, len(self.blob), self.nenv, nsub, int(disable_contact), fp(self.qpos), fp(self.qvel),
                                     fp(self.qacc_ws), fp(ctrl), fp(self.sensordata),
                                     self.flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                     self.stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                     ctypes.c_void_p(rec.ctypes.data) if rec is not None else None,
                                     ncon.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if ncon is not None else None, cap,
                                     fp(self.dbg) if dbg_env >= 0 else None, dbg_env, ctypes.byref(hv))
        check(self.L, rc, "emu_physics_step")
        self.heavy_envs = hv.value


class EmuJacoEnv(EmuEnv):
    """Env-level calls (jaco_step / jaco_forward semantics) on the emulated kernels."""

    def __init__(self, model="jaco2_curtain_torque", nenv=1, task_id=0, frame_skip=50, seed=0):
        super().__init__(model, nenv)
        self.task_id, self.frame_skip, self.seed = task_id, frame_skip, seed
        self.nact = self.L.emu_task_nact(task_id)   # (the library's own rule: env_arrays.h jaco_task_nact)
        self.task = np.zeros((nenv, self.L.emu_task_floats()), np.float32)
        self.cache = np.zeros((nenv, self.L.emu_cache_floats()), np.float32)
        self.obs = np.zeros((nenv, 26), np.float32)
        self.reward = np.zeros(nenv, np.float32)
        self.done = np.zeros(nenv, np.uint8)
        self.task[:, 0] = 0.6; self.task[:, 16] = 0.6
        rest = np.zeros(24, np.float32)
        assert self.L.emu_marker_rest(self.blob, len(self.blob), rest.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
        self.marker = np.tile(rest, (nenv, 1))   # ["hand", "subgoal_reach"] x (position, rotation): parked at the XML pose

    def _call(self, mode, action=None, noise=None):
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a is not None else None
        hv = ctypes.c_int(0)
        self.L.emu_set_obs_mode(int(getattr(self, "obs_mode", 0)))
        try:
            rc = self.L.emu_env_call(self.blob, len(self.blob), self.nenv, mode, self.frame_skip, self.task_id, self.nact, self.seed,
                                     fp(self.qpos), fp(self.qvel), fp(self.qacc_ws), fp(self.sensordata),
                                     self.flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), self.stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                     fp(self.task), fp(self.cache), fp(action), fp(noise), fp(self.obs), fp(self.reward),
                                     self.done.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), fp(self.marker), ctypes.byref(hv))
        finally:
            self.L.emu_set_obs_mode(0)   # (the library's switch, not this env's: the next caller finds the default)
        assert rc == 0
        self.heavy_envs = hv.value

    def placing_hold(self, nsub=150):
        """JM_HOLD: the held part of the placing reset (jaco_reset runs it between the reset kernel and jaco_forward)."""
        fs, self.frame_skip = self.frame_skip, nsub
        try:
            self._call(JM_HOLD, None, None)
        finally:
            self.frame_skip = fs

    def grasping_prereach(self, cap=4000, noise=None):
        """JM_PREREACH: the pre-reach loops of the grasping reset (jaco_reset runs them after the draws); returns the observation row."""
        fs, self.frame_skip = self.frame_skip, cap
        try:
            self._call(JM_PREREACH, None, None if noise is None else np.ascontiguousarray(noise, np.float32))
        finally:
            self.frame_skip = fs
        return self.obs.copy()

    def set_auto_reset(self, on):
        """option "auto_reset": a finished env is reset (draws + sim.forward() + first observation) by the wave that finished it."""
        self.L.emu_set_auto_reset(int(on))

    def set_init_buffer(self, rows):
        """kwarg init_buffer (jaco_set_init_buffer of the library): recorded rows every reset draws its reaching goal from; None = sampled goals."""
        if rows is None:
            self.L.emu_set_init_buffer(None, 0, 0)
            return
        r = np.ascontiguousarray(rows, np.float32)
        self.L.emu_set_init_buffer(r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r.shape[0], r.shape[1])

    def reset_env(self, env, noise=None):
        """jaco_reset(mask = {env}): the reset kernel's work for one env, then the forward pass + observation (JM_FORWARD; here for all envs,
        which is harmless for the others: a forward pass does not change state)."""
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        check(self.L, self.L.emu_reset_env(self.blob, len(self.blob), self.task_id, self.seed, env, fp(self.qpos), fp(self.qvel), fp(self.qacc_ws),
                                           fp(self.task), fp(self.marker)), "emu_reset_env")

    def forward(self, noise=None):
        self._call(JM_FORWARD, None, None if noise is None else np.ascontiguousarray(noise, np.float32))
        return self.obs.copy()

    def env_step(self, action, noise=None):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action, np.float32), (self.nenv, self.nact)))
        self._call(JM_STEP, a, None if noise is None else np.ascontiguousarray(noise, np.float32))
        return self.obs.copy(), self.reward.copy(), self.done.copy()
