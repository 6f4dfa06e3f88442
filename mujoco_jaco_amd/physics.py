"""Ctrl-level batched physics: the `Mujoco` sim-interface tier of the reference, batched.

Mirrors /root/reference/env_script/mujoco.py (send_forces :258-278, get_feedback :349-359, get/set state :213-246,
get_xyz / get_orientation :148-210, get_obj_vel :212-215) for `num_envs` environments resident on one MI355X.
PyTorch is used only to own device buffers and streams; every computation is in libjaco_env.so.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .robot_config import ContactNames, FrameTable


class JacoError(RuntimeError):
    pass


def _rows(t, dev, n, rows=-1):
    """t as a contiguous fp32 [rows, n] tensor on dev (rows -1: as many as it holds), or None."""
    return None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(rows, n).contiguous()


def _ptr(t):
    """A tensor's device pointer, or None."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ref(rec):
    """The address of a ctypes record (or of an array of them), as the C ABI's untyped pointer."""
    return ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p)


def _plan_record(plan, alpha, plan_index):
    """The JacoRolloutPlan of jaco_rollout_fb and jaco_rollout_cost from their launch methods' arguments."""
    return _lib.JacoRolloutPlan(_ptr(plan["ctrl"]), _ptr(plan.get("kff")), _ptr(plan.get("gain")), _ptr(plan.get("xref")), _ptr(alpha), _ptr(plan_index),
                                int(plan["ctrl"].shape[0]))


class Contacts:
    """One contact record (BatchedMujoco.contacts): the fields of include/jaco_env.h JacoContact as [B, K, ...] device tensors."""

    def __init__(self, rec, ncon, gmap):
        B, K, _ = rec.shape
        f = rec[..., :_lib.CONTACT_FLOATS]
        i = rec.view(torch.int32)[..., _lib.CONTACT_FLOATS:]
        self.ncon = ncon.clone()
        self.valid = torch.arange(K, device=rec.device)[None, :] < self.ncon[:, None]
        v = self.valid
        z = lambda t: torch.where(v.reshape(B, K, *([1] * (t.dim() - 2))), t, torch.zeros((), dtype=t.dtype, device=t.device))
        self.dist = z(f[..., 0])
        self.pos = z(f[..., 1:4])
        self.frame = z(f[..., 4:13]).reshape(B, K, 3, 3)
        self.force = z(f[..., 13:19])
        ids = i.long()
        geom = gmap[ids[..., 0:2].clamp(0, gmap.numel() - 1)]
        neg = torch.full((), -1, dtype=torch.int64, device=rec.device)
        self.geom = torch.where(v[..., None], geom, neg)
        self.body = torch.where(v[..., None], ids[..., 2:4], neg)
        self.dim = torch.where(v, i[..., 4], torch.zeros((), dtype=torch.int32, device=rec.device))

    def world_force(self):
        """[B, K, 3] contact force in world coordinates: the force geom 1's body exerts on geom 2's body (MuJoCo's sign: J = frame (J2 - J1))."""
        return (self.frame[..., :3, :] * self.force[..., :3, None]).sum(-2)

    def net_force(self, body_a, body_b):
        """[B, 3] world-frame force that MJCF body id body_a exerts on body_b, summed over the recorded contacts between them."""
        fw = self.world_force()
        ab = (self.body[..., 0] == body_a) & (self.body[..., 1] == body_b)
        ba = (self.body[..., 0] == body_b) & (self.body[..., 1] == body_a)
        sgn = ab.to(fw.dtype) - ba.to(fw.dtype)
        return (fw * sgn[..., None]).sum(1)


def _closed_loop_args(sim, what, ctrl, qpos, qvel, gain, x_ref, dofs, feedforward, alpha, plan_index, state_index, noise=None, targets=None):
    """The arguments BatchedMujoco.rollout_feedback, rollout_cost and rollout_osc share (a function of the module, so that a stand-in sim
    which borrows the methods needs nothing but the launch methods), checked and made contiguous device tensors: {"plan": {"ctrl", "kff",
    "gain", "xref", "target_pos", "target_quat"}, "alpha", "plan_index", "state_index", "qpos", "qvel", "nstates", "n", "T", "dofs",
    "noise"}.  n is the length of whichever of plan_index, state_index, alpha and noise is given (all the same), else the number of
    plans.  targets = (target_pos [P, T, F, 3], target_quat [P, T, F, 4], F) (rollout_osc): the plans are the targets', and ctrl
    [P, T, nu] may be None."""
    dev = sim.device
    f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)
    ctrl, gain, x_ref, kff, alpha, noise = f32(ctrl), f32(gain), f32(x_ref), f32(feedforward), f32(alpha), f32(noise)
    tp = tq = None
    if targets is not None:
        tp, tq, F = f32(targets[0]), f32(targets[1]), int(targets[2])
        if tp.dim() != 4 or tuple(tp.shape[2:]) != (F, 3):
            raise ValueError("%s: target_pos has shape %s, not [P, T, %d, 3]" % (what, tuple(tp.shape), F))
        P, T = int(tp.shape[0]), int(tp.shape[1])
        if tuple(tq.shape) != (P, T, F, 4):
            raise ValueError("%s: target_quat has shape %s, not [%d, %d, %d, 4]" % (what, tuple(tq.shape), P, T, F))
        if ctrl is not None and tuple(ctrl.shape) != (P, T, sim.nu):
            raise ValueError("%s: ctrl has shape %s, not [%d, %d, %d]" % (what, tuple(ctrl.shape), P, T, sim.nu))
    else:
        if ctrl.dim() != 3 or ctrl.shape[2] != sim.nu:
            raise ValueError("%s: ctrl has shape %s, not [P, T, %d]" % (what, tuple(ctrl.shape), sim.nu))
        P, T = int(ctrl.shape[0]), int(ctrl.shape[1])
    if kff is not None and kff.shape != ctrl.shape:
        raise ValueError("%s: feedforward has shape %s, not ctrl's %s" % (what, tuple(kff.shape), tuple(ctrl.shape)))
    dofs = [] if dofs is None else [int(d) for d in dofs]
    if gain is not None:
        nx = 2 * len(dofs)
        if not dofs:
            raise ValueError("%s: a gain needs dofs" % what)
        if gain.shape != (P, T, sim.nu, nx):
            raise ValueError("%s: gain has shape %s, not [%d, %d, %d, %d] (2 x %d dofs)" % (what, tuple(gain.shape), P, T, sim.nu, nx, len(dofs)))
        if x_ref is None or x_ref.shape != (P, T, nx):
            raise ValueError("%s: x_ref has shape %s, not [%d, %d, %d]" % (what, None if x_ref is None else tuple(x_ref.shape), P, T, nx))
    if alpha is not None and kff is None:
        raise ValueError("%s: alpha needs feedforward" % what)
    if noise is not None and (noise.dim() != 3 or tuple(noise.shape[1:]) != (T, sim.nu)):
        raise ValueError("%s: noise has shape %s, not [n, %d, %d]" % (what, tuple(noise.shape), T, sim.nu))
    q, v = _rows(qpos, dev, sim.nq), _rows(qvel, dev, sim.nv)
    if q is not None and v is not None and q.shape[0] != v.shape[0]:
        raise ValueError("%s: %d qpos rows but %d qvel rows" % (what, q.shape[0], v.shape[0]))
    nstates = sim.num_envs if q is None and v is None else (q if q is not None else v).shape[0]
    pidx, sidx = sim._index(plan_index), sim._index(state_index)
    alpha = None if alpha is None else alpha.reshape(-1).contiguous()
    counts = {k: t.numel() for k, t in (("plan_index", pidx), ("state_index", sidx), ("alpha", alpha)) if t is not None}
    if noise is not None:
        counts["noise"] = int(noise.shape[0])
    if len(set(counts.values())) > 1:
        raise ValueError("%s: %s" % (what, " but ".join("%d entries of %s" % (c, k) for k, c in counts.items())))
    n = next(iter(counts.values())) if counts else P
    c = lambda t: None if t is None else t.contiguous()
    plan = {"ctrl": c(ctrl), "kff": c(kff), "gain": c(gain), "xref": c(x_ref) if gain is not None else None, "target_pos": c(tp), "target_quat": c(tq)}
    return dict(plan=plan, alpha=alpha, plan_index=pidx, state_index=sidx, qpos=q, qvel=v, nstates=nstates, n=n, T=T, dofs=dofs, noise=c(noise))


class BatchedMujoco:
    def __init__(self, num_envs, robot_file="jaco2_curtain_torque", device=0, frame_skip=50, task=0, seed=0):
        if not torch.cuda.is_available():
            raise JacoError("BatchedMujoco needs a HIP device (no CPU path exists)")
        self.device = torch.device("cuda", device)
        self._blob = open(_lib.model_path(robot_file), "rb").read()
        self.L = _lib.load(_lib.variant_for(self._blob))
        self._blob_buf = ctypes.create_string_buffer(self._blob, len(self._blob))
        cfg = _lib.JacoConfig(ctypes.cast(self._blob_buf, ctypes.c_void_p), len(self._blob), int(num_envs), int(device),
                              int(frame_skip), int(task), int(seed))
        self.h = ctypes.c_void_p()
        rc = self.L.jaco_create(ctypes.byref(cfg), ctypes.byref(self.h))
        if rc != 0:
            raise JacoError("jaco_create failed (%d): %s" % (rc, self.L.jaco_last_error(None).decode()))
        dims = [ctypes.c_int() for _ in range(6)]
        self._chk(self.L.jaco_dims(self.h, *[ctypes.byref(d) for d in dims]))
        self.nq, self.nv, self.nu, self.nsensor, self.nobs, self.nact = [d.value for d in dims]
        self.num_envs = int(num_envs)
        self.robot_file = robot_file
        self.frames = FrameTable.for_model(robot_file)   # MJCF body name -> kernel frame (robot_config.py)
        # bumped by every call that changes the state (and by JacoBatchedEnv's reset / step / state setters): cached query results
        # (BatchedMujocoConfig) are valid while it stands still
        self.state_version = 0

    def _chk(self, rc):
        if rc != 0:
            raise JacoError("libjaco_env error %d: %s" % (rc, self.L.jaco_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.jaco_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _dev(self, t, n, dtype=torch.float32):
        if t is None:
            return None
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == self.num_envs * n, (t.shape, t.dtype, n)
        return ctypes.c_void_p(t.data_ptr())

    # ---- state (sim.get_state / set_state)
    def set_state(self, qpos=None, qvel=None, qacc_warmstart=None):
        self.state_version += 1
        self._chk(self.L.jaco_set_state(self.h, self._dev(qpos, self.nq), self._dev(qvel, self.nv),
                                        self._dev(qacc_warmstart, self.nv), self._stream()))

    def get_state(self):
        qpos = torch.empty(self.num_envs, self.nq, device=self.device)
        qvel = torch.empty(self.num_envs, self.nv, device=self.device)
        qacc = torch.empty(self.num_envs, self.nv, device=self.device)
        self._chk(self.L.jaco_get_state(self.h, self._dev(qpos, self.nq), self._dev(qvel, self.nv), self._dev(qacc, self.nv), self._stream()))
        return qpos, qvel, qacc

    def state_views(self):
        """Copies of (qpos, qvel, qacc_warmstart) as [num_envs, n] tensors on the current stream."""
        return self.get_state()

    def reset_state(self):
        self.state_version += 1
        self._chk(self.L.jaco_reset_state(self.h, self._stream()))

    # ---- env snapshots (jaco_save_envs / jaco_load_envs: sim.get_state / set_state as a full-state pair, per env)
    @property
    def snapshot_words(self):
        """W: 32-bit words of one snapshot row of this handle (a multiple of 4)."""
        if getattr(self, "_snap_w", None) is None:
            self._snap_w = int(self.L.jaco_snapshot_words(self.h))
        return self._snap_w

    def _index(self, idx):
        """An env / row index list as an int32 device tensor (no synchronisation); None stays None."""
        if idx is None:
            return None
        return torch.as_tensor(idx).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()

    def save_envs(self, envs=None, out=None):
        """rows [n, W] int32: row i = the complete state of env envs[i] (None: all envs in order) -- everything a later step reads of it
        (include/jaco_env.h, "env snapshots").  Rows are plain tensors: index, concatenate, move to the host, torch.save them.  `out`: a
        contiguous int32 device tensor [>= n, W] to write into (its first n rows are returned).  One kernel launch on the current stream."""
        e = self._index(envs)
        n = self.num_envs if e is None else e.numel()
        W = self.snapshot_words
        if out is None:
            out = torch.empty(n, W, dtype=torch.int32, device=self.device)
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == W and out.shape[0] >= n, (out.shape, out.dtype)
        self._chk(self.L.jaco_save_envs(self.h, ctypes.c_void_p(e.data_ptr()) if e is not None else None, n, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out[:n]

    def load_envs(self, rows, envs=None, row_index=None):
        """env envs[i] := rows[row_index[i]] (envs None: all envs in order; row_index None: row i).  The same row may go to many envs
        (fan-out); an env listed twice is undefined.  Out-of-range indices are skipped; a row of another build / model / task leaves its
        env untouched and sets JACO_FLAG_BAD_SNAPSHOT in flags().  The loaded envs continue bit for bit as the saved ones did (on another
        env index: on that index's random stream).  One kernel launch on the current stream."""
        rows = rows.to(device=self.device, dtype=torch.int32)
        rows = rows.reshape(-1, self.snapshot_words).contiguous()
        e, r = self._index(envs), self._index(row_index)
        n = e.numel() if e is not None else (r.numel() if r is not None else self.num_envs)
        if e is not None and r is not None and r.numel() != n:
            raise ValueError("load_envs: %d envs but %d row indices" % (n, r.numel()))
        self.state_version += 1
        self._chk(self.L.jaco_load_envs(self.h, ctypes.c_void_p(e.data_ptr()) if e is not None else None, n, ctypes.c_void_p(rows.data_ptr()), int(rows.shape[0]),
                                        ctypes.c_void_p(r.data_ptr()) if r is not None else None, self._stream()))

    # ---- send_forces
    def send_forces(self, ctrl, nsub=1):
        self.state_version += 1
        self._chk(self.L.jaco_physics_step(self.h, self._dev(ctrl, self.nu), int(nsub), self._stream()))

    def send_forces_debug(self, ctrl, env, nsub=1):
        n = self.L.jaco_debug_dump_floats()
        out = np.zeros(n, np.float32)
        torch.cuda.synchronize()
        self.state_version += 1
        self._chk(self.L.jaco_physics_step_debug(self.h, self._dev(ctrl, self.nu), int(nsub), int(env),
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n))
        return out

    # ---- robot-configuration queries (jaco_query; MujocoConfig: robot_config.BatchedMujocoConfig)
    def _query(self, frames, qpos, qvel, want):
        """One jaco_query launch: {name: tensor} of the outputs in `want` (names of JacoQueryOut), in the C ABI's layout.  qpos [B, nq] /
        qvel [B, nv] fp32 or None: contiguous device tensors."""
        nf, B, dev = len(frames), self.num_envs, self.device
        shapes = {"xpos": (B, nf, 3), "xmat": (B, nf, 9), "jac": (B, nf, 6, self.nv), "qM": (B, self.nv, self.nv), "qfrc_bias": (B, self.nv)}
        res = {k: torch.empty(shapes[k], device=dev) for k in want}
        out = _lib.JacoQueryOut(*[_ptr(res.get(k)) for k in shapes])
        arr = (_lib.JacoFrame * max(nf, 1))(*frames)
        self._chk(self.L.jaco_query(self.h, _ref(arr), nf, self._dev(qpos, self.nq), self._dev(qvel, self.nv), _ref(out), self._stream()))
        return res

    def query(self, frames, qpos=None, qvel=None, xpos=True, xmat=True, jac=True, qM=True, qfrc_bias=True):
        """One query launch on the current stream: {"xpos": [B, nf, 3], "xmat": [B, nf, 9], "jac": [B, nf, 6, nv], "qM": [B, nv, nv],
        "qfrc_bias": [B, nv]} (the outputs asked for) of the frames (_lib.JacoFrame list, FrameTable.jaco_frame) at the current state or at
        the given qpos [B, nq] / qvel [B, nv].  The values of a sim.forward() on that state; the handle's state is not touched."""
        on = {"xpos": xpos, "xmat": xmat, "jac": jac, "qM": qM, "qfrc_bias": qfrc_bias}
        return self._query(frames, qpos, qvel, tuple(k for k in on if on[k]))

    # ---- inverse kinematics (jaco_ik: a damped least-squares solve per env, one launch)
    def _ik(self, frame, seed, target_pos, target_quat, **options):
        """One jaco_ik launch: {"qpos": [B, nq], "resid": [B, 2] the last |e_p| / |e_r|, "status": [B, 2] int32 (iterations, converged)}.
        seed [B, nq], target_pos [B, 3], target_quat [B, 4] fp32, seed and target_quat or None: contiguous device tensors."""
        B, dev = self.num_envs, self.device
        res = {"qpos": torch.empty(B, self.nq, device=dev), "resid": torch.empty(B, 2, device=dev),
               "status": torch.empty(B, 2, dtype=torch.int32, device=dev)}
        opt = _lib.JacoIkOptions(**options)
        self._chk(self.L.jaco_ik(self.h, _ref(frame), _ref(opt), self._dev(seed, self.nq), self._dev(target_pos, 3), self._dev(target_quat, 4),
                                 _ptr(res["qpos"]), _ptr(res["resid"]), _ptr(res["status"]), self._stream()))
        return res

    def ik(self, frame, target_pos, target_quat=None, qpos=None, **options):
        """Which arm configuration puts `frame` (_lib.JacoFrame; FrameTable.jaco_frame(name, point=...): `point` is the controlled point)
        at target_pos [B, 3] and, if given, at the orientation target_quat [B, 4] (unit quaternions, w first)?  Seed: qpos [B, nq], default
        the current state.  options: tol_pos, tol_rot, damping, max_step, max_iters, dof_mask (include/jaco_env.h).  One launch on the
        current stream; {"qpos": [B, nq] the seed with the active dofs replaced, "converged": [B] bool, "iters": [B] int32, "err_pos" /
        "err_rot": [B] the last |e_p| / |e_r|}.  The sim's state is not touched: apply the result with set_state."""
        B, dev = self.num_envs, self.device
        tp, tq, seed = _rows(target_pos, dev, 3, B), _rows(target_quat, dev, 4, B), _rows(qpos, dev, self.nq, B)
        if tp is None:
            raise ValueError("ik: target_pos is required")
        r = self._ik(frame, seed, tp, tq, **options)
        status, resid = r["status"], r["resid"]
        return {"qpos": r["qpos"], "converged": status[:, 1] != 0, "iters": status[:, 0], "err_pos": resid[:, 0], "err_rot": resid[:, 1]}

    # ---- operational-space controller (jaco_osc: abr_control's OSC.generate per env and frame, one launch; jaco_osc_task: the same
    # with task axes and null-space terms)
    def _osc(self, frames, qpos, qvel, target_pos, target_quat, ctrl_in, task, rest_qpos, **options):
        """One jaco_osc launch (task None) or one jaco_osc_task launch (task: the keyword values of _lib.JacoOscTask): {"ctrl": [B, nu],
        "status": [B, nf] int32, non-zero where the pseudo-inverse branch ran}.  qpos [B, nq], qvel [B, nv], target_pos [B, 3 nf],
        target_quat [B, 4 nf], ctrl_in [B, nu], rest_qpos [B, nq] fp32, each but target_pos or None: contiguous device tensors."""
        nf, B, dev = len(frames), self.num_envs, self.device
        res = {"ctrl": torch.empty(B, self.nu, device=dev), "status": torch.empty(B, max(nf, 1), dtype=torch.int32, device=dev)}
        opt = _lib.JacoOscOptions(**options)
        arr = (_lib.JacoFrame * max(nf, 1))(*frames)
        head = (self.h, _ref(arr), nf, _ref(opt))
        state = (self._dev(qpos, self.nq), self._dev(qvel, self.nv), self._dev(target_pos, 3 * nf), self._dev(target_quat, 4 * nf))
        tail = (self._dev(ctrl_in, self.nu), _ptr(res["ctrl"]), _ptr(res["status"]), self._stream())
        if task is None:
            self._chk(self.L.jaco_osc(*head, *state, *tail))
        else:
            rec = _lib.JacoOscTask(**task)
            self._chk(self.L.jaco_osc_task(*head, _ref(rec), *state, self._dev(rest_qpos, self.nq), *tail))
        return res

    def osc(self, frames, target_pos, target_quat=None, qpos=None, qvel=None, ctrl=None, axes=None, null_kv=0.0, rest_qpos=None, rest_kp=0.0,
            rest_kv=0.0, rest_mask=0, **options):
        """The torques that drive `frames` (one or two _lib.JacoFrame; FrameTable.jaco_frame(name, point=...): `point` is the controlled
        point) towards target_pos [B, nf, 3] / target_quat [B, nf, 4] (unit quaternions, w first), from the values of a forward pass on
        qpos [B, nq] / qvel [B, nv] (default: the current state).  ctrl [B, nu]: the row the torques are written into (default zeros);
        only the motor actuators of the frames' active dofs change.  options: kp, ko, kv, vmax_xyz, vmax_abg, dof_mask
        (include/jaco_env.h).  One launch on the current stream, no synchronisation; {"ctrl": [B, nu], "singular": [B, nf] bool, True
        where the pseudo-inverse branch ran}.  The sim's state is not touched: apply the result with send_forces.
        Task axes and null-space terms (jaco_osc_task; with all of them at their defaults the call is jaco_osc): axes = one 6-bit mask
        (bit 0-2: x, y, z; bit 3-5: the rotational rows) or six booleans, or one of those per frame -- abr_control's ctrlr_dof;
        target_quat may be None when no rotational row is selected.  null_kv > 0: Damping(null_kv).  rest_qpos [B, nq]:
        RestingConfig(rest_kp, rest_kv) towards those joint angles on the dofs of rest_mask (bit d = dof d; 0: every active dof), read
        only at those dofs' qpos addresses.  Both act in the null space of the selected task rows."""
        if isinstance(frames, _lib.JacoFrame):
            frames = [frames]
        nf, B, dev = len(frames), self.num_envs, self.device
        tp, tq = _rows(target_pos, dev, 3 * nf, B), _rows(target_quat, dev, 4 * nf, B)
        q, v, cin = _rows(qpos, dev, self.nq, B), _rows(qvel, dev, self.nv, B), _rows(ctrl, dev, self.nu, B)
        if axes is None and null_kv == 0.0 and rest_qpos is None and rest_kp == 0.0 and rest_kv == 0.0 and rest_mask == 0:
            task = None
        else:
            task = dict(axes=_lib.osc_axes(axes, nf), null_kv=null_kv, rest_kp=rest_kp, rest_kv=rest_kv, rest_mask=rest_mask)
        r = self._osc(frames, q, v, tp, tq, cin, task, _rows(rest_qpos, dev, self.nq, B), **options)
        return {"ctrl": r["ctrl"], "singular": r["status"] != 0}

    # ---- joint-space controller and inverse dynamics (jaco_joint: abr_control's Joint.generate per env, one launch)
    def _joint(self, qpos, qvel, target_qpos, target_qvel, qacc_ff, ctrl_in, **options):
        """One jaco_joint launch: ctrl [B, nu].  qpos / target_qpos [B, nq], qvel / target_qvel / qacc_ff [B, nv], ctrl_in [B, nu] fp32,
        each or None: contiguous device tensors."""
        out = torch.empty(self.num_envs, self.nu, device=self.device)
        opt = _lib.JacoJointOptions(**options)
        self._chk(self.L.jaco_joint(self.h, _ref(opt), self._dev(qpos, self.nq), self._dev(qvel, self.nv), self._dev(target_qpos, self.nq),
                                    self._dev(target_qvel, self.nv), self._dev(qacc_ff, self.nv), self._dev(ctrl_in, self.nu), _ptr(out), self._stream()))
        return out

    def joint(self, target_qpos=None, target_qvel=None, qacc=None, qpos=None, qvel=None, ctrl=None, **options):
        """The torques that drive the arm to the configuration target_qpos [B, nq] (read only at the qpos addresses of the active dofs: a
        row of ik()["qpos"] goes in as it is) with the joint velocities target_qvel [B, nv] and the feed-forward accelerations qacc
        [B, nv] (each None: zeros; without target_qpos there is no position term and kp must be 0), from the values of a forward pass
        on qpos [B, nq] / qvel [B, nv] (default: the current state):  u = M[A, A] (qacc + kp s e + kv (target_qvel - qvel)) + qfrc_bias
        on the active dofs A, e the joint error (wrapped into [-pi, pi) on unlimited joints only), s the velocity limit's one scale.
        ctrl [B, nu]: the row the torques are written into (default zeros); only the motor actuators of the active dofs change.
        options: kp, kv, vmax, dof_mask (include/jaco_env.h; dof_mask 0: every hinge dof with a motor actuator).  kp = kv = 0 with qacc
        is inverse dynamics; kp = kv = 0 with nothing else is bias compensation.  One launch on the current stream, no synchronisation;
        returns the ctrl tensor [B, nu].  The sim's state is not touched: apply the result with send_forces."""
        B, dev = self.num_envs, self.device
        tq, tv, ff = _rows(target_qpos, dev, self.nq, B), _rows(target_qvel, dev, self.nv, B), _rows(qacc, dev, self.nv, B)
        q, v, cin = _rows(qpos, dev, self.nq, B), _rows(qvel, dev, self.nv, B), _rows(ctrl, dev, self.nu, B)
        return self._joint(q, v, tq, tv, ff, cin, **options)

    # ---- forward dynamics and its linearisation (jaco_fd: qacc_smooth of a forward pass and its derivatives per env, one launch)
    def _fd(self, ctrl, qpos, qvel, want, **options):
        """One jaco_fd launch: {name: tensor} of the outputs in `want` (names of JacoFdOut), in the C ABI's layout."""
        B, dev = self.num_envs, self.device
        c, q, v = _rows(ctrl, dev, self.nu, B), _rows(qpos, dev, self.nq, B), _rows(qvel, dev, self.nv, B)
        shapes = {"qacc": (B, self.nv), "qfrc_smooth": (B, self.nv), "dqacc_dqpos": (B, self.nv, self.nv), "dqacc_dqvel": (B, self.nv, self.nv),
                  "dqacc_dctrl": (B, self.nu, self.nv)}
        res = {k: torch.empty(shapes[k], device=dev) for k in want}
        out = _lib.JacoFdOut(*[_ptr(res.get(k)) for k in shapes])
        opt = _lib.JacoFdOptions(**options)
        self._chk(self.L.jaco_fd(self.h, _ref(opt), self._dev(q, self.nq), self._dev(v, self.nv), self._dev(c, self.nu), _ref(out), self._stream()))
        return res

    def forward_dynamics(self, ctrl=None, qpos=None, qvel=None, implicit_damping=False, want_qfrc=False):
        """qacc [B, nv]: the acceleration that ctrl [B, nu] (None: zeros) produces at qpos [B, nq] / qvel [B, nv] (default: the current
        state) -- data.qacc_smooth after a forward pass: M^-1 qfrc_smooth, qfrc_smooth = passive - bias + actuator, the actuators as
        the step applies them (ctrlrange, the fingers' position servos, forcerange).  UNCONSTRAINED: no contacts, no joint limits.
        implicit_damping=True: (M + h D)^-1 qfrc_smooth, what a contact-free substep adds to qvel per h.  want_qfrc=True: (qacc,
        qfrc_smooth).  One launch on the current stream, no synchronisation; the sim's state is not touched."""
        r = self._fd(ctrl, qpos, qvel, ("qacc", "qfrc_smooth") if want_qfrc else ("qacc",), implicit_damping=int(bool(implicit_damping)))
        return (r["qacc"], r["qfrc_smooth"]) if want_qfrc else r["qacc"]

    def linearize(self, ctrl=None, qpos=None, qvel=None, dofs=None, eps_qpos=_lib.JacoFdOptions.DEFAULTS["eps_qpos"],
                  eps_qvel=_lib.JacoFdOptions.DEFAULTS["eps_qvel"], implicit_damping=True):
        """{"qacc": [B, nv], "dq": [B, nv, nv], "dv": [B, nv, nv], "du": [B, nv, nu]}: forward_dynamics and its Jacobians with respect to
        the hinge coordinates, the joint velocities and the ctrl (dq[b, i, j] = d qacc_i / d q_j, j a dof index), from ONE launch: central
        differences of half-width eps_qpos / eps_qvel for dq / dv (the whole chain re-evaluated, the servos included), analytic du
        (exactly zero for an actuator held by its ctrlrange or forcerange).  dofs: the hinge dofs to differentiate by (default: all of
        them); the other columns of dq and dv are zero.  The returned Jacobians are transposed views of the kernel's row-per-perturbation
        arrays."""
        mask = 0 if dofs is None else sum(1 << int(d) for d in dofs)
        if dofs is not None and not mask:
            raise ValueError("linearize: an empty dof list")
        r = self._fd(ctrl, qpos, qvel, ("qacc", "dqacc_dqpos", "dqacc_dqvel", "dqacc_dctrl"), eps_qpos=eps_qpos, eps_qvel=eps_qvel,
                     implicit_damping=int(bool(implicit_damping)), dof_mask=mask)
        return {"qacc": r["qacc"], "dq": r["dqacc_dqpos"].transpose(1, 2), "dv": r["dqacc_dqvel"].transpose(1, 2), "du": r["dqacc_dctrl"].transpose(1, 2)}

    # ---- open-loop rollouts (jaco_rollout: n rollouts of T knots x hold contact-free substeps, one launch)
    def _launch_rollout(self, entry, Options, Out, options, head, frame, n, state_index, nstates, qpos, qvel, inputs, want):
        """What the launches of the rollout family share: {name: tensor} of the outputs in `want`, allocated from the family's shape
        table (`Out`, the entry's JacoRollout*Out record, holds the first of its names); no launch for n == 0 (every entry returns
        JACO_OK then); else entry(handle, options, *head, frame, n, state_index, nstates, qpos, qvel, *inputs, out, stream), its return
        code checked.  Options: the entry's options record, built from the keywords `options`; head, inputs: what the entry takes
        before the output frame and after the states, as the C ABI's pointers."""
        T = options["nknots"]
        rows = 1 if options.get("final_only") else T
        evals = T * (options["hold"] if options.get("per_substep", Options.DEFAULTS.get("per_substep")) else 1)
        shapes = {"qpos": (n, rows, self.nq), "qvel": (n, rows, self.nv), "xpos": (n, rows, 3), "xmat": (n, rows, 9), "status": (n,),
                  "ctrl": (n, max(evals, 0), self.nu), "cost": (n,), "terms": (n, 3)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "status" else torch.float32, device=self.device) for k in want}
        if n == 0:   # (no launch: the entry returns JACO_OK for n == 0)
            return res
        opt, out = Options(**options), Out(*[_ptr(res.get(k)) for k, _ in Out._fields_])
        self._chk(entry(self.h, _ref(opt), *head, None if frame is None else _ref(frame), n, _ptr(state_index), int(nstates), _ptr(qpos), _ptr(qvel), *inputs,
                        _ref(out), self._stream()))
        return res

    def _rollout(self, ctrl, qpos, qvel, state_index, nstates, frame, want, **options):
        """One jaco_rollout launch: {name: tensor} of the outputs in `want` (names of JacoRolloutOut), in the C ABI's layout.  ctrl
        [n, nknots, nu] fp32, qpos / qvel [nstates, ..] fp32 or None, state_index [n] int32 or None: contiguous device tensors."""
        return self._launch_rollout(self.L.jaco_rollout, _lib.JacoRolloutOptions, _lib.JacoRolloutOut, options, (), frame, ctrl.shape[0], state_index, nstates,
                                    qpos, qvel, (_ptr(ctrl),), want)

    def rollout(self, ctrl, qpos=None, qvel=None, state_index=None, hold=1, frame=None, final_only=False):
        """What happens over the next T x hold substeps if the ctrl sequences ctrl [n, T, nu] are applied?  mujoco.rollout.rollout,
        contact-free: rollout i starts from row state_index[i] ([n] integers; None: row i) of qpos [nstates, nq] / qvel [nstates, nv]
        (both, or neither: the current state of the num_envs envs) with a zero warm start, and holds ctrl[i, k] for `hold` substeps in
        knot k.  Every substep is the one send_forces runs under option "disable_contact": joint limits are in, contacts are not, free
        bodies fall.  n is not tied to num_envs: K sequences per env share a state row through state_index.
        {"qpos": [n, T, nq], "qvel": [n, T, nv]: the state after each knot;  "status": [n] int32, JACO_FLAG_NAN / JACO_FLAG_SOLVER_MAXITER
        of the rollout, or _lib.JACO_ROLLOUT_BAD_INDEX where state_index was outside [0, nstates): those rollouts' rows are left
        unwritten} plus, with frame (_lib.JacoFrame; FrameTable.jaco_frame), {"xpos": [n, T, 3], "xmat": [n, T, 9]}: the frame's pose
        after each knot.  final_only=True: the arrays have one knot row, the last.  One launch on the current stream, no
        synchronisation; the sim's state is not touched."""
        dev = self.device
        ctrl = torch.as_tensor(ctrl, dtype=torch.float32, device=dev)
        if ctrl.dim() != 3 or ctrl.shape[2] != self.nu:
            raise ValueError("rollout: ctrl has shape %s, not [n, T, %d]" % (tuple(ctrl.shape), self.nu))
        n = ctrl.shape[0]
        q, v = _rows(qpos, dev, self.nq), _rows(qvel, dev, self.nv)
        if q is not None and v is not None and q.shape[0] != v.shape[0]:
            raise ValueError("rollout: %d qpos rows but %d qvel rows" % (q.shape[0], v.shape[0]))
        nstates = self.num_envs if q is None and v is None else (q if q is not None else v).shape[0]
        idx = self._index(state_index)
        if idx is not None and idx.numel() != n:
            raise ValueError("rollout: %d ctrl sequences but %d state indices" % (n, idx.numel()))
        want = ("qpos", "qvel", "status") + (("xpos", "xmat") if frame is not None else ())
        return self._rollout(ctrl.contiguous(), q, v, idx, nstates, frame, want, nknots=int(ctrl.shape[1]), hold=int(hold), final_only=int(bool(final_only)))

    # ---- closed-loop rollouts (jaco_rollout_fb: jaco_rollout with the feedback law evaluated inside the kernel, one launch)
    def _rollout_fb(self, plan, alpha, plan_index, qpos, qvel, state_index, nstates, frame, want, n, **options):
        """One jaco_rollout_fb launch: {name: tensor} of the outputs in `want` (names of JacoRolloutFbOut), in the C ABI's layout.  plan:
        {"ctrl": [P, nknots, nu], "kff", "gain", "xref": tensors or None}; alpha [n] fp32, plan_index / state_index [n] int32, qpos / qvel
        [nstates, ..] fp32, each or None: contiguous device tensors."""
        rec = _plan_record(plan, alpha, plan_index)
        return self._launch_rollout(self.L.jaco_rollout_fb, _lib.JacoRolloutFbOptions, _lib.JacoRolloutFbOut, options, (), frame, n, state_index, nstates,
                                    qpos, qvel, (_ref(rec),), want)

    def rollout_feedback(self, ctrl, qpos=None, qvel=None, gain=None, x_ref=None, dofs=None, feedforward=None, alpha=None, plan_index=None,
                         state_index=None, hold=1, per_substep=False, frame=None, final_only=False):
        """rollout() in closed loop: the ctrl of knot k is computed inside the kernel from the state at knot k,
            u = ctrl[p, k] + alpha[i] * feedforward[p, k] + gain[p, k] @ (x - x_ref[p, k]),   x = [qpos at the hinge dofs `dofs`, qvel at them]
        (include/jaco_env.h states the exact fp32 order; the difference is not wrapped; u is clamped to ctrlrange by the actuators as any
        ctrl is) -- the forward pass of iLQR and its line search, a plan tracked with TVLQR gains, PD tracking.  Plans: ctrl [P, T, nu],
        gain [P, T, nu, 2 nd] with x_ref [P, T, 2 nd] and dofs (nd <= 18 hinge dofs), feedforward [P, T, nu]; each of gain and feedforward
        may be None.  Rollout i follows plan plan_index[i] (None: plan i) from state row state_index[i] (None: row i) of qpos / qvel (as
        rollout()) with the step alpha[i] (None: 1; needs feedforward): n is the length of whichever of plan_index, state_index and alpha
        is given (all the same), else P.  per_substep=False: the law is evaluated at the start of a knot and held for its `hold`
        substeps; True: before every substep, against the same knot's rows.
        Returns rollout()'s dict plus "ctrl" [n, E, nu]: the u of every evaluation as commanded (E = T, or T * hold with per_substep),
        all E rows also with final_only.  status: _lib.JACO_ROLLOUT_BAD_INDEX where plan_index or state_index was out of range.  One
        launch on the current stream, no synchronisation; the sim's state is not touched."""
        a = _closed_loop_args(self, "rollout_feedback", ctrl, qpos, qvel, gain, x_ref, dofs, feedforward, alpha, plan_index, state_index)
        want = ("qpos", "qvel", "status", "ctrl") + (("xpos", "xmat") if frame is not None else ())
        return self._rollout_fb(a["plan"], a["alpha"], a["plan_index"], a["qpos"], a["qvel"], a["state_index"], a["nstates"], frame, want, a["n"], nknots=a["T"],
                                hold=int(hold), final_only=int(bool(final_only)), per_substep=int(bool(per_substep)), dofs=a["dofs"] if a["plan"]["gain"] is not None else ())

    # ---- costed rollouts (jaco_rollout_cost: jaco_rollout_fb with noise added and the running cost accumulated inside the kernel, one launch)
    def _rollout_cost(self, plan, goal, alpha, plan_index, qpos, qvel, state_index, nstates, frame, want, n, **options):
        """One jaco_rollout_cost launch: {name: tensor} of the outputs in `want` (names of JacoRolloutCostOut), in the C ABI's layout.
        plan: as _rollout_fb's; goal: {"noise": [n, nknots, nu], "xgoal": [P, G, nx], "pgoal": [P, G, 3]: tensors or None}; options: the
        keywords of _lib.JacoRolloutCostOptions."""
        rec = _plan_record(plan, alpha, plan_index)
        g = _lib.JacoRolloutGoal(_ptr(goal.get("noise")), _ptr(goal.get("xgoal")), _ptr(goal.get("pgoal")))
        return self._launch_rollout(self.L.jaco_rollout_cost, _lib.JacoRolloutCostOptions, _lib.JacoRolloutCostOut, options, (), frame, n, state_index, nstates,
                                    qpos, qvel, (_ref(rec), _ref(g)), want)

    def rollout_cost(self, ctrl, qpos=None, qvel=None, noise=None, gain=None, x_ref=None, dofs=None, feedforward=None, alpha=None, plan_index=None,
                     state_index=None, hold=1, frame=None, x_goal=None, p_goal=None, wx=None, wx_final=None, wu=None, wp=0.0, wp_final=0.0,
                     want=("cost", "terms", "status"), final_only=False):
        """rollout_feedback() costed inside the kernel -- what MPPI, CEM, random shooting and iLQR's line search want of a rollout: one
        number.  The plans, the law (evaluated once per knot), the states and the indices are rollout_feedback()'s.  noise [n, T, nu]:
        added to the law's u in one fp32 add; the sum is applied and is what "ctrl" holds.  The cost of rollout i on plan p,
            J = sum_k [ 1/2 sum_a wu[a] u_ka^2 + 1/2 sum_j WX_k[j] (x_(k+1)j - x_goal[p, g, j])^2 + 1/2 WP_k |pos_(k+1) - p_goal[p, g]|^2 ],
        x = [qpos at the hinge dofs `dofs`, qvel at them] and pos the position of `frame` after knot k (the words row k of "qpos" /
        "qvel" / "xpos" holds), (WX, WP) = (wx, wp) on the running knots and (wx_final, wp_final) on the last; differences are not
        wrapped.  Goals: x_goal [P, 2 nd] or [P, T, 2 nd], p_goal [P, 3] or [P, T, 3] (one goal per plan, or one per plan and knot; both
        the same way).  Weights: wx / wx_final [2 nd], wu [nu] (scalars broadcast), wp / wp_final scalars, all finite and >= 0; None: zeros.
        Returns only the tensors named in `want`, of "cost" [n], "terms" [n, 3] (the ctrl, state and pose parts), "status" [n] and
        rollout_feedback()'s "qpos", "qvel", "xpos", "xmat", "ctrl"; a rollout whose status has JACO_FLAG_NAN has cost = terms = +inf.
        cost and terms do not depend on `want` or final_only, bit for bit.  One launch on the current stream, no synchronisation; the
        sim's state is not touched."""
        what = "rollout_cost"
        a = _closed_loop_args(self, what, ctrl, qpos, qvel, gain, x_ref, dofs, feedforward, alpha, plan_index, state_index, noise)
        dev, P, T, nx = self.device, int(a["plan"]["ctrl"].shape[0]), a["T"], 2 * len(a["dofs"])
        known = ("qpos", "qvel", "xpos", "xmat", "status", "ctrl", "cost", "terms")
        want = tuple(want)
        if not want or set(want) - set(known):
            raise ValueError("%s: want %s names none or not only outputs (%s)" % (what, want, ", ".join(known)))

        def goal(t, width, name):
            if t is None:
                return None, None
            t = torch.as_tensor(t, dtype=torch.float32, device=dev)
            if tuple(t.shape) == (P, width):
                return t.reshape(P, 1, width).contiguous(), 0
            if tuple(t.shape) == (P, T, width):
                return t.contiguous(), 1
            raise ValueError("%s: %s has shape %s, not [%d, %d] or [%d, %d, %d]" % (what, name, tuple(t.shape), P, width, P, T, width))
        xg, per_x = goal(x_goal, nx, "x_goal")
        pg, per_p = goal(p_goal, 3, "p_goal")
        if per_x is not None and per_p is not None and per_x != per_p:
            raise ValueError("%s: x_goal is given per %s but p_goal per %s" % (what, *[("plan", "plan and knot")[m] for m in (per_x, per_p)]))

        def weights(w, width, name):
            if w is None:
                return ()
            w = np.asarray(torch.as_tensor(w).detach().cpu().numpy() if torch.is_tensor(w) else w, np.float64)
            if w.ndim == 0:
                w = np.full(width, float(w))
            if w.shape != (width,):
                raise ValueError("%s: %s has shape %s, not [%d]" % (what, name, tuple(w.shape), width))
            return w
        options = dict(nknots=T, hold=int(hold), final_only=int(bool(final_only)), goal_per_knot=int(bool(per_x or per_p)),
                       dofs=a["dofs"] if (a["plan"]["gain"] is not None or xg is not None) else (),
                       wx=weights(wx, nx, "wx"), wxT=weights(wx_final, nx, "wx_final"), wu=weights(wu, self.nu, "wu"), wp=float(wp), wpT=float(wp_final))
        return self._rollout_cost(a["plan"], {"noise": a["noise"], "xgoal": xg, "pgoal": pg}, a["alpha"], a["plan_index"], a["qpos"], a["qvel"],
                                  a["state_index"], a["nstates"], frame, want, a["n"], **options)

    # ---- rollouts under the operational-space controller (jaco_rollout_osc: jaco_rollout with jaco_osc's law inside the substep, one launch)
    def _rollout_osc(self, frames, plan, plan_index, qpos, qvel, state_index, nstates, frame, want, n, **options):
        """One jaco_rollout_osc launch: {name: tensor} of the outputs in `want` (names of JacoRolloutFbOut), in the C ABI's layout.
        frames: the controlled _lib.JacoFrame list; plan: {"ctrl": [P, nknots, nu] or None, "target_pos": [P, nknots, F, 3], "target_quat":
        [P, nknots, F, 4]}; frame: the output frame or None; options: the keywords of _lib.JacoRolloutOscOptions (nframes is set here)."""
        nf = len(frames)
        rec = _lib.JacoRolloutOscPlan(_ptr(plan.get("ctrl")), _ptr(plan["target_pos"]), _ptr(plan["target_quat"]), _ptr(plan_index), int(plan["target_pos"].shape[0]))
        arr = (_lib.JacoFrame * max(nf, 1))(*frames)
        return self._launch_rollout(self.L.jaco_rollout_osc, _lib.JacoRolloutOscOptions, _lib.JacoRolloutFbOut, dict(options, nframes=nf), (_ref(arr), nf), frame, n,
                                    state_index, nstates, qpos, qvel, (_ref(rec),), want)

    def rollout_osc(self, frames, target_pos, target_quat, qpos=None, qvel=None, ctrl=None, plan_index=None, state_index=None, hold=1, per_substep=True,
                    frame=None, final_only=False, **options):
        """rollout() under the operational-space controller: where are the arm and the hand after T x hold substeps of driving `frames`
        (one or two _lib.JacoFrame, as osc()) towards target_pos [P, T, F, 3] / target_quat [P, T, F, 4] (unit quaternions, w first)?
        The motor words of the ctrl are osc()'s law, evaluated inside the kernel on each substep's own mass matrix, bias and poses --
        before every substep (per_substep=True: the env's own loop of "OSC towards the target, then a substep"), or in the first substep
        of a knot and held for its `hold` substeps (False).  ctrl [P, T, nu]: the base rows the torques are written into (None:
        zeros); only the motor actuators of the frames' active dofs change, gripper commands and the other arm's words go through.
        Rollout i follows plan plan_index[i] (None: plan i) from state row state_index[i] (None: row i) of qpos / qvel (as rollout()):
        n is the length of whichever index is given (both the same), else P; K target samples of an env share its state row.
        options: kp, ko, kv, vmax_xyz, vmax_abg, dof_mask (include/jaco_env.h).  No task axes, no null-space terms, no contacts.
        Returns rollout_feedback()'s dict: "qpos", "qvel", "status", "ctrl" [n, E, nu] (the commanded row of every evaluation, E = T * hold
        or T, all rows also with final_only) and, with frame (one _lib.JacoFrame, controlled or not), "xpos", "xmat".  status carries
        _lib.JACO_ROLLOUT_OSC_SINGULAR0 / _SINGULAR1 when frame 0 / 1 took the pseudo-inverse branch at some evaluation.  One launch on
        the current stream, no synchronisation; the sim's state is not touched."""
        if isinstance(frames, _lib.JacoFrame):
            frames = [frames]
        a = _closed_loop_args(self, "rollout_osc", ctrl, qpos, qvel, None, None, None, None, None, plan_index, state_index,
                              targets=(target_pos, target_quat, len(frames)))
        want = ("qpos", "qvel", "status", "ctrl") + (("xpos", "xmat") if frame is not None else ())
        return self._rollout_osc(list(frames), a["plan"], a["plan_index"], a["qpos"], a["qvel"], a["state_index"], a["nstates"], frame, want, a["n"],
                                 nknots=a["T"], hold=int(hold), final_only=int(bool(final_only)), per_substep=int(bool(per_substep)), **options)

    # ---- transition Jacobians of the rollout step (jaco_transition_fd: finite differences of `hold` substeps over n pairs, one launch)
    def _transition(self, ctrl, qpos, qvel, n, want, **options):
        """One jaco_transition_fd launch: {name: tensor} of the outputs in `want` (names of JacoTransitionOut), in the C ABI's layout.
        ctrl [n, nu] fp32 or None, qpos [n, nq] / qvel [n, nv] fp32 or None: contiguous device tensors; options: the keywords of
        _lib.JacoTransitionOptions."""
        nx, na = 2 * len(options["dofs"]), len(options["acts"])
        shapes = {"A": (n, nx, nx), "B": (n, nx, na), "next_qpos": (n, self.nq), "next_qvel": (n, self.nv), "status": (n,)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "status" else torch.float32, device=self.device) for k in want}
        if n == 0:   # (no launch: the entry returns JACO_OK for n == 0)
            return res
        opt, out = _lib.JacoTransitionOptions(**options), _lib.JacoTransitionOut(*[_ptr(res.get(k)) for k in shapes])
        self._chk(self.L.jaco_transition_fd(self.h, _ref(opt), int(n), _ptr(qpos), _ptr(qvel), _ptr(ctrl), _ref(out), self._stream()))
        return res

    def transition_fd(self, ctrl, qpos=None, qvel=None, dofs=(), acts=(), hold=1, centered=True, groups=None,
                      eps_qpos=_lib.JacoTransitionOptions.DEFAULTS["eps_qpos"], eps_qvel=_lib.JacoTransitionOptions.DEFAULTS["eps_qvel"],
                      eps_ctrl=_lib.JacoTransitionOptions.DEFAULTS["eps_ctrl"], want=("A", "B")):
        """The transition Jacobians of the step the rollouts simulate -- mjd_transitionFD on `hold` contact-free substeps, joint-limit
        rows and their warm-started solve included: x' = f(x, u), A = df/dx, B = df/du with x = [qpos at the hinge dofs `dofs`, qvel at
        them] (rollout_feedback's convention) and u = ctrl at the words `acts`, by central (centered=False: forward) differences of
        half-width eps_qpos / eps_qvel / eps_ctrl, formed on the increments of the compensated state (include/jaco_env.h states the
        exact fp32 order).  ctrl [..., nu] (None: zeros) with qpos [..., nq] / qvel [..., nv] of the same leading shape (both, or neither:
        the current state of the num_envs envs): the pairs are not tied to num_envs -- every knot of every trajectory, straight from
        rollout_feedback's outputs.  groups: wavefronts per pair (None: the library chooses from the number of pairs).
        Returns, for what `want` names: {"A": [..., nx, nx], "B": [..., nx, na]: the layout lqr_backward reads;  "next_qpos": [..., nq],
        "next_qvel": [..., nv], "status": [...] int32: the nominal step, rollout(hold=hold)'s bits on one knot}.  One launch on the
        current stream, no synchronisation; the sim's state is not touched."""
        dev = self.device
        known = ("A", "B", "next_qpos", "next_qvel", "status")
        want = tuple(want)
        if not want or set(want) - set(known):
            raise ValueError("transition_fd: want %s names none or not only outputs (%s)" % (want, ", ".join(known)))
        given = [(name, torch.as_tensor(t, dtype=torch.float32, device=dev), width) for name, t, width in
                 (("ctrl", ctrl, self.nu), ("qpos", qpos, self.nq), ("qvel", qvel, self.nv)) if t is not None]
        lead = None
        for name, t, width in given:
            if t.dim() < 1 or t.shape[-1] != width:
                raise ValueError("transition_fd: %s has shape %s, not [..., %d]" % (name, tuple(t.shape), width))
            if lead is not None and tuple(t.shape[:-1]) != lead:
                raise ValueError("transition_fd: %s has the leading shape %s, not %s" % (name, tuple(t.shape[:-1]), lead))
            lead = tuple(t.shape[:-1])
        if (qpos is None) != (qvel is None):
            raise ValueError("transition_fd: qpos and qvel are given together or not at all")
        if lead is None or qpos is None:
            if lead not in (None, (self.num_envs,)):
                raise ValueError("transition_fd: ctrl has the leading shape %s, but the current state has %d envs" % (lead, self.num_envs))
            lead = (self.num_envs,)
        n = int(np.prod(lead, dtype=np.int64))
        c, q, v = (_rows(t, dev, width) for t, width in ((ctrl, self.nu), (qpos, self.nq), (qvel, self.nv)))
        r = self._transition(c, q, v, n, want, dofs=tuple(int(d) for d in dofs), acts=tuple(int(a) for a in acts), hold=int(hold),
                             centered=int(bool(centered)), groups=0 if groups is None else int(groups), eps_qpos=float(eps_qpos), eps_qvel=float(eps_qvel),
                             eps_ctrl=float(eps_ctrl))
        return {k: t.reshape(lead + tuple(t.shape[1:])) for k, t in r.items()}

    # ---- the quadratic expansion of rollout_cost's cost along trajectories (jaco_cost_quad: R x T work items, one launch)
    def _cost_quad(self, qpos, qvel, ctrl, goal, frame, R, T, want, **options):
        """One jaco_cost_quad launch: {name: tensor} of the outputs in `want` (names of JacoCostQuadOut), in the C ABI's layout.  qpos
        [R, T, nq] / qvel [R, T, nv] / ctrl [R, T, nu] fp32 or None; goal: {"xgoal": [P, G, nx], "pgoal": [P, G, 3], "goal_idx": [R] int32:
        tensors or None, "ngoals": P}; options: the keywords of _lib.JacoCostQuadOptions."""
        nx, na = 2 * len(options["dofs"]), len(options["acts"])
        shapes = {"lx": (R, T, nx), "lxx": (R, T, nx, nx), "lu": (R, T, na), "Vx": (R, nx), "Vxx": (R, nx, nx), "l": (R, T), "status": (R, T)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "status" else torch.float32, device=self.device) for k in want}
        opt = _lib.JacoCostQuadOptions(**options)
        if R == 0:   # (no launch, as the entry for R == 0; empty tensors have no address to hand it, so what it would refuse is not seen here)
            return res
        out = _lib.JacoCostQuadOut(*[_ptr(res.get(k)) for k, _ in _lib.JacoCostQuadOut._fields_])
        g = _lib.JacoCostQuadGoal(_ptr(goal.get("xgoal")), _ptr(goal.get("pgoal")), _ptr(goal.get("goal_idx")), int(goal.get("ngoals", 0)))
        self._chk(self.L.jaco_cost_quad(self.h, _ref(opt), None if frame is None else _ref(frame), int(R), _ptr(qpos), _ptr(qvel), _ptr(ctrl), _ref(g), _ref(out),
                                        self._stream()))
        return res

    def cost_quad(self, qpos, qvel, ctrl=None, dofs=(), acts=(), frame=None, x_goal=None, p_goal=None, goal_index=None, wx=None, wx_final=None,
                  wu=None, wp=0.0, wp_final=0.0, want=("lx", "lxx", "lu", "Vx", "Vxx", "l", "status")):
        """The quadratic expansion of rollout_cost()'s cost along R trajectories of T knots, in the layout lqr_backward reads -- iLQR's cost
        expansion in one launch.  qpos [R, T, nq], qvel [R, T, nv]: the state AFTER each knot (x_1 .. x_T), ctrl [R, T, nu] (None: zeros):
        the commanded row of each knot -- rollout_feedback's / rollout_cost's outputs as they are.  x = [qpos at the hinge dofs `dofs`,
        qvel at them] (2 nd), u = ctrl at the words `acts`; goals x_goal [P, 2 nd] or [P, T, 2 nd], p_goal [P, 3] or [P, T, 3] (both the
        same way), trajectory r taking goal goal_index[r] (None: goal r); weights wx / wx_final [2 nd], wu [len(acts)] (scalars broadcast),
        wp / wp_final, all finite and >= 0, None: zeros.  The cost is rollout_cost()'s, re-indexed to lqr_backward's convention: l_t(x_t,
        u_t) for t < T -- the start state is not costed, so row 0 of lx / lxx is zero -- and a terminal cost on x_T with the final weights.
        The pose term is expanded in Gauss-Newton form on the positional Jacobian of `frame`'s origin (include/jaco_env.h).
        Returns, for what `want` names: {"lx": [R, T, 2 nd], "lxx": [R, T, 2 nd, 2 nd], "lu": [R, T, na], "Vx": [R, 2 nd], "Vxx": [R, 2 nd,
        2 nd], "l": [R, T]: knot k's own summand of rollout_cost()'s cost, "status": [R, T] int32: JACO_FLAG_NAN, or
        _lib.JACO_ROLLOUT_BAD_INDEX where goal_index was out of range: that item wrote nothing else}; luu is diag(wu) and lux zero.  No
        output depends on `want`.  One launch on the current stream, no synchronisation; the sim's state is not touched."""
        what, dev = "cost_quad", self.device
        known = ("lx", "lxx", "lu", "Vx", "Vxx", "l", "status")
        want = tuple(want)
        if not want or set(want) - set(known):
            raise ValueError("%s: want %s names none or not only outputs (%s)" % (what, want, ", ".join(known)))
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
        qpos, qvel, ctrl = f32(qpos), f32(qvel), f32(ctrl)
        lead = None
        for name, t, width in (("qpos", qpos, self.nq), ("qvel", qvel, self.nv), ("ctrl", ctrl, self.nu)):
            if t is None:
                continue
            if t.dim() != 3 or t.shape[2] != width or (lead is not None and tuple(t.shape[:2]) != lead):
                raise ValueError("%s: %s has shape %s, not [%s, %d]" % (what, name, tuple(t.shape), "R, T" if lead is None else "%d, %d" % lead, width))
            lead = tuple(t.shape[:2])
        if lead is None:
            raise ValueError("%s: one of qpos, qvel and ctrl is required" % what)
        if (qpos is None) != (qvel is None):
            raise ValueError("%s: qpos and qvel are given together or not at all" % what)
        R, T = int(lead[0]), int(lead[1])
        dofs, acts = tuple(int(d) for d in dofs), tuple(int(a) for a in acts)
        nx = 2 * len(dofs)
        idx = self._index(goal_index)
        if idx is not None and idx.numel() != R:
            raise ValueError("%s: %d trajectories but %d goal indices" % (what, R, idx.numel()))

        def goal(t, width, name):
            if t is None:
                return None, None, None
            t = f32(t)
            if t.dim() == 2 and t.shape[1] == width:
                return t.reshape(t.shape[0], 1, width), 0, int(t.shape[0])
            if t.dim() == 3 and tuple(t.shape[1:]) == (T, width):
                return t, 1, int(t.shape[0])
            raise ValueError("%s: %s has shape %s, not [P, %d] or [P, %d, %d]" % (what, name, tuple(t.shape), width, T, width))
        xg, per_x, Px = goal(x_goal, nx, "x_goal")
        pg, per_p, Pp = goal(p_goal, 3, "p_goal")
        if per_x is not None and per_p is not None and (per_x != per_p or Px != Pp):
            raise ValueError("%s: x_goal %s and p_goal %s are not given the same way" % (what, tuple(xg.shape), tuple(pg.shape)))

        def weights(w, width, name):
            if w is None:
                return ()
            w = np.asarray(torch.as_tensor(w).detach().cpu().numpy() if torch.is_tensor(w) else w, np.float64)
            if w.ndim == 0:
                w = np.full(width, float(w))
            if w.shape != (width,):
                raise ValueError("%s: %s has shape %s, not [%d]" % (what, name, tuple(w.shape), width))
            return w
        options = dict(nknots=T, goal_per_knot=int(bool(per_x or per_p)), dofs=dofs, acts=acts, wx=weights(wx, nx, "wx"), wxT=weights(wx_final, nx, "wx_final"),
                       wu=weights(wu, len(acts), "wu"), wp=float(wp), wpT=float(wp_final))
        return self._cost_quad(qpos, qvel, ctrl, {"xgoal": xg, "pgoal": pg, "goal_idx": idx, "ngoals": Px if Px is not None else (Pp or 0)}, frame, R, T, want, **options)

    # ---- the iLQR / TVLQR backward pass (jaco_lqr: the whole recursion of every problem in one launch)
    def _lqr(self, opt, prob, out, n):
        """One jaco_lqr launch.  opt: the keywords of _lib.JacoLqrOptions; prob: {field of JacoLqrProblem: contiguous device tensor or
        None} plus "nprob"; out: {field of JacoLqrOut: tensor or None}, written in place."""
        o = _lib.JacoLqrOptions(**opt)
        p = _lib.JacoLqrProblem(*[_ptr(prob.get(k)) for k in ("A", "B", "lxx", "luu", "lux", "lx", "lu", "Vxx", "Vx", "mu", "prob_idx")], int(prob["nprob"]))
        r = _lib.JacoLqrOut(*[_ptr(out.get(k)) for k in ("gain", "kff", "dV", "Vxx0", "Vx0", "status")])
        self._chk(self.L.jaco_lqr(self.h, _ref(o), int(n), _ref(p), _ref(r), self._stream()))

    def lqr_backward(self, A, B, lxx, luu, lux=None, lx=None, lu=None, Vxx=None, Vx=None, mu=None, problem_index=None, rows=None, rows_out=None,
                     out=None):
        """The backward pass of iLQR / TVLQR for P problems of T knots in one launch: the feed-forward k_t and the gains K_t of
            u = u_ref + alpha k_t + K_t (x - x_ref)                       (rollout_feedback's convention)
        that minimise the quadratic model  sum_t (1/2 dx'lxx dx + 1/2 du'luu du + du'lux dx + lx'dx + lu'du) + 1/2 dx_T'Vxx dx_T + Vx'dx_T
        under  dx_{t+1} = A_t dx_t + B_t du_t  (include/jaco_env.h states the recursion).  A [P, T, nx, nx], B [P, T, nx, nu].  A cost
        array has the axes [P, T, ...]: lxx [P, T, nx, nx], luu [P, T, nu, nu], lux [P, T, nu, nx], lx [P, T, nx], lu [P, T, nu]; its
        knot axis may be left out (lxx [P, nx, nx]: the same at every knot), then its problem axis too (lxx [nx, nx]), and an
        axis of length 1 stands for all P problems or all T knots (lxx [1, T, nx, nx], lx [P, 1, nx]) -- nothing is expanded, the kernel
        reads the one copy.  lux, lx,
        lu None: zeros.  Terminal cost: Vxx [P, nx, nx] or [nx, nx] (None: lxx at the last knot), Vx [P, nx] or [nx] (None: zeros).
        Solve i works on problem problem_index[i] (None: problem i) with the regularisation mu[i] added to Quu's diagonal before it is
        factored (None: 0; one number: every solve's): n is the length of whichever of the two is given (both the same), else P -- one launch tries a ladder of
        regularisations on every problem.  rows / rows_out: control a is written to row rows[a] of rows_out rows (the motor words of the
        model's nu: the arrays are then rollout_feedback's gain / feedforward as they are); the other rows are zero.
        Returns {"gain": [n, T, rows, nx], "kff": [n, T, rows], "dV": [n, 2] -- the model's cost change of a step alpha is alpha dV[0] +
        alpha^2 dV[1] --, "Vxx0": [n, nx, nx], "Vx0": [n, nx]: the cost-to-go at knot 0, "status": [n] int32: 0, _lib.JACO_LQR_BAD_INDEX
        (problem_index out of range: nothing written), or _lib.JACO_LQR_NOT_PD | t: Quu + mu I was not positive definite (or a number
        not finite) at knot t; the rows of the knots > t are written, nothing else}.  out: a dict of tensors to write into instead of
        fresh ones (any subset of the names; a name mapped to None is not computed).  One launch on the current stream, no
        synchronisation; neither the model nor the sim's state is read."""
        dev = self.device
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
        A, B = f32(A), f32(B)
        if A.dim() != 4 or A.shape[2] != A.shape[3] or B.dim() != 4 or B.shape[:3] != A.shape[:3]:
            raise ValueError("lqr_backward: A has shape %s and B %s, not [P, T, nx, nx] and [P, T, nx, nu]" % (tuple(A.shape), tuple(B.shape)))
        P, T, nx, nu = int(A.shape[0]), int(A.shape[1]), int(A.shape[2]), int(B.shape[3])
        shared = {"knots": 0, "probs": 0}

        def cost(name, t, tail, knots=True):
            """The array as the kernel reads it, its dropped axes recorded in the two masks."""
            t = f32(t)
            if t is None:
                return None
            lead = tuple(t.shape[:t.dim() - len(tail)])
            full = (P, T) if knots else (P,)
            if tuple(t.shape[len(lead):]) != tail or len(lead) > len(full) or any(a not in (1, b) for a, b in zip(lead, full)):
                raise ValueError("lqr_backward: %s has shape %s, not %s with the leading axes %s (or fewer)" % (name, tuple(t.shape), list(tail), list(full)))
            if knots and (len(lead) < 2 or (lead[1] == 1 and T > 1)):   # (a knot axis of length 1 is one block per problem: [P, 1, ..] = [P, ..])
                shared["knots"] |= _lib.JACO_LQR_SHARED[name]
            if not lead or (lead[0] == 1 and P > 1):
                shared["probs"] |= _lib.JACO_LQR_SHARED[name]
            return t
        prob = {"A": A, "B": B, "lxx": cost("lxx", lxx, (nx, nx)), "luu": cost("luu", luu, (nu, nu)), "lux": cost("lux", lux, (nu, nx)),
                "lx": cost("lx", lx, (nx,)), "lu": cost("lu", lu, (nu,)), "nprob": P}
        if Vxx is None:   # lxx at the last knot
            l, m = prob["lxx"], _lib.JACO_LQR_SHARED["lxx"]
            Vxx = l[:, -1] if l.dim() == 4 else l
        prob["Vxx"], prob["Vx"] = cost("Vxx", Vxx, (nx, nx), knots=False), cost("Vx", Vx, (nx,), knots=False)
        idx = self._index(problem_index)
        mu = None if mu is None else f32(mu).reshape(-1)
        counts = {k: t.numel() for k, t in (("problem_index", idx), ("mu", mu)) if t is not None and not (k == "mu" and t.numel() == 1)}
        if len(set(counts.values())) > 1:
            raise ValueError("lqr_backward: %s" % " but ".join("%d entries of %s" % (c, k) for k, c in counts.items()))
        n = next(iter(counts.values())) if counts else P
        if mu is not None and mu.numel() == 1 and n != 1:   # (one mu for every solve)
            mu = mu.expand(n).contiguous()
        prob["mu"], prob["prob_idx"] = mu, idx
        if (rows is None) != (rows_out is None):
            raise ValueError("lqr_backward: rows and rows_out go together")
        R = nu if rows_out is None else int(rows_out)
        if rows is not None and len(rows) != nu:
            raise ValueError("lqr_backward: %d rows for %d controls" % (len(rows), nu))
        shapes = {"gain": (n, T, R, nx), "kff": (n, T, R), "dV": (n, 2), "Vxx0": (n, nx, nx), "Vx0": (n, nx), "status": (n,)}
        res = {}
        for k, sh in shapes.items():
            if out is not None and k in out:
                t = out[k]
                if t is not None and (tuple(t.shape) != sh or not t.is_contiguous() or t.dtype != (torch.int32 if k == "status" else torch.float32)):
                    raise ValueError("lqr_backward: out[%r] has shape %s, not a contiguous %s" % (k, tuple(t.shape), list(sh)))
                res[k] = t
            elif k == "status":
                res[k] = torch.zeros(sh, dtype=torch.int32, device=dev)
            else:   # (rows that no control maps to are never written: zeroed here once)
                res[k] = (torch.zeros if rows is not None and k in ("gain", "kff") else torch.empty)(sh, dtype=torch.float32, device=dev)
        if n > 0:
            self._lqr(dict(nknots=T, nx=nx, nu=nu, rows_out=0 if rows is None else R, rows=() if rows is None else rows,
                           shared_knots=shared["knots"], shared_probs=shared["probs"]), prob, res, n)
        return res

    def get_xyz(self, name):
        """[num_envs, 3] world position of an MJCF body (sim.data.get_body_xpos, mujoco.py:148-170)."""
        return self.query([self.frames.jaco_frame(name)], xmat=False, jac=False, qM=False, qfrc_bias=False)["xpos"][:, 0]

    def get_orientation(self, name):
        """[num_envs, 4] orientation of an MJCF body as a unit quaternion, w first (sim.data.get_body_xquat, mujoco.py:172-210)."""
        from .robot_config import mat2quat
        return mat2quat(self.query([self.frames.jaco_frame(name)], xpos=False, jac=False, qM=False, qfrc_bias=False)["xmat"][:, 0])

    def get_obj_vel(self):
        """[num_envs, 3] linear velocity of the object (qvel[9:12], what the step kernel's terminal test reads; mujoco.py:212-215)."""
        return self.get_state()[1][:, 9:12]

    def get_feedback(self, ee=None):
        """{"q": [num_envs, n_arm], "dq": [num_envs, n_arm]}: joint angles and velocities of the arm dofs (the hinge joints on the
        kinematic chain of `ee`; default "EE", on the two-arm model both arms' chains) -- mujoco.py:349-359."""
        if ee is None:
            ee = ["EE"] if "EE" in self.frames.bodies else [n for n in ("EE_1", "EE_2") if n in self.frames.bodies]
        elif isinstance(ee, str):
            ee = [ee]
        qadr, dadr = [], []
        for n in ee:
            a, d = self.frames.chain(n)
            qadr += a
            dadr += d
        qpos, qvel, _ = self.get_state()
        return {"q": qpos[:, qadr], "dq": qvel[:, dadr]}

    # ---- contact readout (jaco_set_contact_record; data.contact + mj_contactForce after mj_step)
    def record_contacts(self, capacity=16):
        """Turn the contact record on with room for `capacity` contacts per env (0: off).  From the next step call on, every
        jaco_physics_step / jaco_step writes each env's contacts of its last integrating substep and their contact-frame forces; read
        them with contacts().  Forward passes and resets write nothing (with auto_reset the record holds the terminal step's contacts)."""
        capacity = int(capacity)
        if capacity <= 0:
            self._chk(self.L.jaco_set_contact_record(self.h, None, None, 0))
            self._crec = self._cn = None
            return
        # [B][capacity] JacoContact records (CONTACT_WORDS 32-bit words each) and [B] counts; zeroed so that contacts() before the
        # first step reads "no contact"
        rec = torch.zeros(self.num_envs, capacity, _lib.CONTACT_WORDS, dtype=torch.float32, device=self.device)
        cn = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self._chk(self.L.jaco_set_contact_record(self.h, ctypes.c_void_p(rec.data_ptr()), ctypes.c_void_p(cn.data_ptr()), capacity))
        self._crec, self._cn = rec, cn   # (kept alive here: the library only holds the pointers)
        if getattr(self, "_gmap", None) is None:
            self.contact_names = ContactNames.for_model(self.robot_file)
            self._gmap = torch.tensor(self.contact_names.kernel_geom, dtype=torch.int64, device=self.device)

    def contacts(self):
        """The record of the last step call as device tensors (copies; no host synchronisation).  B envs, K = capacity:
        ncon [B] int32, the TRUE contact count (> K: records past K were dropped);  valid [B, K] bool (slot < min(ncon, K));
        dist [B, K];  pos [B, K, 3];  frame [B, K, 3, 3] (row 0 = normal, from geom 1 towards geom 2);  force [B, K, 6] in the contact
        frame (mj_contactForce: normal, two tangential, torsional, two rolling);  dim [B, K] int32;  geom [B, K, 2] / body [B, K, 2]
        MJCF geom / body ids (-1 in invalid slots).  Invalid slots are zero."""
        if getattr(self, "_crec", None) is None:
            raise JacoError("contacts(): call record_contacts(capacity) first")
        return Contacts(self._crec, self._cn, self._gmap)

    def net_contact_force(self, body_a, body_b, contacts=None):
        """[num_envs, 3] world-frame force that MJCF body `body_a` exerts on `body_b` (names or ids), summed over their recorded contacts
        (those past the capacity are not in the record).  Computed in torch from contacts() (or the `contacts` given)."""
        return (contacts if contacts is not None else self.contacts()).net_force(self._body(body_a), self._body(body_b))

    def _body(self, b):
        if isinstance(b, str):
            if getattr(self, "contact_names", None) is None:
                self.contact_names = ContactNames.for_model(self.robot_file)
            return self.contact_names.body_id(b)
        return int(b)

    def sensordata(self):
        out = torch.empty(self.num_envs, self.nsensor, device=self.device)
        self._chk(self.L.jaco_get_sensordata(self.h, self._dev(out, self.nsensor), self._stream()))
        return out

    def flags(self):
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._chk(self.L.jaco_get_flags(self.h, self._dev(out, 1, torch.int32), self._stream()))
        return out

    def clear_flags(self):
        self._chk(self.L.jaco_clear_flags(self.h, self._stream()))

    def stats(self):
        out = torch.empty(self.num_envs, 4, dtype=torch.int32, device=self.device)
        self._chk(self.L.jaco_get_stats(self.h, self._dev(out, 4, torch.int32), self._stream()))
        return out

    def set_option(self, name, value):
        self._chk(self.L.jaco_set_option(self.h, name.encode(), float(value)))

    def launch_count(self):
        """Kernel launches issued for this handle since the previous call (host-side counter)."""
        return int(self.L.jaco_launch_count(self.h))

    def enable_timing(self, on=True):
        self._chk(self.L.jaco_enable_timing(self.h, int(on)))

    def step_time_ms(self):
        """Mean device time of a whole step launch set in the timing window (call before kernel_time_ms, which closes it)."""
        ms = ctypes.c_double()
        self._chk(self.L.jaco_step_time_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def kernel_time_ms(self):
        ms, n = ctypes.c_double(), ctypes.c_int()
        self._chk(self.L.jaco_kernel_time_ms(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
