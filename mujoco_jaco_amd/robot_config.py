"""Robot-configuration queries: the `MujocoConfig` half of the reference, batched.

Mirrors /root/reference/env_script/mujoco_config.py:201-447 (J, M, g, R, quaternion, Tx) and the body-pose getters of mujoco.py:148-215
for `num_envs` environments.  Every number comes from one jaco_query launch (include/jaco_env.h; kernel mujoco_jaco_amd/csrc/query.h):
the values of a sim.forward() on the current (or a given) state.

FrameTable maps MJCF body names (assets/<model>.names.txt) to the frames the kernel takes: a body welded to a moving body becomes that
weld root's fused index plus its constant pose in the root's frame (the pose compile.fuse uses, modelc.kin.rel_pose); a body welded to
the world becomes a world-fixed frame.  The default Jacobian reference point is the body's own centre of mass (body_ipos): mj_jacBodyCom.
"""
import numpy as np

from . import _lib
from .modelc import blob as blobmod
from .modelc import kin


def read_names(path):
    """{kind: [name or None]} of a shipped assets/<model>.names.txt (MJCF order; "-" = unnamed)."""
    out = {}
    for line in open(path):
        if ":" in line:
            k, v = line.split(":", 1)
            out[k.strip()] = [None if n == "-" else n for n in v.split()]
    return out


def quat2mat32(q):
    """Row-major fp32 rotation of a unit quaternion, rounded exactly as the library's model loader rounds its frames (model_blob.cpp)."""
    w, x, y, z = (float(c) for c in q)
    return np.array([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], np.float64).astype(np.float32)


class FrameTable:
    """MJCF body name -> kernel frame (fused body, pose in it), built from the model blob and its names file."""

    def __init__(self, M, names):
        self.M, self.names = M, names
        self.bodies = names["body"]
        nbody = int(M["nbody"][0])
        self.weld = M["body_weldid"]
        self.xpos0, self.xquat0, _, _ = kin.fk(M, M["qpos0"])
        self.fid = {0: -1}
        for i, r in enumerate([b for b in range(1, nbody) if self.weld[b] == b]):
            self.fid[r] = i
        self._motor = None

    @classmethod
    def for_model(cls, robot_file):
        path = _lib.model_path(robot_file)
        return cls(blobmod.load(path), read_names(path[:-len(".jacomdl")] + ".names.txt"))

    def body_id(self, name):
        if name not in self.bodies:
            raise ValueError("unknown body %r: the model's bodies are %s" % (name, [n for n in self.bodies if n]))
        b = self.bodies.index(name)
        if self.M["body_mocapid"][b] >= 0:
            raise ValueError("body %r is a mocap body (a task-layer marker): its pose is not a function of the state; read it with env.markers()" % name)
        return b

    def frame(self, name):
        """(fused body or -1, position, unit quaternion) of the body in that fused body's frame (fp64), as compile.fuse computes it."""
        b = self.body_id(name)
        w = self.weld[b]
        if w == 0:
            return -1, np.array(self.xpos0[b], np.float64), np.array(self.xquat0[b], np.float64)
        p, q = kin.rel_pose(self.xpos0, self.xquat0, b, w)
        return self.fid[w], np.asarray(p, np.float64), np.asarray(q, np.float64)

    def com(self, name):
        """The body's centre of mass in its own frame (body_ipos): mj_jacBodyCom's point."""
        return np.asarray(self.M["body_ipos"].reshape(-1, 3)[self.body_id(name)], np.float64)

    def jaco_frame(self, name, point=None):
        """The kernel's frame record (_lib.JacoFrame) of a body; point: Jacobian reference point in the body's frame (default: its COM)."""
        fb, p, q = self.frame(name)
        f = _lib.JacoFrame()
        f.body = fb
        f.pos[:] = [float(v) for v in np.asarray(p, np.float64).astype(np.float32)]
        f.mat[:] = [float(v) for v in quat2mat32(q)]
        f.point[:] = [float(v) for v in np.asarray(self.com(name) if point is None else point, np.float64).astype(np.float32)]
        return f

    def chain(self, name):
        """(qpos addresses, dof addresses) of the joints on the kinematic chain from the world to body `name`, root first
        (get_joints_in_ee_kinematic_tree, mujoco.py:115-146).  Hinge joints only: they are what `q` can be spliced into."""
        b = self.body_id(name)
        joints = []
        while b > 0:
            ja, jn = int(self.M["body_jntadr"][b]), int(self.M["body_jntnum"][b])
            joints = list(range(ja, ja + jn)) + joints
            b = int(self.M["body_parentid"][b])
        for j in joints:
            if self.M["jnt_type"][j] != kin.JNT_HINGE:
                raise ValueError("body %r hangs from a free joint: it has no arm chain of hinge joints" % name)
        return [int(self.M["jnt_qposadr"][j]) for j in joints], [int(self.M["jnt_dofadr"][j]) for j in joints]

    def hinge_joints(self, joints):
        """Joint ids of the MJCF joint names `joints` (one name or a list of them), in the order given: each a hinge joint of the
        model, none listed twice."""
        M, names = self.M, self.names["joint"]
        ids = []
        for n in ([joints] if isinstance(joints, str) else joints):
            if n is None or n not in names:
                raise ValueError("unknown joint %r: the model's joints are %s" % (n, [x for x in names if x]))
            j = names.index(n)
            if M["jnt_type"][j] != kin.JNT_HINGE:
                raise ValueError("joint %r is not a hinge joint" % n)
            if j in ids:
                raise ValueError("joint %r is listed twice" % n)
            ids.append(j)
        return ids

    def motor_of_dof(self):
        """{dof: index of its motor actuator} (the blob's fused actuator table; position servos are left out), built once."""
        if self._motor is None:
            M = self.M
            self._motor = {int(M["jnt_dofadr"][int(j)]): a for a, (j, pos) in enumerate(zip(M["actuator_jntid"], M["actuator_position"])) if not pos}
        return self._motor


class ContactNames:
    """MJCF geom / body names <-> the ids of the contact record (BatchedMujoco.contacts): geoms and bodies are reported as MJCF ids
    (assets/<model>.names.txt order).  The kernel's geom ids, which the library writes, map to MJCF ids through the blob's f_geom_orig
    (`kernel_geom`); bodies are the original (unfused) MJCF bodies already."""

    def __init__(self, M, names):
        self.M, self.names = M, names
        self.bodies, self.geoms = names["body"], names["geom"]
        self.kernel_geom = np.asarray(M["f_geom_orig"], np.int64)   # kernel geom id -> MJCF geom id

    @classmethod
    def for_model(cls, robot_file):
        path = _lib.model_path(robot_file)
        return cls(blobmod.load(path), read_names(path[:-len(".jacomdl")] + ".names.txt"))

    def body_id(self, name):
        if name not in self.bodies:
            raise ValueError("unknown body %r: the model's bodies are %s" % (name, [n for n in self.bodies if n]))
        return self.bodies.index(name)

    def geom_id(self, name):
        if name not in self.geoms:
            raise ValueError("unknown geom %r: the model's named geoms are %s" % (name, [n for n in self.geoms if n]))
        return self.geoms.index(name)

    def body_name(self, i):
        return self.bodies[int(i)] if 0 <= int(i) < len(self.bodies) else None

    def geom_name(self, i):
        return self.geoms[int(i)] if 0 <= int(i) < len(self.geoms) else None

    def geom_body(self, i):
        """MJCF body id of MJCF geom i."""
        return int(self.M["geom_bodyid"][int(i)])


def mat2quat(R):
    """[..., 9] row-major rotations -> [..., 4] unit quaternions, w first, w >= 0 (mju_mat2Quat's branches)."""
    import torch
    m = R.reshape(*R.shape[:-1], 3, 3)
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    tr = m00 + m11 + m22
    c0 = torch.stack([1 + tr, m21 - m12, m02 - m20, m10 - m01], -1)
    c1 = torch.stack([m21 - m12, 1 + m00 - m11 - m22, m01 + m10, m02 + m20], -1)
    c2 = torch.stack([m02 - m20, m01 + m10, 1 - m00 + m11 - m22, m12 + m21], -1)
    c3 = torch.stack([m10 - m01, m02 + m20, m12 + m21, 1 - m00 - m11 + m22], -1)
    pick = torch.stack([tr, m00, m11, m22], -1).argmax(-1)
    q = torch.where((pick == 0)[..., None], c0, torch.where((pick == 1)[..., None], c1, torch.where((pick == 2)[..., None], c2, c3)))
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[..., :1] < 0, -q, q)


def splice(sim, qadr, dadr, q, dq):
    """(qpos, qvel) rows for the sim: copies of its current state with q [num_envs, len(qadr)] written at the qpos addresses qadr and dq
    [num_envs, len(dadr)] at the dof addresses dadr (each may be None: left as it is); (None, None), the current state itself, when both
    are None."""
    if q is None and dq is None:
        return None, None
    import torch
    qpos, qvel, _ = sim.get_state()
    if q is not None:
        qpos[:, qadr] = torch.as_tensor(q, dtype=qpos.dtype, device=qpos.device).reshape(qpos.shape[0], len(qadr))
    if dq is not None:
        qvel[:, dadr] = torch.as_tensor(dq, dtype=qvel.dtype, device=qvel.device).reshape(qvel.shape[0], len(dadr))
    return qpos.contiguous(), qvel.contiguous()


class BatchedMujocoConfig:
    """MujocoConfig (mujoco_config.py:201-447) over a BatchedMujoco: J, M, g, R, quaternion, Tx for every env at once.

    `arm` = the dofs of the hinge joints on the kinematic chain of `ee` (get_joints_in_ee_kinematic_tree, mujoco.py:115-146): dofs 0-5 on
    the single-arm models, one arm's six on the two-arm model (ee = "EE_1" / "EE_2").  Accessors return [num_envs, ...] tensors on the
    sim's device restricted to the arm (full=True: all nv dofs).  q: [num_envs, n_arm] joint angles spliced into the current qpos (the
    current qvel stays); q=None: the current state.  One query launch fills every output for the registered frames (at most 16 body
    names, registered on first use); accessors reuse that result until the sim's state changes (BatchedMujoco.state_version).
    """

    def __init__(self, sim, ee="EE"):
        self.sim = sim
        self.table = sim.frames
        self.ee = ee
        self.arm_qadr, self.arm = self.table.chain(ee)
        self.n_arm = len(self.arm)
        self._names, self._frames = [], []
        self._cache, self._cache_key = None, None
        self._word_index = {}   # (_words: index lists as device tensors)
        self._register(ee)

    def _register(self, name):
        if name in self._names:
            return self._names.index(name)
        if len(self._names) >= _lib.JACO_QUERY_MAX_FRAMES:
            raise ValueError("at most %d frames per BatchedMujocoConfig (registered: %s)" % (_lib.JACO_QUERY_MAX_FRAMES, self._names))
        f = self.table.jaco_frame(name)   # (raises ValueError for unknown and mocap bodies)
        self._names.append(name)
        self._frames.append(f)
        self._cache = None
        return len(self._names) - 1

    def _result(self, q):
        if q is None:
            key = self.sim.state_version
            if self._cache is None or self._cache_key != key:
                self._cache = self.sim.query(self._frames)
                self._cache_key = key
            return self._cache
        return self.sim.query(self._frames, qpos=self._spliced(q, None)[0])

    def _cols(self, t, full):
        return t if full else t[..., self.arm]

    def J(self, name, q=None, full=False):
        """[num_envs, 6, n_arm]: translational rows 0-2, rotational rows 3-5 at the body's COM (mj_jacBodyCom)."""
        i = self._register(name)
        return self._cols(self._result(q)["jac"][:, i], full)

    def M(self, q=None, full=False):
        """[num_envs, n_arm, n_arm] joint-space inertia (mj_fullM)."""
        qM = self._result(q)["qM"]
        return qM if full else qM[:, self.arm][:, :, self.arm]

    def g(self, q=None, full=False):
        """[num_envs, n_arm]: -qfrc_bias (gravity, Coriolis and centrifugal forces at the current qvel)."""
        return -self._cols(self._result(q)["qfrc_bias"], full)

    def R(self, name, q=None):
        """[num_envs, 3, 3] body rotation (xmat)."""
        i = self._register(name)
        return self._result(q)["xmat"][:, i].reshape(-1, 3, 3)

    def quaternion(self, name, q=None):
        """[num_envs, 4] body orientation, w first."""
        i = self._register(name)
        return mat2quat(self._result(q)["xmat"][:, i])

    def ik(self, name, pos, quat=None, q=None, x=None, **options):
        """([num_envs, n_arm] arm angles, [num_envs] converged): the configuration that puts the point x (3-vector in the body frame,
        default the body origin) of body `name` at pos [num_envs, 3] -- Tx(name, q=result, x=x) ~ pos -- and, with quat [num_envs, 4]
        (w first), the body at that orientation.  Seed: q ([num_envs, n_arm] arm angles spliced into the current qpos, as every
        accessor's q), default the current state.  options: tol_pos, tol_rot, damping, max_step, max_iters, dof_mask (BatchedMujoco.ik).
        One jaco_ik launch; the sim's state is not touched."""
        seed = self._spliced(q, None)[0]
        frame = self.table.jaco_frame(name, point=np.zeros(3) if x is None else np.asarray(x, np.float64).reshape(3))
        r = self.sim.ik(frame, pos, quat, seed, **options)
        return r["qpos"][:, self.arm_qadr], r["converged"]

    def osc(self, names=None, **gains):
        """BatchedOSC over this sim: abr_control's OSC(robot_config, kp, ko, kv, vmax); names default to this config's end effector."""
        return BatchedOSC(self, names=(self.ee,) if names is None else names, **gains)

    def joint(self, kp=50.0, kv=20.0, vmax=None, joints=None):
        """BatchedJoint over this sim: abr_control's Joint(robot_config, kp, kv); joints default to every motor-driven hinge joint."""
        return BatchedJoint(self, kp=kp, kv=kv, vmax=vmax, joints=joints)

    def _spliced(self, q, dq):
        """(qpos, qvel) rows for the sim: None where the current state is meant, else q / dq [num_envs, n_arm] spliced into it."""
        return splice(self.sim, self.arm_qadr, self.arm, q, dq)

    def forward_dynamics(self, ctrl=None, q=None, dq=None, implicit_damping=False, full=False):
        """[num_envs, n_arm] joint accelerations that ctrl [num_envs, nu] (None: zeros) produces (full=True: all nv dofs): mj_forward's
        qacc_smooth, contact-free (BatchedMujoco.forward_dynamics).  q / dq: arm angles / velocities spliced into the current state."""
        qpos, qvel = self._spliced(q, dq)
        return self._cols(self.sim.forward_dynamics(ctrl, qpos, qvel, implicit_damping=implicit_damping), full)

    def _joint_subset(self, joints, what):
        """(dofs, qpos addresses, motor actuators) of the hinge joints `joints` (MJCF names; default: this config's arm), the actuators in
        the joints' order -- the x = [q_J, dq_J] and u of linearize and rollout_feedback."""
        M = self.table.M
        if joints is None:
            dofs, qadr = list(self.arm), list(self.arm_qadr)
        else:
            ids = self.table.hinge_joints(joints)
            dofs, qadr = [int(M["jnt_dofadr"][j]) for j in ids], [int(M["jnt_qposadr"][j]) for j in ids]
        if not dofs:
            raise ValueError("%s: no joint chosen" % what)
        motor = self.table.motor_of_dof()
        return dofs, qadr, [motor[d] for d in dofs if d in motor]

    def linearize(self, joints=None, ctrl=None, q=None, dq=None, **steps):
        """(A [num_envs, 2 n, 2 n], B [num_envs, 2 n, m], c [num_envs, 2 n]) of the discrete contact-free transition of one substep on
        the hinge joints `joints` (MJCF names; default: this config's arm), around the current state (or q / dq spliced into it) and
        ctrl [num_envs, nu] (None: zeros):  x' ~ A x + B u + c  with the state x = [q_J, dq_J], u the ctrl words of the motor actuators
        of those joints (in the joints' order; B.shape[-1] of them), and the integrator's order: dq' = dq + h qacc, q' = q + h dq'
        (h the model's timestep, qacc with the implicit joint damping of the step).  The other dofs and ctrl words are held at their
        values.  One jaco_fd launch (BatchedMujoco.linearize) plus the assembly in torch; steps: eps_qpos, eps_qvel."""
        import torch
        M = self.table.M
        dofs, qadr, acts = self._joint_subset(joints, "linearize")
        h = float(M["opt_timestep"][0])
        qpos, qvel = self._spliced(q, dq)
        r = self.sim.linearize(ctrl, qpos, qvel, dofs=dofs, implicit_damping=True, **steps)
        if qpos is None:
            qpos, qvel, _ = self.sim.get_state()
        n, B = len(dofs), qpos.shape[0]
        a = r["qacc"][:, dofs]
        Aq, Av, Bu = r["dq"][:, dofs][:, :, dofs], r["dv"][:, dofs][:, :, dofs], r["du"][:, dofs][:, :, acts]
        I = torch.eye(n, dtype=a.dtype, device=a.device).expand(B, n, n)
        Fv = I + h * Av                      # d dq' / d dq
        A = torch.cat([torch.cat([I + h * h * Aq, h * Fv], 2), torch.cat([h * Aq, Fv], 2)], 1)
        Bm = torch.cat([h * h * Bu, h * Bu], 1)
        x = torch.cat([qpos[:, qadr], qvel[:, dofs]], 1)
        u = torch.zeros(B, len(acts), dtype=a.dtype, device=a.device) if ctrl is None else \
            torch.as_tensor(ctrl, dtype=a.dtype, device=a.device).reshape(B, -1)[:, acts]
        v1 = x[:, n:] + h * a
        x1 = torch.cat([x[:, :n] + h * v1, v1], 1)
        c = x1 - (A @ x[:, :, None])[:, :, 0] - (Bm @ u[:, :, None])[:, :, 0]
        return A, Bm, c

    def rollout(self, ctrl, hold=1, q=None, dq=None, final_only=False):
        """Open-loop prediction of this config's arm and end effector: ctrl [num_envs, T, nu] (one sequence per env) or [num_envs, K, T,
        nu] (K candidate sequences per env, all started from that env's state through a state index -- the states are not copied), each
        row held for `hold` substeps, from the current state (or q / dq, arm angles / velocities spliced into it).  Contact-free, with
        joint limits (BatchedMujoco.rollout).  {"q": [num_envs, K, T, n_arm], "dq": likewise, "ee_pos": [num_envs, K, T, 3], "ee_mat":
        [num_envs, K, T, 9]: the arm's joints and the pose of `ee` after each knot; "status": [num_envs, K]}; without K the K axis is
        squeezed; final_only=True: T = 1, the last knot.  One jaco_rollout launch; the sim's state is not touched."""
        import torch
        B = self.sim.num_envs
        ctrl = torch.as_tensor(ctrl, dtype=torch.float32, device=self.sim.device)
        if ctrl.dim() not in (3, 4) or ctrl.shape[0] != B:
            raise ValueError("rollout: ctrl has shape %s, not [%d, T, nu] or [%d, K, T, nu]" % (tuple(ctrl.shape), B, B))
        squeeze = ctrl.dim() == 3
        K, T = (1 if squeeze else ctrl.shape[1]), ctrl.shape[-2]
        qpos, qvel = self._spliced(q, dq)
        index = torch.arange(B, dtype=torch.int32, device=ctrl.device).repeat_interleave(K)
        r = self.sim.rollout(ctrl.reshape(B * K, T, ctrl.shape[-1]), qpos, qvel, state_index=index, hold=hold, frame=self._frames[0], final_only=final_only)
        rows = 1 if final_only else T
        out = {"q": r["qpos"][..., self.arm_qadr], "dq": r["qvel"][..., self.arm], "ee_pos": r["xpos"], "ee_mat": r["xmat"]}
        out = {k: t.reshape(B, K, rows, t.shape[-1]) for k, t in out.items()}
        out["status"] = r["status"].reshape(B, K)
        return {k: t[:, 0] for k, t in out.items()} if squeeze else out

    def rollout_feedback(self, u, K=None, x_ref=None, k=None, alphas=None, joints=None, ctrl=None, hold=1, per_substep=False, q=None, dq=None,
                         final_only=False):
        """Closed-loop prediction on the joints and actuators that linearize(joints=...) uses: x = [q_J, dq_J], u the motor words of
        those joints in the same order (m of them).  Env b follows its plan  u_t = u[b, t] + alpha k[b, t] + K[b, t] (x_t - x_ref[b, t])
        -- u [B, T, m], K [B, T, m, 2 n] with x_ref [B, T, 2 n] (lqr_gains' sign convention), k [B, T, m]; K and k may be None -- from the
        current state (or q / dq, arm angles / velocities spliced into it); the law is evaluated inside the kernel at the start of each
        knot and held for `hold` substeps (per_substep=True: before every substep).  The other ctrl words are those of ctrl [B, nu]
        (None: zeros), held over the horizon.  alphas [A]: every env runs its plan once per step size -- iLQR's line search; the A
        rollouts of an env share its plan and its state through indices, nothing is copied.
        {"q": [B, A, T, n_arm], "dq": likewise, "ee_pos": [B, A, T, 3], "ee_mat": [B, A, T, 9]: as rollout(); "u": [B, A, E, m]: the
        applied motor words of every evaluation as commanded (E = T, or T * hold with per_substep; all of them also with final_only);
        "status": [B, A]}; without alphas the A axis is squeezed.  One jaco_rollout_fb launch (BatchedMujoco.rollout_feedback); the
        sim's state is not touched."""
        import torch
        B, dev, nu = self.sim.num_envs, self.sim.device, self.sim.nu
        dofs, qadr, acts = self._joint_subset(joints, "rollout_feedback")
        n, m = len(dofs), len(acts)
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)
        u, K, x_ref, k = f32(u), f32(K), f32(x_ref), f32(k)
        if u.dim() != 3 or u.shape[0] != B or u.shape[2] != m:
            raise ValueError("rollout_feedback: u has shape %s, not [%d, T, %d]" % (tuple(u.shape), B, m))
        T = int(u.shape[1])
        if k is not None and k.shape != u.shape:
            raise ValueError("rollout_feedback: k has shape %s, not u's %s" % (tuple(k.shape), tuple(u.shape)))
        if K is not None:
            if K.shape != (B, T, m, 2 * n):
                raise ValueError("rollout_feedback: K has shape %s, not [%d, %d, %d, %d]" % (tuple(K.shape), B, T, m, 2 * n))
            if x_ref is None or x_ref.shape != (B, T, 2 * n):
                raise ValueError("rollout_feedback: x_ref has shape %s, not [%d, %d, %d]" % (None if x_ref is None else tuple(x_ref.shape), B, T, 2 * n))
        if alphas is not None and k is None:
            raise ValueError("rollout_feedback: alphas need k")
        base = torch.zeros(B, nu, dtype=torch.float32, device=dev) if ctrl is None else f32(ctrl).reshape(B, nu)
        full = base[:, None, :].repeat(1, T, 1)
        full[:, :, acts] = u
        kff = gain = None
        if k is not None:
            kff = torch.zeros_like(full)
            kff[:, :, acts] = k
        if K is not None:
            gain = torch.zeros(B, T, nu, 2 * n, dtype=torch.float32, device=dev)
            gain[:, :, acts] = K
        index = alpha = None
        A = 1
        if alphas is not None:
            alphas = f32(alphas).reshape(-1)
            A = int(alphas.numel())
            index = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(A)
            alpha = alphas.repeat(B)
        qpos, qvel = self._spliced(q, dq)
        r = self.sim.rollout_feedback(full, qpos, qvel, gain=gain, x_ref=x_ref, dofs=dofs, feedforward=kff, alpha=alpha, plan_index=index, state_index=index,
                                      hold=hold, per_substep=per_substep, frame=self._frames[0], final_only=final_only)
        out = {"q": r["qpos"][..., self.arm_qadr], "dq": r["qvel"][..., self.arm], "ee_pos": r["xpos"], "ee_mat": r["xmat"], "u": r["ctrl"][..., acts]}
        out = {key: t.reshape(B, A, t.shape[-2], t.shape[-1]) for key, t in out.items()}
        out["status"] = r["status"].reshape(B, A)
        return {key: t[:, 0] for key, t in out.items()} if alphas is None else out

    def linearize_rollout(self, u, K=None, x_ref=None, k=None, alpha=None, joints=None, ctrl=None, q=None, dq=None, hold=1, **steps):
        """The trajectory of rollout_feedback's plan and the transition Jacobians of every knot of it, of the very step the rollouts
        simulate (`hold` substeps, joint-limit rows included) -- what one iLQR iteration linearises: the arguments are rollout_feedback's
        (alpha: one step size, a scalar or [B]; needs k), on the joints and motor words linearize(joints=...) uses.
        (A [B, T, 2 n, 2 n], Bm [B, T, 2 n, m], x [B, T + 1, 2 n], u_applied [B, T, m], status [B]):  x_(t+1) ~ x_(t+1) + A_t dx_t + Bm_t du_t
        about the trajectory x (x[:, 0] the start) under the applied motor words u_applied; A and Bm go straight into ilqr_backward, x and
        u_applied into rollout_feedback(..., alphas=) as x_ref and u.  Two launches on this handle: one rollout_feedback for the full state
        and applied ctrl of every knot, one transition_fd over the B * T (state at the start of knot t, applied ctrl of knot t) pairs;
        steps: eps_qpos, eps_qvel, eps_ctrl, centered, groups.  The sim's state is not touched."""
        p = self._closed_loop("linearize_rollout", u, K, x_ref, k, alpha, joints, ctrl, q, dq, hold)
        return self._linearized(p, hold, steps)

    def _words(self, words):
        """A list of dofs, addresses or ctrl words as an index tensor on the sim's device, uploaded once per list: indexing with it
        enqueues a gather / scatter, where a Python list is uploaded, synchronously, at every use."""
        import torch
        key = tuple(int(w) for w in words)
        cache = self._word_index
        if key not in cache:
            cache[key] = torch.tensor(key, dtype=torch.long, device=self.sim.device)
        return cache[key]

    def _closed_loop(self, what, u, K, x_ref, k, alpha, joints, ctrl, q, dq, hold):
        """What linearize_rollout, ilqr_expand and ilqr's last evaluation share: one rollout_feedback launch of every env's plan (alpha: one
        step size per env) on the joints' dofs and motor words.  {"r": sim.rollout_feedback's dict, "Q" [B, T + 1, nq], "V" [B, T + 1, nv]:
        the full state at the start of every knot and at the end, "x" [B, T + 1, 2 n], "u" [B, T, m]: the applied motor words, "dofs",
        "qadr", "acts", "T"}."""
        import torch
        sim = self.sim
        B, dev, nu = sim.num_envs, sim.device, sim.nu
        dofs, qadr, acts = self._joint_subset(joints, what)
        n, m = len(dofs), len(acts)
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)
        u, K, x_ref, k = f32(u), f32(K), f32(x_ref), f32(k)
        if u.dim() != 3 or u.shape[0] != B or u.shape[2] != m:
            raise ValueError("%s: u has shape %s, not [%d, T, %d]" % (what, tuple(u.shape), B, m))
        T = int(u.shape[1])
        if alpha is not None and k is None:
            raise ValueError("%s: alpha needs k" % what)
        at = self._words(acts)
        base = torch.zeros(B, nu, dtype=torch.float32, device=dev) if ctrl is None else f32(ctrl).reshape(B, nu)
        full = base[:, None, :].repeat(1, T, 1)
        full[:, :, at] = u
        kff = gain = None
        if k is not None:
            kff = torch.zeros_like(full)
            kff[:, :, at] = k
        if K is not None:
            gain = torch.zeros(B, T, nu, 2 * n, dtype=torch.float32, device=dev)
            gain[:, :, at] = K
        if alpha is not None:
            alpha = f32(alpha).reshape(-1).expand(B).contiguous()
        qpos, qvel = self._spliced(q, dq)
        r = sim.rollout_feedback(full, qpos, qvel, gain=gain, x_ref=x_ref, dofs=dofs, feedforward=kff, alpha=alpha, hold=hold)
        if qpos is None:
            qpos, qvel, _ = sim.get_state()
        Q, V = torch.cat([qpos[:, None], r["qpos"]], 1), torch.cat([qvel[:, None], r["qvel"]], 1)   # [B, T + 1, ..]: the state at the start of every knot, and the end
        return dict(r=r, Q=Q, V=V, x=torch.cat([Q[..., self._words(qadr)], V[..., self._words(dofs)]], 2), u=r["ctrl"][..., at], dofs=dofs, qadr=qadr, acts=acts, T=T)

    def _linearized(self, p, hold, steps):
        """linearize_rollout's five results from _closed_loop's: the one transition_fd launch over the B * T (state at the start of knot t,
        applied ctrl of knot t) pairs."""
        import torch
        sim, T, dofs, acts = self.sim, p["T"], p["dofs"], p["acts"]
        r, Q, V = p["r"], p["Q"], p["V"]
        lin = sim.transition_fd(r["ctrl"], Q[:, :T].contiguous(), V[:, :T].contiguous(), dofs=dofs, acts=acts, hold=hold, want=("A", "B") if acts else ("A",), **steps)
        Bm = lin["B"] if acts else torch.zeros(sim.num_envs, T, 2 * len(dofs), 0, dtype=torch.float32, device=sim.device)   # (no motor on the chosen joints: as linearize, no column)
        return lin["A"], Bm, p["x"], p["u"], r["status"]

    def _cost_arguments(self, what, n, m, T, q_goal, dq_goal, ee_goal, w_q, w_dq, w_ee, w_u, w_q_final, w_dq_final, w_ee_final):
        """The goals and weights of rollout_cost, ilqr_expand and ilqr, checked and put into the sim tier's form: {"x_goal": [B, 2 n] or
        [B, T, 2 n] or None (no state weight), "p_goal", "wx", "wxT" [2 n], "wu" [m] fp64 arrays, "wp", "wpT"}."""
        import torch
        B, dev = self.sim.num_envs, self.sim.device
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)
        # the goals: x_goal = [q_goal, dq_goal], per env or per env and knot
        goals = {name: f32(t) for name, t in (("q_goal", q_goal), ("dq_goal", dq_goal), ("ee_goal", ee_goal)) if t is not None}
        for name, t in goals.items():
            width = 3 if name == "ee_goal" else n
            if tuple(t.shape) not in ((B, width), (B, T, width)):
                raise ValueError("%s: %s has shape %s, not [%d, %d] or [%d, %d, %d]" % (what, name, tuple(t.shape), B, width, B, T, width))
        if len({t.dim() for t in goals.values()}) > 1:
            raise ValueError("%s: the goals (%s) are given all per env or all per env and knot" % (what, ", ".join(goals)))
        x_goal = None
        if "q_goal" in goals or "dq_goal" in goals:
            like = goals.get("q_goal", goals.get("dq_goal"))
            x_goal = torch.cat([goals.get("q_goal", torch.zeros_like(like)), goals.get("dq_goal", torch.zeros_like(like))], -1)

        def vec(w, width, name):
            w = np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, np.float64)
            if w.ndim == 0:
                return np.full(width, float(w))
            if w.shape != (width,):
                raise ValueError("%s: %s has shape %s, not [%d]" % (what, name, tuple(w.shape), width))
            return w
        on = lambda name, w: vec(w, n, name) * (name.split("_")[1] + "_goal" in goals)   # (a goal that is not given weighs nothing)
        last = lambda w, running: running if w is None else w
        wx = np.concatenate([on("w_q", w_q), on("w_dq", w_dq)])
        wxT = np.concatenate([on("w_q_final", last(w_q_final, w_q)), on("w_dq_final", last(w_dq_final, w_dq))])
        pose = "ee_goal" in goals
        return dict(x_goal=x_goal if wx.any() or wxT.any() else None, p_goal=goals.get("ee_goal"), wx=wx, wxT=wxT, wu=vec(w_u, m, "w_u"),
                    wp=float(w_ee) * pose, wpT=float(last(w_ee_final, w_ee)) * pose)

    def ilqr_expand(self, u, K=None, x_ref=None, k=None, alpha=None, joints=None, ctrl=None, q=None, dq=None, hold=1, q_goal=None, dq_goal=None,
                    ee_goal=None, w_q=0.0, w_dq=0.0, w_ee=0.0, w_u=0.0, w_q_final=None, w_dq_final=None, w_ee_final=None, **steps):
        """Everything iLQR's backward pass reads, about the trajectory of rollout_feedback's plan: linearize_rollout's five results and the
        quadratic expansion of rollout_cost's cost (its goals, weights and conventions) along that trajectory.  {"A" [B, T, 2 n, 2 n], "B"
        [B, T, 2 n, m], "x" [B, T + 1, 2 n], "u" [B, T, m], "status" [B]: linearize_rollout's, bit for bit;  "lx" [B, T, 2 n], "lxx" [B, T,
        2 n, 2 n], "lu" [B, T, m], "luu" [m, m] = diag(w_u), "Vx" [B, 2 n], "Vxx" [B, 2 n, 2 n]: ilqr_backward's arguments as they are (the
        start state is not costed: row 0 of lx / lxx is zero; the pose term in Gauss-Newton form);  "l" [B, T]: knot t's own summand of
        rollout_cost's cost}.  Three launches on this handle: rollout_feedback, transition_fd, cost_quad (BatchedMujoco.cost_quad); steps:
        linearize_rollout's.  The sim's state is not touched."""
        import torch
        p = self._closed_loop("ilqr_expand", u, K, x_ref, k, alpha, joints, ctrl, q, dq, hold)
        n, m, T = len(p["dofs"]), len(p["acts"]), p["T"]
        c = self._cost_arguments("ilqr_expand", n, m, T, q_goal, dq_goal, ee_goal, w_q, w_dq, w_ee, w_u, w_q_final, w_dq_final, w_ee_final)
        A, Bm, x, ua, status = self._linearized(p, hold, steps)
        r = p["r"]
        e = self.sim.cost_quad(r["qpos"], r["qvel"], r["ctrl"], dofs=p["dofs"], acts=p["acts"], frame=self._frames[0], x_goal=c["x_goal"], p_goal=c["p_goal"],
                               wx=c["wx"], wx_final=c["wxT"], wu=c["wu"], wp=c["wp"], wp_final=c["wpT"],
                               want=("lx", "lxx", "Vx", "Vxx", "l") + (("lu",) if m else ()))
        if not m:
            e["lu"] = torch.zeros(x.shape[0], T, 0, dtype=torch.float32, device=x.device)
        return dict(A=A, B=Bm, x=x, u=ua, status=status, luu=torch.diag(self._filled(c["wu"])), **e)

    def _filled(self, values):
        """The numbers `values` as an fp32 vector on the sim's device, built there by fills: nothing is uploaded, so nothing synchronises."""
        import torch
        dev = self.sim.device
        return torch.cat([torch.full((1,), float(x), dtype=torch.float32, device=dev) for x in values]) if len(values) else torch.zeros(0, dtype=torch.float32, device=dev)

    ILQR_ALPHAS = (0.0,) + tuple(2.0 ** -i for i in range(7))

    def ilqr(self, u0, iterations, alphas=ILQR_ALPHAS, mu0=1e-3, mu_up=10.0, mu_down=0.1, mu_max=1e6, joints=None, ctrl=None, q=None, dq=None, hold=1,
             q_goal=None, dq_goal=None, ee_goal=None, w_q=0.0, w_dq=0.0, w_ee=0.0, w_u=0.0, w_q_final=None, w_dq_final=None, w_ee_final=None):
        """`iterations` iLQR iterations on this handle from the plan u0 [B, T, m], on rollout_cost's cost (its goals and weights) and the
        joints and motor words linearize uses; every env is its own problem with its own regularisation and step.  One iteration is five
        launches: ilqr_expand (the current trajectory, A, B and the cost's expansion), ilqr_backward with mu [B] on Quu's diagonal, and
        rollout_cost over the ladder `alphas` of step sizes, which must hold 0: the current plan's true cost comes from the same kernel
        in the same call.  Per env the step is the argmin over the ladder's costs that are finite and carry no flag but
        JACO_FLAG_SOLVER_MAXITER; a strict improvement on the alpha = 0 entry accepts it and multiplies mu by mu_down, anything else (a
        solve with JACO_LQR_NOT_PD too) keeps alpha = 0 and multiplies mu by mu_up (at most mu_max).  The next ilqr_expand re-simulates
        the chosen closed loop (u, K, x_ref, k, alpha [B]) and its applied motor words become the plan, so the line search materialises
        no trajectory; after the last iteration one more rollout_feedback launch does that for the result: 5 iterations + 1 launches.
        All selection happens on the device: nothing is read back, no synchronisation.
        {"u" [B, T, m]: the plan, "x" [B, T + 1, 2 n]: its trajectory, "K" [B, T, m, 2 n], "k" [B, T, m]: the last backward pass's, about
        the plan before the last step, "cost" [iterations + 1, B]: cost[i] is the alpha = 0 entry of iteration i's ladder, the cost of the
        plan that iteration started from, and cost[iterations] the chosen entry of the last ladder; a rollout fed its own applied ctrl
        reproduces itself bit for bit, so cost[i + 1] is also the chosen entry of iteration i's ladder and cost never rises, bit for bit,
        "accepted" [iterations, B] bool, "mu" [B], "status" [B] int32: the OR of the rollouts' status words (JACO_FLAG_NAN /
        JACO_FLAG_SOLVER_MAXITER) along the way to the result -- every ilqr_expand's rollout, every chosen ladder entry and the last
        rollout_feedback.  The backward pass's words are not in it: a solve with JACO_LQR_NOT_PD is an ordinary rejection and shows in
        "accepted" and "mu"}."""
        import torch
        sim = self.sim
        B, dev = sim.num_envs, sim.device
        ladder = [float(a) for a in alphas]
        if 0.0 not in ladder:
            raise ValueError("ilqr: the step sizes %s do not hold 0, the current plan" % (ladder,))
        if iterations < 1:
            raise ValueError("ilqr: %d iterations" % iterations)
        zero = ladder.index(0.0)
        alphas = self._filled(ladder)
        cost_args = dict(q_goal=q_goal, dq_goal=dq_goal, ee_goal=ee_goal, w_q=w_q, w_dq=w_dq, w_ee=w_ee, w_u=w_u, w_q_final=w_q_final, w_dq_final=w_dq_final,
                         w_ee_final=w_ee_final)
        where = dict(joints=joints, ctrl=ctrl, q=q, dq=dq, hold=hold)
        mu = torch.full((B,), float(mu0), dtype=torch.float32, device=dev)
        cost = torch.zeros(iterations + 1, B, dtype=torch.float32, device=dev)
        accepted = torch.zeros(iterations, B, dtype=torch.bool, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        u, K, x_ref, k, step = torch.as_tensor(u0, dtype=torch.float32, device=dev), None, None, None, None
        for i in range(iterations):
            e = self.ilqr_expand(u, K=K, x_ref=x_ref, k=k, alpha=step, **where, **cost_args)
            u, x_ref = e["u"], e["x"][:, :-1].contiguous()
            K, k, _, solved = self.ilqr_backward(e["A"], e["B"], e["lxx"], e["luu"], lx=e["lx"], lu=e["lu"], Vxx=e["Vxx"], Vx=e["Vx"], mu=mu, joints=joints)
            pd = solved == 0
            # (a solve that stopped at a knot leaves the rows below it unwritten: such an env keeps its plan, with zero gains)
            K, k = torch.where(pd[:, None, None, None], K, torch.zeros_like(K)), torch.where(pd[:, None, None], k, torch.zeros_like(k))
            c = self.rollout_cost(u, K=K, x_ref=x_ref, k=k, alphas=alphas, **where, **cost_args)
            usable = torch.isfinite(c["cost"]) & ((c["status"] & ~_lib.JACO_FLAG_SOLVER_MAXITER) == 0)
            ranked = torch.where(usable, c["cost"], torch.full_like(c["cost"], float("inf")))
            best = ranked.argmin(1, keepdim=True)
            here = c["cost"][:, zero]
            ok = pd & (ranked.gather(1, best)[:, 0] < here)
            chosen = torch.where(ok[:, None], best, torch.full_like(best, zero))
            step = alphas[chosen[:, 0]]
            mu = torch.where(ok, mu * float(mu_down), (mu * float(mu_up)).clamp(max=float(mu_max)))
            cost[i], cost[i + 1], accepted[i] = here, c["cost"].gather(1, chosen)[:, 0], ok
            status = status | e["status"] | c["status"].gather(1, chosen)[:, 0]
        p = self._closed_loop("ilqr", u, K, x_ref, k, step, joints, ctrl, q, dq, hold)
        return dict(u=p["u"], x=p["x"], K=K, k=k, cost=cost, accepted=accepted, mu=mu, status=status | p["r"]["status"])

    def rollout_cost(self, u, noise=None, K=None, x_ref=None, k=None, alphas=None, joints=None, q_goal=None, dq_goal=None, ee_goal=None, w_q=0.0,
                     w_dq=0.0, w_ee=0.0, w_u=0.0, w_q_final=None, w_dq_final=None, w_ee_final=None, ctrl=None, hold=1, q=None, dq=None,
                     trajectories=False):
        """rollout_feedback() costed inside the kernel, on the same joints (x = [q_J, dq_J], 2 n) and motor words (m): what a sampling
        planner or iLQR's line search wants of a rollout.  Env b follows its plan (u [B, T, m], K, x_ref, k as rollout_feedback()) with
        either noise [B, S, T, m] -- S samples per env, sample s applies u_t + noise[b, s, t] (one fp32 add onto the law's value) -- or
        alphas [A] step sizes, not both; the S (or A) rollouts of an env share its plan, goals and state through indices, nothing is
        copied.  The cost of a rollout:
            sum_t [ 1/2 w_u |u_t|^2 + 1/2 sum_j w_q[j] (q_(t+1)j - q_goal[b, j])^2 + 1/2 sum_j w_dq[j] (dq_(t+1)j - dq_goal[b, j])^2
                    + 1/2 w_ee |ee_(t+1) - ee_goal[b]|^2 ]
        with the *_final weights on the last knot (None: the running weight).  Goals: q_goal / dq_goal [B, n] or [B, T, n] (one missing:
        zeros, weight and all), ee_goal [B, 3] or [B, T, 3], all per env or all per env and knot.  Weights: scalars, or [n] (w_q, w_dq)
        and [m] (w_u) vectors; u is the commanded motor words, before the actuators' clamp; the other ctrl words (ctrl [B, nu], None:
        zeros) carry no cost.
        {"cost": [B, S], "terms": [B, S, 3] (ctrl, state and pose parts), "status": [B, S]}, a non-finite rollout costing +inf; with
        trajectories=True also rollout_feedback()'s "q", "dq", "ee_pos", "ee_mat", "u", every knot; without noise and alphas the S axis
        is squeezed.  One jaco_rollout_cost launch (BatchedMujoco.rollout_cost); the sim's state is not touched."""
        import torch
        B, dev, nu = self.sim.num_envs, self.sim.device, self.sim.nu
        dofs, qadr, acts = self._joint_subset(joints, "rollout_cost")
        n, m = len(dofs), len(acts)
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)
        u, K, x_ref, k, noise = f32(u), f32(K), f32(x_ref), f32(k), f32(noise)
        if u.dim() != 3 or u.shape[0] != B or u.shape[2] != m:
            raise ValueError("rollout_cost: u has shape %s, not [%d, T, %d]" % (tuple(u.shape), B, m))
        T = int(u.shape[1])
        if k is not None and k.shape != u.shape:
            raise ValueError("rollout_cost: k has shape %s, not u's %s" % (tuple(k.shape), tuple(u.shape)))
        if K is not None:
            if K.shape != (B, T, m, 2 * n):
                raise ValueError("rollout_cost: K has shape %s, not [%d, %d, %d, %d]" % (tuple(K.shape), B, T, m, 2 * n))
            if x_ref is None or x_ref.shape != (B, T, 2 * n):
                raise ValueError("rollout_cost: x_ref has shape %s, not [%d, %d, %d]" % (None if x_ref is None else tuple(x_ref.shape), B, T, 2 * n))
        if alphas is not None and k is None:
            raise ValueError("rollout_cost: alphas need k")
        if alphas is not None and noise is not None:
            raise ValueError("rollout_cost: noise or alphas, not both")
        if noise is not None and (noise.dim() != 4 or noise.shape[0] != B or tuple(noise.shape[2:]) != (T, m)):
            raise ValueError("rollout_cost: noise has shape %s, not [%d, S, %d, %d]" % (tuple(noise.shape), B, T, m))
        base = torch.zeros(B, nu, dtype=torch.float32, device=dev) if ctrl is None else f32(ctrl).reshape(B, nu)
        full = base[:, None, :].repeat(1, T, 1)
        at = self._words(acts)
        full[:, :, at] = u
        kff = gain = None
        if k is not None:
            kff = torch.zeros_like(full)
            kff[:, :, at] = k
        if K is not None:
            gain = torch.zeros(B, T, nu, 2 * n, dtype=torch.float32, device=dev)
            gain[:, :, at] = K
        index = alpha = eps = None
        S = 1
        if alphas is not None:
            alphas = f32(alphas).reshape(-1)
            S = int(alphas.numel())
            alpha = alphas.repeat(B)
        if noise is not None:
            S = int(noise.shape[1])
            eps = torch.zeros(B * S, T, nu, dtype=torch.float32, device=dev)
            eps[:, :, at] = noise.reshape(B * S, T, m)
        if alphas is not None or noise is not None:
            index = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(S)
        c = self._cost_arguments("rollout_cost", n, m, T, q_goal, dq_goal, ee_goal, w_q, w_dq, w_ee, w_u, w_q_final, w_dq_final, w_ee_final)
        wu = np.zeros(nu)
        wu[acts] = c["wu"]
        qpos, qvel = self._spliced(q, dq)
        want = ("cost", "terms", "status") + (("qpos", "qvel", "xpos", "xmat", "ctrl") if trajectories else ())
        r = self.sim.rollout_cost(full, qpos, qvel, noise=eps, gain=gain, x_ref=x_ref, dofs=dofs, feedforward=kff, alpha=alpha, plan_index=index,
                                  state_index=index, hold=hold, frame=self._frames[0], x_goal=c["x_goal"], p_goal=c["p_goal"], wx=c["wx"], wx_final=c["wxT"], wu=wu,
                                  wp=c["wp"], wp_final=c["wpT"], want=want)
        out = {"cost": r["cost"].reshape(B, S), "terms": r["terms"].reshape(B, S, 3), "status": r["status"].reshape(B, S)}
        if trajectories:
            tr = {"q": r["qpos"][..., qadr], "dq": r["qvel"][..., dofs], "ee_pos": r["xpos"], "ee_mat": r["xmat"], "u": r["ctrl"][..., acts]}
            out.update({key: t.reshape(B, S, t.shape[-2], t.shape[-1]) for key, t in tr.items()})
        return {key: t[:, 0] for key, t in out.items()} if index is None else out

    def mppi_update(self, u, noise, cost, temperature, status=None):
        """The MPPI update of the nominal from S costed samples per env: (u_new [B, T, m], weights [B, S]) with
            w = softmax(-(cost - min cost) / temperature) over the samples,   u_new = u + sum_s w[b, s] noise[b, s]
        for u [B, T, m], noise [B, S, T, m], cost [B, S] as rollout_cost(u, noise=noise) returns it.  A sample whose cost is not finite,
        or whose status (rollout_cost's, optional) is anything but 0 or JACO_FLAG_SOLVER_MAXITER, gets weight 0; an env with no usable
        sample keeps its u.  Batched torch on the sim's device, no synchronisation (small and memory-bound: not worth a kernel)."""
        import torch
        dev = self.sim.device
        u, noise, cost = [torch.as_tensor(t, dtype=torch.float32, device=dev) for t in (u, noise, cost)]
        if noise.dim() != 4 or tuple(noise.shape[:1] + noise.shape[2:]) != tuple(u.shape) or tuple(cost.shape) != tuple(noise.shape[:2]):
            raise ValueError("mppi_update: u %s, noise %s and cost %s are not [B, T, m], [B, S, T, m] and [B, S]" % (tuple(u.shape), tuple(noise.shape), tuple(cost.shape)))
        if not temperature > 0:
            raise ValueError("mppi_update: the temperature %r is not positive" % (temperature,))
        usable = torch.isfinite(cost)
        if status is not None:
            st = torch.as_tensor(status, device=dev).reshape(cost.shape)
            usable = usable & ((st & ~_lib.JACO_FLAG_SOLVER_MAXITER) == 0)
        c = torch.where(usable, cost, torch.full_like(cost, float("inf")))
        lowest = torch.where(usable.any(1, keepdim=True), c.min(1, keepdim=True).values, torch.zeros_like(c[:, :1]))
        e = torch.where(usable, torch.exp(-(c - lowest) / float(temperature)), torch.zeros_like(c))
        w = e / e.sum(1, keepdim=True).clamp_min(1e-30)   # (the lowest usable sample contributes exp(0) = 1: the sum is >= 1, or 0 with no sample)
        step = (w[:, :, None, None] * torch.where(usable[:, :, None, None], noise, torch.zeros_like(noise))).sum(1)
        return u + step, w

    def ilqr_backward(self, A, B, lxx, luu, lux=None, lx=None, lu=None, Vxx=None, Vx=None, mu=None, joints=None, full=False):
        """The backward pass of iLQR on the joints and actuators that linearize(joints=...) and rollout_feedback(joints=...) use: x =
        [q_J, dq_J] (2 n), u the motor words of those joints in the same order (m).  A [B, T, 2 n, 2 n], B [B, T, 2 n, m]: linearize's,
        stacked over the knots; the cost expansion lxx, luu, lux, lx, lu, the terminal Vxx, Vx and the regularisation mu as
        BatchedMujoco.lqr_backward takes them.  (K [B, T, m, 2 n], k [B, T, m], dV [B, 2], status [B]) for rollout_feedback(K=, k=,
        alphas=): the model's cost change of a step alpha is alpha dV[:, 0] + alpha^2 dV[:, 1]; status 0, or _lib.JACO_LQR_NOT_PD | t.
        full=True: (gain [B, T, nu, 2 n], kff [B, T, nu], dV, status), the rows scattered to the model's ctrl words by the kernel,
        ready for sim.rollout_feedback(gain=, feedforward=).  One jaco_lqr launch."""
        dofs, qadr, acts = self._joint_subset(joints, "ilqr_backward")
        n, m = len(dofs), len(acts)
        if A.dim() != 4 or tuple(A.shape[2:]) != (2 * n, 2 * n) or B.dim() != 4 or tuple(B.shape[2:]) != (2 * n, m):
            raise ValueError("ilqr_backward: A has shape %s and B %s, not [B, T, %d, %d] and [B, T, %d, %d]" % (tuple(A.shape), tuple(B.shape), 2 * n, 2 * n, 2 * n, m))
        scatter = dict(rows=acts, rows_out=self.sim.nu) if full else {}
        r = self.sim.lqr_backward(A, B, lxx, luu, lux=lux, lx=lx, lu=lu, Vxx=Vxx, Vx=Vx, mu=mu, **scatter)
        return r["gain"], r["kff"], r["dV"], r["status"]

    def lqr(self, A, B, Q, R, Qf=None, status=False):
        """lqr_gains(A, B, Q, R, Qf) in one jaco_lqr launch, in fp32 on the sim's device: K [..., T, m, nx] for A [..., T, nx, nx], B [...,
        T, nx, m], Q, Qf [nx, nx], R [m, m] or batched like A without the knot axis.  Where lqr_gains' linalg.solve returns garbage
        silently, a problem whose R + B'P B is not positive definite (or holds a number that is not finite) at knot t gets zero gains
        at the knots <= t and the status word _lib.JACO_LQR_NOT_PD | t.  status=True returns (K, status [...] int32, 0 = solved), a
        device tensor: reading it is the caller's synchronisation, which is why no error is raised here."""
        import torch
        f32 = lambda t: torch.as_tensor(t, dtype=torch.float32, device=self.sim.device)
        A, B = f32(A), f32(B)
        lead, nx, m = tuple(A.shape[:-3]), A.shape[-1], B.shape[-1]
        flat = lambda t, tail: None if t is None else (f32(t) if f32(t).dim() == len(tail) else f32(t).expand(lead + tail).reshape((-1,) + tail))
        A, B = A.reshape((-1,) + tuple(A.shape[-3:])), B.reshape((-1,) + tuple(B.shape[-3:]))
        # (zeros: a problem whose R + B'P B is not positive definite at some knot keeps zero gains from that knot down, not garbage)
        K = torch.zeros(A.shape[0], A.shape[1], m, nx, dtype=torch.float32, device=self.sim.device)
        st = self.sim.lqr_backward(A, B, flat(Q, (nx, nx)), flat(R, (m, m)), Vxx=flat(Qf, (nx, nx)),
                                   out=dict(gain=K, kff=None, dV=None, Vxx0=None, Vx0=None))["status"]
        K = K.reshape(lead + tuple(K.shape[1:]))
        return (K, st.reshape(lead)) if status else K

    def Tx(self, name, q=None, x=None):
        """[num_envs, 3] world position of the body origin, or of the point x (3-vector in the body frame) on it."""
        i = self._register(name)
        r = self._result(q)
        p = r["xpos"][:, i]
        if x is None:
            return p
        import torch
        x = torch.as_tensor(x, dtype=p.dtype, device=p.device).reshape(3)
        return p + (r["xmat"][:, i].reshape(-1, 3, 3) @ x)


def lqr_gains(A, B, Q, R, Qf=None):
    """K [..., T, m, nx]: the finite-horizon LQR gains of  x_{t+1} = A_t x_t + B_t u_t  (A [..., T, nx, nx], B [..., T, nx, m], as
    linearize returns them, stacked over the knots) under the cost  sum_t (dx' Q dx + du' R du) + dx_T' Qf dx_T  (Q, Qf [nx, nx], R
    [m, m], or batched like A; Qf None: Q), in rollout_feedback's sign convention: u = u_ref + K (x - x_ref).  The backward Riccati
    recursion in batched torch, in the tensors' dtype."""
    import torch
    T = A.shape[-3]
    Q, R = torch.as_tensor(Q, dtype=A.dtype, device=A.device), torch.as_tensor(R, dtype=A.dtype, device=A.device)
    P = Q if Qf is None else torch.as_tensor(Qf, dtype=A.dtype, device=A.device)
    Ks = []
    for t in range(T - 1, -1, -1):
        At, Bt = A[..., t, :, :], B[..., t, :, :]
        BtP = Bt.transpose(-1, -2) @ P
        Kt = -torch.linalg.solve(R + BtP @ Bt, BtP @ At)
        P = Q + At.transpose(-1, -2) @ P @ (At + Bt @ Kt)
        P = 0.5 * (P + P.transpose(-1, -2))
        Ks.append(Kt)
    return torch.stack(Ks[::-1], -3)


def quat_from_euler_rxyz(e):
    """[..., 3] 'rxyz' Euler angles -> [..., 4] unit quaternions, w first (transformations.quaternion_from_euler(a, b, c, 'rxyz'):
    qx(a) qy(b) qz(c)), in torch on the tensor's device."""
    import torch
    h = 0.5 * e
    ca, cb, cc = torch.cos(h[..., 0]), torch.cos(h[..., 1]), torch.cos(h[..., 2])
    sa, sb, sc = torch.sin(h[..., 0]), torch.sin(h[..., 1]), torch.sin(h[..., 2])
    w1, x1, y1, z1 = ca * cb, sa * cb, ca * sb, sa * sb
    q = torch.stack([w1 * cc - z1 * sc, x1 * cc + y1 * sc, y1 * cc - x1 * sc, w1 * sc + z1 * cc], -1)
    return q / q.norm(dim=-1, keepdim=True)


class Damping:
    """abr_control's null-space controller Damping(robot_config, kv): -kv M dq, filtered into the null space of the task."""

    def __init__(self, kv):
        self.kv = float(kv)


class RestingConfig:
    """abr_control's null-space controller RestingConfig(robot_config, rest_angles, kp, kv): M (kp e - kv dq) on the held joints, e the
    wrapped difference to their rest angles, filtered into the null space of the task.  rest_angles covers the joints of the controlled
    chains in order (one entry per joint; with two names either one list per name or both chains one after the other): a list with None
    for joints that are not held, or a [B, chain length] tensor (every joint held, per env)."""

    def __init__(self, rest_angles, kp, kv):
        self.rest_angles, self.kp, self.kv = rest_angles, float(kp), float(kv)


class BatchedOSC:
    """abr_control's OSC(robot_config, kp, ko, kv, vmax, ctrlr_dof, null_controllers) (env_mujoco_util.py:59-63) over a
    BatchedMujocoConfig: .generate() returns the ctrl rows of every env from ONE launch (jaco_osc; jaco_osc_task when task axes or
    null-space controllers are given).  names: one or two MJCF bodies whose origins and orientations are controlled (("EE",);
    ("EE_1", "EE_2") on the two-arm model: both arms in one launch); each drives the hinge joints on its own chain.  ctrlr_dof: six
    booleans (x, y, z, then the three rotational rows), or one such list per name; None: all six.  null_controllers: Damping and / or
    RestingConfig instances.  The quantities are those of a forward pass on the state the call is given (fresh; the reference's are one
    substep stale)."""

    def __init__(self, robot_config, names=("EE",), kp=50.0, ko=180.0, kv=20.0, vmax=(0.4, 1.0472), ctrlr_dof=None, null_controllers=()):
        self.robot_config, self.sim = robot_config, robot_config.sim
        self.names = (names,) if isinstance(names, str) else tuple(names)
        if not 1 <= len(self.names) <= _lib.JACO_OSC_MAX_FRAMES:
            raise ValueError("BatchedOSC controls 1 to %d frames, not %d" % (_lib.JACO_OSC_MAX_FRAMES, len(self.names)))
        self.frames = [robot_config.table.jaco_frame(n, point=np.zeros(3)) for n in self.names]
        self.chains = [robot_config.table.chain(n) for n in self.names]   # (qpos addresses, dof addresses) per name
        self.options = dict(kp=float(kp), ko=float(ko), kv=float(kv), vmax_xyz=float(vmax[0]), vmax_abg=float(vmax[1]))
        self.axes = _lib.osc_axes(ctrlr_dof, len(self.names))[:len(self.names)]
        self.rotational = any((a or 63) & 56 for a in self.axes)
        self.task = self._task(ctrlr_dof, list(null_controllers))   # the task keywords of sim.osc; empty: plain jaco_osc

    def _task(self, ctrlr_dof, null_controllers):
        task = {} if ctrlr_dof is None else dict(axes=list(self.axes))
        unknown = [c for c in null_controllers if not isinstance(c, (Damping, RestingConfig))]
        resting = [c for c in null_controllers if isinstance(c, RestingConfig)]
        if unknown or len(resting) > 1:
            raise ValueError("null_controllers holds Damping instances and at most one RestingConfig")
        damping = sum(c.kv for c in null_controllers if isinstance(c, Damping))
        if damping:
            task["null_kv"] = damping
        if resting:
            import torch
            qadr = [a for c in self.chains for a in c[0]]
            dadr = [d for c in self.chains for d in c[1]]
            ra = resting[0].rest_angles
            B = self.sim.num_envs
            rest = torch.zeros(B, self.sim.nq, dtype=torch.float32, device=self.sim.device)
            if torch.is_tensor(ra):
                rest[:, qadr] = ra.to(dtype=torch.float32, device=rest.device).reshape(B, len(qadr))
                held = dadr
            else:
                ra = list(ra)
                if len(ra) == len(self.chains) and all(hasattr(r, "__len__") for r in ra):
                    ra = [torch.as_tensor(r, dtype=torch.float32).reshape(B, -1).T if torch.is_tensor(r) else r for r in ra]
                    ra = [x for r in ra for x in r]
                if len(ra) != len(qadr):
                    raise ValueError("RestingConfig: %d rest angles for %d controlled joints" % (len(ra), len(qadr)))
                held = [d for d, r in zip(dadr, ra) if r is not None]
                for a, r in zip(qadr, ra):
                    if r is not None:
                        rest[:, a] = torch.as_tensor(r, dtype=torch.float32, device=rest.device)
            if not held:
                raise ValueError("RestingConfig holds no joint")
            task.update(rest_qpos=rest, rest_kp=resting[0].kp, rest_kv=resting[0].kv, rest_mask=sum(1 << d for d in held))
        return task

    def _state(self, q, dq):
        """Full qpos / qvel rows with the controlled chains' q / dq ([B, sum of chain lengths]) spliced into the current state."""
        return splice(self.sim, [a for c in self.chains for a in c[0]], [d for c in self.chains for d in c[1]], q, dq)

    def generate_pose(self, pos, quat=None, q=None, dq=None, ctrl=None):
        """ctrl [B, nu] for target positions pos [B, 3] (or [B, n_names, 3]) and unit quaternions quat [B, 4] ([B, n_names, 4]), w first;
        quat may be left out when ctrlr_dof selects no rotational row.  q / dq: joint angles / velocities of the controlled chains
        (default: the sim's state); ctrl: the row to write into (default zeros) -- every word but the controlled motors' is kept."""
        if quat is None and self.rotational:
            raise ValueError("generate_pose needs target quaternions: ctrlr_dof selects a rotational axis")
        qpos, qvel = self._state(q, dq)
        return self.sim.osc(self.frames, pos, quat, qpos, qvel, ctrl, **self.task, **self.options)["ctrl"]

    def generate(self, target, q=None, dq=None, ctrl=None):
        """abr_control's generate(q, dq, target): target [B, 6] (or [B, n_names, 6]) = position + 'rxyz' Euler angles."""
        import torch
        t = torch.as_tensor(target, dtype=torch.float32, device=self.sim.device).reshape(self.sim.num_envs, len(self.names), 6)
        return self.generate_pose(t[..., :3], quat_from_euler_rxyz(t[..., 3:]), q, dq, ctrl)

    def rollout_pose(self, pos, quat, hold=1, per_substep=True, q=None, dq=None, ctrl=None, final_only=False):
        """Where does this controller take the arm?  K candidate target sequences per env, pos [B, K, T, 3] / quat [B, K, T, 4] (unit
        quaternions, w first; [B, K, T, n_names, .] with two names: both arms driven), each knot's target followed for `hold` substeps
        with the controller evaluated inside the kernel before every substep (per_substep=False: once per knot, held), from the sim's
        state (or q / dq, the controlled chains' angles / velocities spliced into it).  The K candidates of an env share its state row
        through a state index: nothing is copied.  ctrl [B, nu]: the row the torques are written into at every evaluation (default
        zeros) -- gripper commands stay as given.  Contact-free, with joint limits (BatchedMujoco.rollout_osc: one jaco_rollout_osc
        launch; the sim's state is not touched).
        {"q": [B, K, T, n_arm], "dq": likewise: the robot config's joints after each knot; "ee_pos": [B, K, T, 3], "ee_mat": [B, K, T, 9]:
        the pose of the controller's first frame; "u": [B, K, E, nu]: the commanded ctrl row of every evaluation (E = T * hold, or T
        without per_substep; all of them also with final_only); "status": [B, K], with _lib.JACO_ROLLOUT_OSC_SINGULAR0 / 1 where a frame
        took the pseudo-inverse branch}; final_only=True: T = 1, the last knot.  Runs the plain controller: one built with ctrlr_dof
        or null_controllers is refused."""
        import torch
        if self.task:
            raise ValueError("BatchedOSC.rollout runs the plain controller: this one was built with ctrlr_dof or null_controllers (jaco_osc_task), "
                             "which the rollout kernel does not evaluate")
        B, dev, nf, cfg = self.sim.num_envs, self.sim.device, len(self.names), self.robot_config
        pos, quat = torch.as_tensor(pos, dtype=torch.float32, device=dev), torch.as_tensor(quat, dtype=torch.float32, device=dev)
        if pos.dim() not in (4, 5) or pos.shape[0] != B or pos.shape[-1] != 3 or (pos.dim() == 5 and pos.shape[3] != nf) or (pos.dim() == 4 and nf != 1):
            raise ValueError("rollout: the target positions have shape %s, not [%d, K, T, 3] (one name) or [%d, K, T, %d, 3]" % (tuple(pos.shape), B, B, nf))
        K, T = int(pos.shape[1]), int(pos.shape[2])
        if tuple(quat.shape) != tuple(pos.shape[:-1]) + (4,):
            raise ValueError("rollout: the target quaternions have shape %s, not %s" % (tuple(quat.shape), tuple(pos.shape[:-1]) + (4,)))
        base = None
        if ctrl is not None:
            base = torch.as_tensor(ctrl, dtype=torch.float32, device=dev).reshape(B, 1, 1, self.sim.nu).expand(B, K, T, self.sim.nu).reshape(B * K, T, self.sim.nu)
        qpos, qvel = self._state(q, dq)
        index = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(K)
        r = self.sim.rollout_osc(self.frames, pos.reshape(B * K, T, nf, 3), quat.reshape(B * K, T, nf, 4), qpos, qvel, ctrl=base, state_index=index, hold=hold,
                                 per_substep=per_substep, frame=self.frames[0], final_only=final_only, **self.options)
        out = {"q": r["qpos"][..., cfg.arm_qadr], "dq": r["qvel"][..., cfg.arm], "ee_pos": r["xpos"], "ee_mat": r["xmat"], "u": r["ctrl"]}
        out = {k: t.reshape(B, K, t.shape[-2], t.shape[-1]) for k, t in out.items()}
        out["status"] = r["status"].reshape(B, K)
        return out

    def rollout(self, target, hold=1, per_substep=True, q=None, dq=None, ctrl=None, final_only=False):
        """rollout_pose() in abr_control's convention: target [B, K, T, 6] ([B, K, T, n_names, 6]) = position + 'rxyz' Euler angles."""
        import torch
        t = torch.as_tensor(target, dtype=torch.float32, device=self.sim.device)
        if t.shape[-1] != 6:
            raise ValueError("rollout: target has shape %s, not [B, K, T, 6] or [B, K, T, n_names, 6]" % (tuple(t.shape),))
        return self.rollout_pose(t[..., :3], quat_from_euler_rxyz(t[..., 3:]), hold, per_substep, q, dq, ctrl, final_only)


class BatchedJoint:
    """abr_control's Joint(robot_config, kp, kv) over a BatchedMujocoConfig: .generate() returns the ctrl rows of every env from ONE
    launch (jaco_joint): u = M (kp s e + kv (target_velocity - dq)) + qfrc_bias on the controlled joints, e the joint error (wrapped
    into [-pi, pi) on unlimited joints only -- abr_control wraps every joint; a limited joint is never sent through its limit here), s
    the one scale of the velocity limit vmax (rad/s; None: no limiting).  joints: MJCF joint names (hinge joints with a motor actuator),
    in the order the per-joint lists of the methods follow; default: every such joint of the model, in dof order (both arms on the
    two-arm model).  The quantities are those of a forward pass on the state the call is given.  Joint damping is not compensated."""

    def __init__(self, robot_config, kp=50.0, kv=20.0, vmax=None, joints=None):
        self.robot_config, self.sim = robot_config, robot_config.sim
        M, names = robot_config.table.M, robot_config.table.names["joint"]
        motor = robot_config.table.motor_of_dof()
        if joints is None:
            ids = sorted((j for j in range(len(names)) if M["jnt_type"][j] == kin.JNT_HINGE and int(M["jnt_dofadr"][j]) in motor),
                         key=lambda j: int(M["jnt_dofadr"][j]))
        else:
            ids = robot_config.table.hinge_joints(joints)
            for j in ids:
                if int(M["jnt_dofadr"][j]) not in motor:
                    raise ValueError("joint %r has no motor actuator (a position servo cannot be torque controlled)" % names[j])
        if not ids:
            raise ValueError("BatchedJoint controls no joint")
        self.joints = [names[j] for j in ids]
        self.qadr = [int(M["jnt_qposadr"][j]) for j in ids]
        self.dadr = [int(M["jnt_dofadr"][j]) for j in ids]
        self.dof_mask = sum(1 << d for d in self.dadr)
        self.kp, self.kv, self.vmax = float(kp), float(kv), 0.0 if vmax is None else float(vmax)

    def _rows(self, t, adr, width, base, what):
        """A full [B, width] row from t: a full row already, or one entry per controlled joint spliced into base() at `adr`."""
        if t is None:
            return None
        import torch
        B, n = self.sim.num_envs, len(adr)
        t = torch.as_tensor(t, dtype=torch.float32, device=self.sim.device)
        if t.dim() == 1 and t.numel() == n:
            t = t.reshape(1, n).expand(B, n)
        if t.dim() >= 1 and t.shape[-1] == n and t.numel() == B * n:
            row = base()
            row[:, adr] = t.reshape(B, n)
            return row.contiguous()
        if t.dim() >= 1 and t.shape[-1] == width and t.numel() == B * width:
            return t.reshape(B, width).contiguous()
        raise ValueError("%s has shape %s: one entry per controlled joint ([%d] or [%d, %d]) or full rows ([%d, %d])" % (what, tuple(t.shape), n, B, n, B, width))

    def _call(self, target, target_velocity, qacc, q, dq, ctrl, kp, kv, vmax):
        import torch
        state = {}

        def cur(i):
            if not state:
                state["s"] = self.sim.get_state()
            return state["s"][i].clone()
        zeros = lambda w: (lambda: torch.zeros(self.sim.num_envs, w, dtype=torch.float32, device=self.sim.device))
        return self.sim.joint(self._rows(target, self.qadr, self.sim.nq, zeros(self.sim.nq), "target"),
                              self._rows(target_velocity, self.dadr, self.sim.nv, zeros(self.sim.nv), "target_velocity"),
                              self._rows(qacc, self.dadr, self.sim.nv, zeros(self.sim.nv), "qacc"),
                              self._rows(q, self.qadr, self.sim.nq, lambda: cur(0), "q"), self._rows(dq, self.dadr, self.sim.nv, lambda: cur(1), "dq"),
                              ctrl, kp=kp, kv=kv, vmax=vmax, dof_mask=self.dof_mask)

    def generate(self, target, target_velocity=None, q=None, dq=None, ctrl=None):
        """ctrl [B, nu] for the joint targets `target`: one angle per controlled joint ([n] for every env, or [B, n]) or a full qpos row
        [B, nq] (a BatchedMujoco.ik result row as it is); target_velocity likewise ([n], [B, n] or [B, nv]; default zeros).  q / dq: the
        state to compute at, per controlled joint (spliced into the sim's state) or full rows; default: the sim's state.  ctrl: the row
        to write into (default zeros) -- every word but the controlled motors' is kept.  (abr_control's generate(q, dq, target,
        target_velocity) with the state last, since it defaults to the sim's.)"""
        return self._call(target, target_velocity, None, q, dq, ctrl, self.kp, self.kv, self.vmax)

    def inverse_dynamics(self, qacc, q=None, dq=None, ctrl=None):
        """ctrl [B, nu] holding the torques that give the controlled joints the accelerations qacc ([n], [B, n] or [B, nv]) at the state:
        M[A, A] qacc + qfrc_bias (the other dofs' accelerations taken as zero)."""
        return self._call(None, None, qacc, q, dq, ctrl, 0.0, 0.0, 0.0)

    def gravity_compensation(self, q=None, dq=None, ctrl=None):
        """ctrl [B, nu] holding qfrc_bias on the controlled joints: gravity, Coriolis and centrifugal forces cancelled (abr_control's
        Floating)."""
        return self._call(None, None, None, q, dq, ctrl, 0.0, 0.0, 0.0)
