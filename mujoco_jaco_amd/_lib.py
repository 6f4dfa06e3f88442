"""ctypes binding of libjaco_env.so (C ABI: include/jaco_env.h).

There is deliberately no fallback: if the HIP extension has not been built
(``python -c "import __graft_entry__ as g; g.build()"``) importing this module raises.
"""
import ctypes
import numbers
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("JACO_ENV_LIB", "libjaco_env.so"))
ASSETS = os.path.join(_HERE, "assets")


JACO_QUERY_MAX_FRAMES = 16


class JacoFrame(ctypes.Structure):
    """JacoFrame of include/jaco_env.h: fused body (-1 world), pose in that body's frame, Jacobian reference point in the frame."""
    _fields_ = [("body", ctypes.c_int), ("pos", ctypes.c_float * 3), ("mat", ctypes.c_float * 9), ("point", ctypes.c_float * 3)]


class JacoQueryOut(ctypes.Structure):
    _fields_ = [("xpos", ctypes.c_void_p), ("xmat", ctypes.c_void_p), ("jac", ctypes.c_void_p), ("qM", ctypes.c_void_p), ("qfrc_bias", ctypes.c_void_p)]


JACO_IK_MAX_ITERS = 256


class JacoIkOptions(ctypes.Structure):
    """JacoIkOptions of include/jaco_env.h; a fresh instance holds the API defaults (JACO_IK_DEFAULTS)."""
    _fields_ = [("tol_pos", ctypes.c_float), ("tol_rot", ctypes.c_float), ("damping", ctypes.c_float), ("max_step", ctypes.c_float),
                ("max_iters", ctypes.c_int32), ("reserved", ctypes.c_int32), ("dof_mask", ctypes.c_uint64)]
    DEFAULTS = dict(tol_pos=1e-5, tol_rot=1e-4, damping=0.02, max_step=0.3, max_iters=60, dof_mask=0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown IK option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


JACO_OSC_MAX_FRAMES = 2


class JacoOscOptions(ctypes.Structure):
    """JacoOscOptions of include/jaco_env.h; a fresh instance holds the API defaults (JACO_OSC_DEFAULTS: the reference's gains)."""
    _fields_ = [("kp", ctypes.c_float), ("ko", ctypes.c_float), ("kv", ctypes.c_float), ("vmax_xyz", ctypes.c_float), ("vmax_abg", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("dof_mask", ctypes.c_uint64)]
    DEFAULTS = dict(kp=50.0, ko=180.0, kv=20.0, vmax_xyz=0.4, vmax_abg=1.0472, dof_mask=0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown OSC option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


class JacoOscTask(ctypes.Structure):
    """JacoOscTask of include/jaco_env.h: the task axes and null-space terms of jaco_osc_task; a fresh instance is plain jaco_osc (all six
    axes, no null-space term)."""
    _fields_ = [("axes", ctypes.c_uint32 * JACO_OSC_MAX_FRAMES), ("null_kv", ctypes.c_float), ("rest_kp", ctypes.c_float), ("rest_kv", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("rest_mask", ctypes.c_uint64)]
    DEFAULTS = dict(axes=(0,) * JACO_OSC_MAX_FRAMES, null_kv=0.0, rest_kp=0.0, rest_kv=0.0, rest_mask=0)

    def __init__(self, **task):
        unknown = set(task) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown OSC task field(s) %s: the fields are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        f = {**self.DEFAULTS, **task}
        f["axes"] = (ctypes.c_uint32 * JACO_OSC_MAX_FRAMES)(*f["axes"])
        super().__init__(**f)


class JacoJointOptions(ctypes.Structure):
    """JacoJointOptions of include/jaco_env.h; a fresh instance holds the API defaults (JACO_JOINT_DEFAULTS)."""
    _fields_ = [("kp", ctypes.c_float), ("kv", ctypes.c_float), ("vmax", ctypes.c_float), ("reserved", ctypes.c_int32), ("dof_mask", ctypes.c_uint64)]
    DEFAULTS = dict(kp=50.0, kv=20.0, vmax=0.0, dof_mask=0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown joint-controller option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


class JacoFdOptions(ctypes.Structure):
    """JacoFdOptions of include/jaco_env.h; a fresh instance holds the API defaults (JACO_FD_DEFAULTS)."""
    _fields_ = [("eps_qpos", ctypes.c_float), ("eps_qvel", ctypes.c_float), ("implicit_damping", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("dof_mask", ctypes.c_uint64)]
    DEFAULTS = dict(eps_qpos=2.0 ** -8, eps_qvel=2.0 ** -3, implicit_damping=0, dof_mask=0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown forward-dynamics option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


class JacoFdOut(ctypes.Structure):
    _fields_ = [("qacc", ctypes.c_void_p), ("qfrc_smooth", ctypes.c_void_p), ("dqacc_dqpos", ctypes.c_void_p), ("dqacc_dqvel", ctypes.c_void_p),
                ("dqacc_dctrl", ctypes.c_void_p)]


JACO_ROLLOUT_MAX_SUBSTEPS = 16384
JACO_ROLLOUT_BAD_INDEX = 0x80000   # jaco_rollout: the rollout's state index was outside [0, nstates); its output rows were left untouched


class JacoRolloutOptions(ctypes.Structure):
    """JacoRolloutOptions of include/jaco_env.h; a fresh instance holds hold = 1 and final_only = 0 (nknots has no default: it is the
    ctrl tensor's knot count)."""
    _fields_ = [("nknots", ctypes.c_int32), ("hold", ctypes.c_int32), ("final_only", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    DEFAULTS = dict(nknots=0, hold=1, final_only=0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown rollout option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


class JacoRolloutOut(ctypes.Structure):
    _fields_ = [("qpos", ctypes.c_void_p), ("qvel", ctypes.c_void_p), ("xpos", ctypes.c_void_p), ("xmat", ctypes.c_void_p), ("status", ctypes.c_void_p)]


JACO_ROLLOUT_FB_MAX_DOFS = 18


class JacoRolloutFbOptions(ctypes.Structure):
    """JacoRolloutFbOptions of include/jaco_env.h; a fresh instance holds hold = 1, final_only = 0, per_substep = 0 and no dofs.  dofs: a
    list of at most JACO_ROLLOUT_FB_MAX_DOFS hinge dofs (ndofs is its length; the library checks the dofs themselves)."""
    _fields_ = [("nknots", ctypes.c_int32), ("hold", ctypes.c_int32), ("final_only", ctypes.c_int32), ("per_substep", ctypes.c_int32),
                ("ndofs", ctypes.c_int32), ("dofs", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS), ("reserved", ctypes.c_int32)]
    DEFAULTS = dict(nknots=0, hold=1, final_only=0, per_substep=0, dofs=())

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown closed-loop rollout option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        o = {**self.DEFAULTS, **options}
        dofs = [int(d) for d in o.pop("dofs")]
        if len(dofs) > JACO_ROLLOUT_FB_MAX_DOFS:
            raise ValueError("%d dofs: a closed-loop rollout takes at most %d" % (len(dofs), JACO_ROLLOUT_FB_MAX_DOFS))
        super().__init__(ndofs=len(dofs), **o)
        self.dofs[:len(dofs)] = dofs


class JacoRolloutPlan(ctypes.Structure):
    _fields_ = [("ctrl", ctypes.c_void_p), ("kff", ctypes.c_void_p), ("gain", ctypes.c_void_p), ("xref", ctypes.c_void_p), ("alpha", ctypes.c_void_p),
                ("plan_idx", ctypes.c_void_p), ("nplans", ctypes.c_int32)]


class JacoRolloutFbOut(ctypes.Structure):
    _fields_ = [("qpos", ctypes.c_void_p), ("qvel", ctypes.c_void_p), ("xpos", ctypes.c_void_p), ("xmat", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("ctrl", ctypes.c_void_p)]


JACO_ROLLOUT_COST_MAX_NU = 18
JACO_FLAG_NAN, JACO_FLAG_SOLVER_MAXITER = 8, 16   # the status bits of a rollout (include/jaco_env.h): a NAN rollout costs +inf


class JacoRolloutCostOptions(ctypes.Structure):
    """JacoRolloutCostOptions of include/jaco_env.h; a fresh instance holds hold = 1, final_only = 0, goal_per_knot = 0, no dofs and zero
    weights.  dofs: at most JACO_ROLLOUT_FB_MAX_DOFS hinge dofs; wx / wxT: at most 2 x that many state weights (running / last knot), wu:
    at most JACO_ROLLOUT_COST_MAX_NU ctrl weights, each zero-filled to its array's length; wp / wpT: the pose weights."""
    _fields_ = [("nknots", ctypes.c_int32), ("hold", ctypes.c_int32), ("final_only", ctypes.c_int32), ("goal_per_knot", ctypes.c_int32),
                ("ndofs", ctypes.c_int32), ("dofs", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS),
                ("wx", ctypes.c_float * (2 * JACO_ROLLOUT_FB_MAX_DOFS)), ("wxT", ctypes.c_float * (2 * JACO_ROLLOUT_FB_MAX_DOFS)),
                ("wu", ctypes.c_float * JACO_ROLLOUT_COST_MAX_NU), ("wp", ctypes.c_float), ("wpT", ctypes.c_float), ("reserved", ctypes.c_int32)]
    DEFAULTS = dict(nknots=0, hold=1, final_only=0, goal_per_knot=0, dofs=(), wx=(), wxT=(), wu=(), wp=0.0, wpT=0.0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown costed rollout option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        o = {**self.DEFAULTS, **options}
        dofs = [int(d) for d in o.pop("dofs")]
        if len(dofs) > JACO_ROLLOUT_FB_MAX_DOFS:
            raise ValueError("%d dofs: a costed rollout takes at most %d" % (len(dofs), JACO_ROLLOUT_FB_MAX_DOFS))
        arrays = {k: [float(w) for w in o.pop(k)] for k in ("wx", "wxT", "wu")}
        for k, w in arrays.items():
            if len(w) > len(getattr(self, k)):
                raise ValueError("%d weights in %s: a costed rollout takes at most %d" % (len(w), k, len(getattr(self, k))))
        super().__init__(ndofs=len(dofs), **o)
        self.dofs[:len(dofs)] = dofs
        for k, w in arrays.items():
            getattr(self, k)[:len(w)] = w


class JacoRolloutGoal(ctypes.Structure):
    _fields_ = [("noise", ctypes.c_void_p), ("xgoal", ctypes.c_void_p), ("pgoal", ctypes.c_void_p)]


class JacoRolloutCostOut(ctypes.Structure):
    _fields_ = [("qpos", ctypes.c_void_p), ("qvel", ctypes.c_void_p), ("xpos", ctypes.c_void_p), ("xmat", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("ctrl", ctypes.c_void_p), ("cost", ctypes.c_void_p), ("terms", ctypes.c_void_p)]


JACO_ROLLOUT_OSC_SINGULAR0, JACO_ROLLOUT_OSC_SINGULAR1 = 0x200000, 0x400000   # jaco_rollout_osc's status: frame 0 / 1 took the pseudo-inverse branch at some evaluation


class JacoRolloutOscOptions(ctypes.Structure):
    """JacoRolloutOscOptions of include/jaco_env.h; a fresh instance holds hold = 1, final_only = 0, per_substep = 1, one frame and
    JacoOscOptions' gains."""
    _fields_ = [("nknots", ctypes.c_int32), ("hold", ctypes.c_int32), ("final_only", ctypes.c_int32), ("per_substep", ctypes.c_int32),
                ("nframes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("kp", ctypes.c_float), ("ko", ctypes.c_float), ("kv", ctypes.c_float),
                ("vmax_xyz", ctypes.c_float), ("vmax_abg", ctypes.c_float), ("dof_mask", ctypes.c_uint64)]
    DEFAULTS = dict(nknots=0, hold=1, final_only=0, per_substep=1, nframes=1, **JacoOscOptions.DEFAULTS)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown OSC rollout option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        super().__init__(**{**self.DEFAULTS, **options})


class JacoRolloutOscPlan(ctypes.Structure):
    _fields_ = [("ctrl", ctypes.c_void_p), ("target_pos", ctypes.c_void_p), ("target_quat", ctypes.c_void_p), ("plan_idx", ctypes.c_void_p),
                ("nplans", ctypes.c_int32)]


JACO_TRANSITION_MAX_HOLD = 1024


class JacoTransitionOptions(ctypes.Structure):
    """JacoTransitionOptions of include/jaco_env.h; a fresh instance holds hold = 1, centered = 1, groups = 0 (the library chooses), no
    dofs, no ctrl words and the default steps.  dofs / acts: at most JACO_ROLLOUT_FB_MAX_DOFS hinge dofs / ctrl words each (ndofs and
    nacts are their lengths; the library checks the entries themselves)."""
    _fields_ = [("hold", ctypes.c_int32), ("centered", ctypes.c_int32), ("groups", ctypes.c_int32),
                ("ndofs", ctypes.c_int32), ("dofs", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS),
                ("nacts", ctypes.c_int32), ("acts", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS),
                ("eps_qpos", ctypes.c_float), ("eps_qvel", ctypes.c_float), ("eps_ctrl", ctypes.c_float), ("reserved", ctypes.c_int32)]
    DEFAULTS = dict(hold=1, centered=1, groups=0, dofs=(), acts=(), eps_qpos=JacoFdOptions.DEFAULTS["eps_qpos"], eps_qvel=JacoFdOptions.DEFAULTS["eps_qvel"],
                    eps_ctrl=2.0 ** -6)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown transition option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        o = {**self.DEFAULTS, **options}
        dofs, acts = [int(d) for d in o.pop("dofs")], [int(a) for a in o.pop("acts")]
        for what, lst in (("dofs", dofs), ("ctrl words", acts)):
            if len(lst) > JACO_ROLLOUT_FB_MAX_DOFS:
                raise ValueError("%d %s: a transition Jacobian takes at most %d" % (len(lst), what, JACO_ROLLOUT_FB_MAX_DOFS))
        super().__init__(ndofs=len(dofs), nacts=len(acts), **o)
        self.dofs[:len(dofs)] = dofs
        self.acts[:len(acts)] = acts


class JacoTransitionOut(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("next_qpos", ctypes.c_void_p), ("next_qvel", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class JacoCostQuadOptions(ctypes.Structure):
    """JacoCostQuadOptions of include/jaco_env.h; a fresh instance holds goal_per_knot = 0, no dofs, no ctrl words and zero weights
    (nknots has no default: it is the trajectories' knot count).  dofs / acts: at most JACO_ROLLOUT_FB_MAX_DOFS hinge dofs / ctrl words;
    wx / wxT: at most 2 x that many state weights (running / last knot), wu: one weight per entry of acts, each zero-filled to its
    array's length; wp / wpT: the pose weights."""
    _fields_ = [("nknots", ctypes.c_int32), ("goal_per_knot", ctypes.c_int32),
                ("ndofs", ctypes.c_int32), ("dofs", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS),
                ("nacts", ctypes.c_int32), ("acts", ctypes.c_int32 * JACO_ROLLOUT_FB_MAX_DOFS),
                ("wx", ctypes.c_float * (2 * JACO_ROLLOUT_FB_MAX_DOFS)), ("wxT", ctypes.c_float * (2 * JACO_ROLLOUT_FB_MAX_DOFS)),
                ("wu", ctypes.c_float * JACO_ROLLOUT_FB_MAX_DOFS), ("wp", ctypes.c_float), ("wpT", ctypes.c_float), ("reserved", ctypes.c_int32)]
    DEFAULTS = dict(nknots=0, goal_per_knot=0, dofs=(), acts=(), wx=(), wxT=(), wu=(), wp=0.0, wpT=0.0)

    def __init__(self, **options):
        unknown = set(options) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown cost expansion option(s) %s: the options are %s" % (sorted(unknown), sorted(self.DEFAULTS)))
        o = {**self.DEFAULTS, **options}
        dofs, acts = [int(d) for d in o.pop("dofs")], [int(a) for a in o.pop("acts")]
        for what, lst in (("dofs", dofs), ("ctrl words", acts)):
            if len(lst) > JACO_ROLLOUT_FB_MAX_DOFS:
                raise ValueError("%d %s: a cost expansion takes at most %d" % (len(lst), what, JACO_ROLLOUT_FB_MAX_DOFS))
        arrays = {k: [float(w) for w in o.pop(k)] for k in ("wx", "wxT", "wu")}
        for k, w in arrays.items():
            if len(w) > len(getattr(self, k)):
                raise ValueError("%d weights in %s: a cost expansion takes at most %d" % (len(w), k, len(getattr(self, k))))
        super().__init__(ndofs=len(dofs), nacts=len(acts), **o)
        self.dofs[:len(dofs)] = dofs
        self.acts[:len(acts)] = acts
        for k, w in arrays.items():
            getattr(self, k)[:len(w)] = w


class JacoCostQuadGoal(ctypes.Structure):
    _fields_ = [("xgoal", ctypes.c_void_p), ("pgoal", ctypes.c_void_p), ("goal_idx", ctypes.c_void_p), ("ngoals", ctypes.c_int32)]
    DEFAULTS = dict(xgoal=None, pgoal=None, goal_idx=None, ngoals=0)


class JacoCostQuadOut(ctypes.Structure):
    _fields_ = [("lx", ctypes.c_void_p), ("lxx", ctypes.c_void_p), ("lu", ctypes.c_void_p), ("Vx", ctypes.c_void_p), ("Vxx", ctypes.c_void_p),
                ("l", ctypes.c_void_p), ("status", ctypes.c_void_p)]
    DEFAULTS = dict.fromkeys(("lx", "lxx", "lu", "Vx", "Vxx", "l", "status"))


JACO_LQR_MAX_NX, JACO_LQR_MAX_NU = 36, 18
JACO_LQR_BAD_INDEX = 0x80000   # jaco_lqr: the solve's problem index was outside [0, nprob); only its status word was written
JACO_LQR_NOT_PD = 0x100000     # jaco_lqr: Quu + mu I not positive definite, or a non-finite number, at knot (status & 0xffff)
JACO_LQR_SHARED = dict(lxx=1, luu=2, lux=4, lx=8, lu=16, Vxx=32, Vx=64)   # the bits of shared_knots / shared_probs


class JacoLqrOptions(ctypes.Structure):
    """JacoLqrOptions of include/jaco_env.h.  rows: the output row of every control (nu distinct rows in [0, rows_out)); with
    rows_out = 0 control a goes to row a."""
    _fields_ = [("nknots", ctypes.c_int32), ("nx", ctypes.c_int32), ("nu", ctypes.c_int32), ("rows_out", ctypes.c_int32),
                ("row", ctypes.c_int32 * JACO_LQR_MAX_NU), ("shared_knots", ctypes.c_uint32), ("shared_probs", ctypes.c_uint32)]

    def __init__(self, nknots=0, nx=0, nu=0, rows_out=0, rows=(), shared_knots=0, shared_probs=0):
        rows = [int(r) for r in rows]
        if len(rows) > JACO_LQR_MAX_NU:
            raise ValueError("%d rows: the backward pass takes at most %d controls" % (len(rows), JACO_LQR_MAX_NU))
        super().__init__(nknots=nknots, nx=nx, nu=nu, rows_out=rows_out, shared_knots=shared_knots, shared_probs=shared_probs)
        self.row[:len(rows)] = rows


class JacoLqrProblem(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("A", "B", "lxx", "luu", "lux", "lx", "lu", "Vxx", "Vx", "mu", "prob_idx")] + [("nprob", ctypes.c_int32)]


class JacoLqrOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("gain", "kff", "dV", "Vxx0", "Vx0", "status")]


def osc_axes(axes, nframes):
    """The axes words of JacoOscTask for `nframes` frames from what the Python surface accepts: None (all six everywhere), one 6-bit mask
    or one list of six booleans (x, y, z, then the three rotational rows) for every frame, or a list of one of those per frame."""
    def one(a):
        if isinstance(a, numbers.Integral):
            return int(a)
        a = list(a)
        if len(a) != 6:
            raise ValueError("task axes are a 6-bit mask or six booleans, not %d entries" % len(a))
        mask = sum(1 << r for r, on in enumerate(a) if on)
        if not mask:
            raise ValueError("the task axes select no row")
        return mask
    if axes is None:
        return (0,) * JACO_OSC_MAX_FRAMES
    shared = isinstance(axes, numbers.Integral) or (len(axes) == 6 and not any(hasattr(a, "__len__") for a in axes))
    if not shared and len(axes) != nframes:
        raise ValueError("%d task-axis entries for %d frames" % (len(axes), nframes))
    per = [one(axes)] * nframes if shared else [one(a) for a in axes]
    return tuple(per[:JACO_OSC_MAX_FRAMES]) + (0,) * (JACO_OSC_MAX_FRAMES - len(per))


class JacoContact(ctypes.Structure):
    """JacoContact of include/jaco_env.h: one record of the contact record (jaco_set_contact_record), 96 bytes."""
    _fields_ = [("dist", ctypes.c_float), ("pos", ctypes.c_float * 3), ("frame", ctypes.c_float * 9), ("force", ctypes.c_float * 6),
                ("geom", ctypes.c_int32 * 2), ("body", ctypes.c_int32 * 2), ("dim", ctypes.c_int32)]


JACO_CONTACT_MAX_CAPACITY = 1024
JACO_FLAG_BAD_SNAPSHOT = 0x40000   # jaco_load_envs: a row of another build / model / task / layout version was refused for this env
CONTACT_WORDS = ctypes.sizeof(JacoContact) // 4        # 24 32-bit words per record
CONTACT_FLOATS = JacoContact.geom.offset // 4          # the first 19 are floats (dist, pos, frame, force), then 5 int32 (geom, body, dim)
assert ctypes.sizeof(JacoContact) == 96 and CONTACT_FLOATS == 19


class JacoConfig(ctypes.Structure):
    _fields_ = [("model_blob", ctypes.c_void_p), ("model_blob_size", ctypes.c_size_t), ("num_envs", ctypes.c_int),
                ("device", ctypes.c_int), ("frame_skip", ctypes.c_int), ("task", ctypes.c_int), ("seed", ctypes.c_uint64)]


# every symbol include/jaco_env.h declares: name -> (restype, argtypes)
_vp, _ci, _cd, _cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_char_p
_ip = ctypes.POINTER(ctypes.c_int)
SYMBOLS = {
    "jaco_create": (_ci, [ctypes.POINTER(JacoConfig), ctypes.POINTER(_vp)]),
    "jaco_destroy": (_ci, [_vp]),
    "jaco_last_error": (_cp, [_vp]),
    "jaco_dims": (_ci, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "jaco_num_envs": (_ci, [_vp]),
    "jaco_set_state": (_ci, [_vp, _vp, _vp, _vp, _vp]),
    "jaco_get_state": (_ci, [_vp, _vp, _vp, _vp, _vp]),
    "jaco_reset_state": (_ci, [_vp, _vp]),
    "jaco_physics_step": (_ci, [_vp, _vp, _ci, _vp]),
    "jaco_get_sensordata": (_ci, [_vp, _vp, _vp]),
    "jaco_get_flags": (_ci, [_vp, _vp, _vp]),
    "jaco_clear_flags": (_ci, [_vp, _vp]),
    "jaco_get_stats": (_ci, [_vp, _vp, _vp]),
    "jaco_set_option": (_ci, [_vp, _cp, _cd]),
    "jaco_reset": (_ci, [_vp, _vp, _vp, _vp]),
    "jaco_placing_hold": (_ci, [_vp, _vp, _ci, _vp]),
    "jaco_grasping_prereach": (_ci, [_vp, _vp, _ci, _vp, _vp]),
    "jaco_step": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_forward": (_ci, [_vp, _vp, _vp]),
    "jaco_take_action": (_ci, [_vp, _vp, _vp]),
    "jaco_terminal_inspection": (_ci, [_vp, _vp, _vp, _vp]),
    "jaco_set_noise": (_ci, [_vp, _vp]),
    "jaco_set_subgoal": (_ci, [_vp, _vp]),
    "jaco_set_init_buffer": (_ci, [_vp, _vp, _ci, _ci, _vp]),
    "jaco_get_task_state": (_ci, [_vp, _vp, _vp]),
    "jaco_set_task_state": (_ci, [_vp, _vp, _vp]),
    "jaco_task_row_floats": (_ci, []),
    "jaco_get_markers": (_ci, [_vp, _vp, _vp]),
    "jaco_get_last_terminal": (_ci, [_vp, _vp, _vp]),
    "jaco_get_terminal_obs": (_ci, [_vp, _vp, _vp]),
    "jaco_set_markers": (_ci, [_vp, _vp, _vp]),
    "jaco_set_frame_skip": (_ci, [_vp, _ci]),
    "jaco_physics_step_debug": (_ci, [_vp, _vp, _ci, _ci, ctypes.POINTER(ctypes.c_float), _ci]),
    "jaco_debug_dump_floats": (_ci, []),
    "jaco_launch_count": (ctypes.c_longlong, [_vp]),
    "jaco_debug_queue_words": (_ci, [_vp, _ip, _ci]),
    "jaco_kernel_time_ms": (_ci, [_vp, ctypes.POINTER(_cd), _ip]),
    "jaco_enable_timing": (_ci, [_vp, _ci]),
    "jaco_step_time_ms": (_ci, [_vp, ctypes.POINTER(_cd)]),
    "jaco_stage_profile": (_ci, [_vp, ctypes.POINTER(ctypes.c_uint64), _ci]),
    "jaco_query": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "jaco_ik": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_osc": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_osc_task": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_joint": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_fd": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_rollout": (_ci, [_vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "jaco_rollout_fb": (_ci, [_vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "jaco_lqr": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp]),
    "jaco_rollout_cost": (_ci, [_vp, _vp, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_rollout_osc": (_ci, [_vp, _vp, _vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "jaco_transition_fd": (_ci, [_vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp]),
    "jaco_cost_quad": (_ci, [_vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jaco_set_contact_record": (_ci, [_vp, _vp, _vp, _ci]),
    "jaco_snapshot_words": (_ci, [_vp]),
    "jaco_save_envs": (_ci, [_vp, _vp, _ci, _vp, _vp]),
    "jaco_load_envs": (_ci, [_vp, _vp, _ci, _vp, _ci, _vp, _vp]),
}

_libs = {}


def load(variant=""):
    """variant "": the default layout (11 fused bodies, 21 dofs in blocks 9 + 6 + 6); "_d12": the build for jaco2_torque.xml and jaco2_curtain_torque_sensor.xml
    (12 hinge dofs in one tree + at most one free object); "_d30": the build for jaco2_dual_torque.xml."""
    if variant not in _libs:
        # torch first: its wheel bundles its own libamdhip64, and the process must run on ONE HIP runtime -- loaded the other way round
        # (this library's /opt/rocm runtime, then torch's) the second runtime finds no device ("no usable HIP device" in jaco_create)
        import torch  # noqa: F401
        path = LIB_PATH if not variant else os.path.join(_HERE, "libjaco_env%s.so" % variant)
        if not os.path.exists(path):
            raise ImportError(
                "mujoco_jaco_amd: %s is missing. Build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback." % path)
        L = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _libs[variant] = L
    return _libs[variant]


def variant_for(blob_bytes):
    """Which build of the library steps this model: the loader of each build rejects models outside its compiled layout."""
    from .modelc import blob as blobmod
    M = blobmod.loads(blob_bytes)
    nv, nb = int(M["nv"][0]), int(M["f_nbody"][0])
    if nv > 21 or nb > 13:
        return "_d30"   # jaco2_dual_torque.xml: two arms + two objects (30 dofs, 20 fused bodies); sim-interface (ctrl) level only
    # the 12-hinge arm (proximal + distal finger joints in the arm's tree), alone (jaco2_torque.xml) or with one free object
    # (jaco2_curtain_torque_sensor.xml: 13 fused bodies, 18 dofs); sim-interface level
    return "_d12" if (nv, nb) in ((12, 12), (18, 13)) else ""


def model_path(name):
    return os.path.join(ASSETS, name + ".jacomdl")
