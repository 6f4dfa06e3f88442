"""The joint-space controller kernel (mujoco_jaco_amd/csrc/joint.h, jaco_joint) under the wavefront emulator (emu_joint of
tests/emu/libjaco_emu{,_d12,_d30}.so, through emu_binding.lib) -- TEST INFRASTRUCTURE ONLY.

Also: the fp64 reference -- the formula of include/jaco_env.h ("joint-space controller") written in numpy on the fp64 oracle's qM,
qfrc_bias and qvel, read as osc_binding.reference reads them --, the input sets of the tests (targets kept off the wrap's and the
saturation's knife edges by construction), the refusal cases and the closed loops.  emu_sim.EmuSim runs BatchedMujoco.joint on the
emulated call (CPU tests of robot_config.BatchedJoint).
"""
import ctypes

import numpy as np

import emu_binding
import ik_binding as ib
import osc_binding as ob
from mujoco_jaco_amd import _lib as product_lib

DEFAULTS = dict(product_lib.JacoJointOptions.DEFAULTS)
GAINS = dict(kp=30.0, kv=12.0)            # the non-default gains of the tests
SAT = dict(kp=30.0, kv=12.0, vmax=0.5)    # saturation level vmax * kv / kp = 0.2 rad
WRAP_MARGIN = 0.05                        # rad: how far a wrapped difference stays from +-pi


def joint(model, qpos, qvel, target_qpos=None, target_qvel=None, qacc=None, ctrl_in=None, alias=False, defaults=False, no_out=False, **options):
    """Emulated jaco_joint: ctrl [B, nu] for fp32 states qpos [B, nq] / qvel [B, nv], target rows [B, nq] / [B, nv] / [B, nv] (None:
    NULL) and ctrl_in [B, nu] (None: NULL).  alias=True: ctrl_out is the ctrl_in buffer.  defaults=True hands a NULL options pointer,
    no_out=True a NULL ctrl_out.  Raises ValueError with the library's message when the call is refused."""
    blob, layout, nu = ob._model_info(model)
    L = emu_binding.lib(layout)
    qpos, qvel = np.ascontiguousarray(qpos, np.float32), np.ascontiguousarray(qvel, np.float32)
    B = qpos.shape[0]
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    row = lambda a, n: None if a is None else np.ascontiguousarray(a, np.float32).reshape(B, n)
    tq, tv, ff = row(target_qpos, qpos.shape[1]), row(target_qvel, qvel.shape[1]), row(qacc, qvel.shape[1])
    cin = None if ctrl_in is None else np.array(ctrl_in, np.float32).reshape(B, nu)   # (a copy: alias=True overwrites it)
    out = cin if alias else np.full((B, nu), np.nan, np.float32)
    opt = product_lib.JacoJointOptions(**options)
    rc = L.emu_joint(blob, len(blob), B, None if defaults else ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), fp(qpos), fp(qvel), fp(tq), fp(tv),
                     fp(ff), fp(cin), None if no_out else fp(out))
    emu_binding.check(L, rc, "emu_joint")
    return out


# ---- the model's joints as the controller sees them
def motor_dofs(model, dof_mask=0):
    """The active set in dof order: hinge dofs with a motor actuator, narrowed by dof_mask."""
    return [d for d in sorted(ob.motor_of(model)) if not dof_mask or (dof_mask >> d) & 1]


def dof_tables(model):
    """({hinge dof: qpos address}, {hinge dof: limited})."""
    M = ib.load_model(model)
    qa, lim = {}, {}
    for j in range(int(M["njnt"][0])):
        if int(M["jnt_type"][j]) == 3:
            qa[int(M["jnt_dofadr"][j])] = int(M["jnt_qposadr"][j])
            lim[int(M["jnt_dofadr"][j])] = bool(M["jnt_limited"][j])
    return qa, lim


def motors(model, dofs):
    m = ob.motor_of(model)
    return [m[d] for d in dofs]


# ---- the fp64 reference
def generate(qM, bias, dq, q, a, qa, wrapped, target_q=None, target_dq=None, qacc=None, kp=50.0, kv=20.0, vmax=0.0):
    """The formula in fp64 for one env: qM [nv, nv], bias / dq [nv], q [nq]; a: the active dofs, qa: their qpos addresses, wrapped: which
    of them are unlimited joints; target_q [nq] / target_dq [nv] / qacc [nv] or None (zeros).  Returns (u [n], e [n], scale, the
    unwrapped differences reduced mod 2 pi [n])."""
    n = len(a)
    diff = np.zeros(n) if target_q is None else np.asarray(target_q, np.float64)[qa] - np.asarray(q, np.float64)[qa]
    red = np.mod(diff + np.pi, 2 * np.pi) - np.pi
    e = np.where(wrapped, red, diff)
    s = 1.0
    if vmax > 0 and kp > 0:
        sat, mx = vmax * kv / kp, np.abs(e).max()
        s = min(1.0, sat / mx) if mx > 0 else 1.0
    acc = (np.zeros(n) if qacc is None else np.asarray(qacc, np.float64)[a]) + kp * s * e
    acc = acc + kv * ((np.zeros(n) if target_dq is None else np.asarray(target_dq, np.float64)[a]) - np.asarray(dq, np.float64)[a])
    return qM[np.ix_(a, a)] @ acc + bias[a], e, s, red


def reference(model, qpos, qvel, target_qpos=None, target_qvel=None, qacc=None, dof_mask=0, kp=50.0, kv=20.0, vmax=0.0):
    """fp64 at the fp32 inputs: {"u" [B, n] (the active dofs in dof order), "e" [B, n], "scale" [B], "red" [B, n], "acts", "wrapped",
    "bias" [B, n] (the oracle's qfrc_bias there)}.  The oracle's quantities as osc_binding.reference takes them: qM, qfrc_bias, qvel."""
    from oracle_binding import Oracle
    o = Oracle(model)
    a = motor_dofs(model, dof_mask)
    qadr, lim = dof_tables(model)
    qa, wrapped = [qadr[d] for d in a], np.array([not lim[d] for d in a])
    B, n = qpos.shape[0], len(a)
    out = dict(u=np.zeros((B, n)), e=np.zeros((B, n)), scale=np.ones(B), red=np.zeros((B, n)), bias=np.zeros((B, n)), acts=a, wrapped=wrapped)
    pick = lambda t, k: None if t is None else np.asarray(t[k], np.float64)
    for k in range(B):
        o.set("qpos", qpos[k].astype(np.float64)); o.set("qvel", qvel[k].astype(np.float64))
        o.forward()
        qM, bias, dq = o.get("qM").reshape(o.nv, o.nv), o.get("qfrc_bias"), o.get("qvel")
        out["u"][k], out["e"][k], out["scale"][k], out["red"][k] = generate(
            qM, bias, dq, qpos[k], a, qa, wrapped, pick(target_qpos, k), pick(target_qvel, k), pick(qacc, k), kp, kv, vmax)
        out["bias"][k] = bias[a]
    return out


def off_the_wrap_edge(ref):
    """True when every unlimited joint's unwrapped difference, reduced mod 2 pi, is at least WRAP_MARGIN away from +-pi."""
    return bool((np.abs(ref["red"][:, ref["wrapped"]]) <= np.pi - WRAP_MARGIN).all())


error = ob.error


# ---- inputs
def targets(model, qpos, spread=1.0, turns=1, seed=13, fill=np.nan):
    """[B, nq] fp32 target rows: q + U(-spread, spread) + 2 pi m (m in -turns .. turns, drawn per entry; unlimited joints only) at the
    qpos addresses of the motor dofs -- so a wrapped difference stays spread < pi - WRAP_MARGIN away from 0 by construction --, `fill`
    (NaN: those words must not be read) everywhere else."""
    assert spread <= np.pi - 2 * WRAP_MARGIN
    rng = np.random.default_rng(seed)
    qadr, lim = dof_tables(model)
    t = np.full(qpos.shape, fill, np.float32)
    for d in motor_dofs(model):
        draw = qpos[:, qadr[d]].astype(np.float64) + rng.uniform(-spread, spread, len(qpos))
        if not lim[d] and turns:
            draw += 2 * np.pi * rng.integers(-turns, turns + 1, len(qpos))
        t[:, qadr[d]] = draw
    return t


def rates(model, B, seed, scale):
    """[B, nv] fp32 rows uniform in +-scale (target velocities, feed-forward accelerations)."""
    nv = int(ib.load_model(model)["nv"][0])
    return np.random.default_rng(seed).uniform(-scale, scale, (B, nv)).astype(np.float32)


def saturation_targets(model, qpos, above, seed=19):
    """[B, nq] fp32 target rows for SAT (level 0.2 rad): every |e_d| <= 0.15 (below: max |e| <= 0.8 sat); above: in addition one drawn dof
    per env at +-(0.3 .. 1.0) (max |e| >= 1.25 sat)."""
    t = targets(model, qpos, spread=0.15, turns=0, seed=seed)
    if above:
        rng = np.random.default_rng(seed + 1)
        qadr, _ = dof_tables(model)
        a = motor_dofs(model)
        for k in range(len(qpos)):
            d = a[int(rng.integers(len(a)))]
            t[k, qadr[d]] = np.float64(qpos[k, qadr[d]]) + rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0)
    return t


# ---- the refusals: one argument set per JACO_EINVAL case of include/jaco_env.h, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"   # dofs 0-5 arm motors, 6-8 finger position servos, 9-20 free joints
REFUSALS = {
    "free_dof": "active dof 9 belongs to a free joint",
    "no_motor": "active dof 6 has no motor actuator",
    "beyond_nv": "dof_mask bit 21 is at or beyond nv = 21",
    "kp_negative": "kp, kv and vmax must be finite and not negative",
    "kv_nan": "kp, kv and vmax must be finite and not negative",
    "vmax_inf": "kp, kv and vmax must be finite and not negative",
    "null_target": "kp > 0 and the target qpos is missing (kp = 0: no position term)",
    "null_out": "the output ctrl is required",
}
EMPTY_MESSAGE = "empty active dof set (the model has no hinge dof with a motor actuator)"


def servo_only_blob(model=REFUSAL_MODEL):
    """The model's blob with every actuator turned into a position servo: the only way to an empty active set (a non-zero dof_mask is
    either refused bit by bit or leaves a dof).  Every shipped model has motors, so the blob is made here."""
    from mujoco_jaco_amd.modelc import blob as blobmod
    import query_binding as qb
    M = blobmod.loads(qb.blob_of(model))
    M["actuator_position"] = np.ones_like(M["actuator_position"])
    return blobmod.dumps(M)


def joint_on_blob(blob, qpos, qvel, layout=""):
    """emu_joint on raw blob bytes, NULL options and targets, kp from the defaults."""
    L = emu_binding.lib(layout)
    qpos, qvel = np.ascontiguousarray(qpos, np.float32), np.ascontiguousarray(qvel, np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out = np.zeros((qpos.shape[0], 9), np.float32)
    rc = L.emu_joint(blob, len(blob), qpos.shape[0], None, fp(qpos), fp(qvel), None, None, None, None, fp(out))
    emu_binding.check(L, rc, "emu_joint")
    return out


def refusal_args(case, B=2):
    """(with_target, no_out, options) of one refused call on REFUSAL_MODEL."""
    opts = {"free_dof": dict(dof_mask=1 << 9), "no_motor": dict(dof_mask=0b1000001), "beyond_nv": dict(dof_mask=(1 << 21) | 1),
            "kp_negative": dict(kp=-1.0), "kv_nan": dict(kv=float("nan")), "vmax_inf": dict(vmax=float("inf"))}.get(case, {})
    return case != "null_target", case == "null_out", opts


# ---- closed loop: 40 x { joint -> send_forces(nsub = 1) } on the arm-only model towards a jaco_ik result row
LOOP_MODEL, LOOP_B, LOOP_STEPS = "jaco2_reaching_torque", 4, 40
# critically damped at 10 rad/s, the approach limited to 0.4 rad/s (saturation level 0.08 rad; every env's largest joint error stays above 1.25 times
# that over the whole loop, asserted in closed_loop_oracle): the demanded torques stay inside the actuators' force ranges (30 / 15 N m), which unlimited gains of this size exceed sixfold,
# and the error shrinks from the first substep on
LOOP_GAINS = dict(kp=100.0, kv=20.0, vmax=0.4)


def loop_inputs():
    """(q0 [4, 9] fp32, hand targets [4, 3] fp32): start poses qpos0 +- 0.5 rad (query_binding.hold_states) and the EE's body origin
    moved 5 cm along a drawn direction (seeds for which all four inverse-kinematics solves converge, in 3-4 iterations)."""
    import query_binding as qb
    q0 = qb.hold_states(LOOP_B, seed=39).astype(np.float32)
    P, _ = ib.oracle_pose(LOOP_MODEL, "EE", np.zeros(3), q0)
    d = np.random.default_rng(40).normal(size=(LOOP_B, 3))
    d *= 0.05 / np.linalg.norm(d, axis=1)[:, None]
    return q0, (P + d).astype(np.float32)


def loop_frame():
    return ib.table_of(LOOP_MODEL).jaco_frame("EE", point=np.zeros(3))


def closed_loop_oracle(q0, target_row, steps=LOOP_STEPS):
    """fp64: the oracle stepped one substep per control tick with generate() on fresh quantities (contacts off).  Returns (final qpos
    [B, 9], the arm's joint error norm before every step and after the last [B, steps + 1])."""
    from oracle_binding import Oracle
    o = Oracle(LOOP_MODEL)
    o.option("disable_contact", 1)
    a = motor_dofs(LOOP_MODEL)
    qadr, lim = dof_tables(LOOP_MODEL)
    qa, wrapped = [qadr[d] for d in a], np.array([not lim[d] for d in a])
    mot = ob.motor_of(LOOP_MODEL)
    out, errs = np.zeros((q0.shape[0], o.nq)), np.zeros((q0.shape[0], steps + 1))
    for k in range(q0.shape[0]):
        o.set("qpos", q0[k].astype(np.float64)); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv))
        c0 = ob.loop_ctrl_row(q0[k:k + 1])[0].astype(np.float64)
        for i in range(steps + 1):
            o.forward()
            u, e, _, _ = generate(o.get("qM").reshape(o.nv, o.nv), o.get("qfrc_bias"), o.get("qvel"), o.get("qpos"), a, qa, wrapped,
                                  target_row[k].astype(np.float64), **LOOP_GAINS)
            errs[k, i] = np.linalg.norm(e)
            assert np.abs(e).max() >= 1.25 * LOOP_GAINS["vmax"] * LOOP_GAINS["kv"] / LOOP_GAINS["kp"]   # off the saturation's knife edge
            if i == steps:
                break
            c = c0.copy()
            for j, d in enumerate(a):
                c[mot[d]] = u[j]
            o.step(c)
        out[k] = o.get("qpos")
    return out, errs


def closed_loop_emu(q0, target_row, steps=LOOP_STEPS):
    """... on the emulated controller and step kernels: final qpos [B, 9] (fp32)."""
    from emu_binding import EmuEnv
    e = EmuEnv(LOOP_MODEL, q0.shape[0])
    e.qpos[:] = q0
    cin = ob.loop_ctrl_row(q0)
    for _ in range(steps):
        e.step(joint(LOOP_MODEL, e.qpos, e.qvel, target_row, ctrl_in=cin, **LOOP_GAINS), nsub=1, disable_contact=True)
    return e.qpos.copy()


# ---- the cases, shared by the CPU tier (run = the emulated call) and the GPU tier (run = BatchedMujoco.joint through numpy):
# run(model, qpos, qvel, target_qpos, target_qvel, qacc, ctrl_in, **options) -> ctrl [B, nu].  Each returns what it measured; the
# caller prints it and holds it to its bound.
MODEL, B = "jaco2_curtain_torque", 67


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_shared = {}


def regular_inputs():
    """Case 1's inputs and fp64 references (default and non-default gains), computed once per process."""
    if not _shared:
        q, v = ob.states(MODEL, B)
        t, tv, ff = targets(MODEL, q), rates(MODEL, B, 14, 0.5), rates(MODEL, B, 15, 2.0)
        ref = reference(MODEL, q, v, t, tv, ff)
        assert off_the_wrap_edge(ref) and np.abs(ref["e"]).max() > 0.9
        _shared.update(q=q, v=v, t=t, tv=tv, ff=ff, ref=ref, ref_gains=reference(MODEL, q, v, t, tv, ff, **GAINS), mot=motors(MODEL, ref["acts"]))
    return _shared


def case_all_terms(run):
    g = regular_inputs()
    u = run(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], None)
    ug = run(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], None, **GAINS)
    assert (bits(u[:, 6:]) == 0).all()   # NULL ctrl_in: the words outside the active motors are zeros
    assert np.abs(g["ref"]["u"] - g["ref_gains"]["u"]).max() > 1.0   # (the gains matter)
    return max(error(u[:, g["mot"]], g["ref"]["u"]).max(), error(ug[:, g["mot"]], g["ref_gains"]["u"]).max())


def case_wrapping(run):
    """Unlimited joints: a target shifted by 2 pi k gives the unshifted answer, and a target across +-pi is reached the short way."""
    g = regular_inputs()
    qadr, lim = dof_tables(MODEL)
    t0 = targets(MODEL, g["q"], turns=0)
    ref = reference(MODEL, g["q"], g["v"], t0)
    assert off_the_wrap_edge(ref)
    worst = error(run(MODEL, g["q"], g["v"], t0, None, None, None)[:, g["mot"]], ref["u"]).max()
    for k in (-2, -1, 1, 2):
        t = t0.copy()
        for d in ref["acts"]:
            if not lim[d]:
                t[:, qadr[d]] = t0[:, qadr[d]].astype(np.float64) + 2 * np.pi * k
        assert off_the_wrap_edge(reference(MODEL, g["q"][:4], g["v"][:4], t[:4]))
        worst = max(worst, error(run(MODEL, g["q"], g["v"], t, None, None, None)[:, g["mot"]], ref["u"]).max())
    # across +-pi: joint 0 at 3.0, target -3.0: the short way is +0.283, not -6
    q, v = g["q"][:4].copy(), np.zeros_like(g["v"][:4])
    q[:, 0] = 3.0
    t = q.copy(); t[:, 0] = -3.0
    r = reference(MODEL, q, v, t)
    assert off_the_wrap_edge(r) and np.allclose(r["e"][:, 0], 2 * np.pi - 6.0, atol=1e-6) and (r["e"][:, 1:] == 0).all()
    worst = max(worst, error(run(MODEL, q, v, t, None, None, None)[:, g["mot"]], r["u"]).max())
    return worst


def case_limited_joint_is_not_wrapped(run):
    """Joint 2 (limited, range 0.33 .. 5.95) at 0.9 rad, target 5.4 rad: the plain difference is +4.5, the wrapped one -1.78."""
    g = regular_inputs()
    q, v = g["q"][:4].copy(), np.zeros_like(g["v"][:4])
    q[:, 2] = 0.9
    t = q.copy(); t[:, 2] = 5.4
    r = reference(MODEL, q, v, t)
    assert np.allclose(r["e"][:, 2], 4.5, atol=1e-6) and np.allclose(r["red"][:, 2], 4.5 - 2 * np.pi, atol=1e-6) and not r["wrapped"][2]
    u = run(MODEL, q, v, t, None, None, None)[:, g["mot"]]
    wrapped_u = r["u"] - 50.0 * 2 * np.pi * np.array([reference_column(MODEL, q[k], 2) for k in range(4)])   # what wrapping would give
    assert error(u, wrapped_u).min() > 1.0   # (far from the wrapped answer on every env)
    return error(u, r["u"]).max()


def reference_column(model, q, d):
    """fp64 column d of M[A, A] at q (the oracle's qM)."""
    from oracle_binding import Oracle
    o = Oracle(model)
    o.set("qpos", q.astype(np.float64)); o.set("qvel", np.zeros(o.nv))
    o.forward()
    a = motor_dofs(model)
    return o.get("qM").reshape(o.nv, o.nv)[np.ix_(a, a)][:, a.index(d)]


def case_saturation(run):
    """vmax below and above saturation; above it the position term is the unsaturated one times sat / max |e|, on every dof alike.
    Returns (the largest error of the five answers, the identity's residual on the kernel's answers [B, n], its slack per unit of
    bound [B, n]): the caller holds residual <= bound * slack."""
    g = regular_inputs()
    sat = SAT["vmax"] * SAT["kv"] / SAT["kp"]
    worst = 0.0
    for above in (False, True):
        t = saturation_targets(MODEL, g["q"], above)
        r = reference(MODEL, g["q"], g["v"], t, g["tv"], None, **SAT)
        mx = np.abs(r["e"]).max(axis=1)
        assert (mx >= 1.25 * sat).all() if above else (mx <= 0.8 * sat).all(), mx
        assert (r["scale"] < 1).all() if above else (r["scale"] == 1).all()
        u = run(MODEL, g["q"], g["v"], t, g["tv"], None, None, **SAT)[:, g["mot"]]
        worst = max(worst, error(u, r["u"]).max())
        if above:
            free = reference(MODEL, g["q"], g["v"], t, g["tv"], None, **GAINS)          # no vmax
            none = reference(MODEL, g["q"], g["v"], t, g["tv"], None, kp=0.0, kv=GAINS["kv"])   # no position term
            f = (sat / mx)[:, None]
            assert np.allclose(r["u"] - none["u"], f * (free["u"] - none["u"]), rtol=1e-9, atol=1e-9)   # the identity, on the fp64 side
            uf = run(MODEL, g["q"], g["v"], t, g["tv"], None, None, **GAINS)[:, g["mot"]]
            un = run(MODEL, g["q"], g["v"], t, g["tv"], None, None, kp=0.0, kv=GAINS["kv"])[:, g["mot"]]
            worst = max(worst, error(uf, free["u"]).max(), error(un, none["u"]).max())
            # each of the three answers is within bound * (1 + |its reference|) of a reference for which the identity is exact
            slack = (1 + np.abs(r["u"])) + (1 + np.abs(none["u"])) + f * ((1 + np.abs(free["u"])) + (1 + np.abs(none["u"])))
            resid = np.abs((u.astype(np.float64) - un) - f * (uf.astype(np.float64) - un))
    return worst, resid, slack


def case_modes(run, query_bias):
    """Inverse dynamics (kp = kv = 0 with qacc) against the reference; bias compensation equal to jaco_query's qfrc_bias as floats.
    query_bias(model, q, v) -> [B, nv] fp32."""
    g = regular_inputs()
    r = reference(MODEL, g["q"], g["v"], None, None, g["ff"], kp=0.0, kv=0.0)
    u = run(MODEL, g["q"], g["v"], None, None, g["ff"], None, kp=0.0, kv=0.0)
    uq = run(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], None, kp=0.0, kv=0.0)   # (targets given, gains zero: the same bits)
    assert (bits(u) == bits(uq)).all()
    b = run(MODEL, g["q"], g["v"], None, None, None, None, kp=0.0, kv=0.0)
    qb_ = query_bias(MODEL, g["q"], g["v"])
    assert (b[:, g["mot"]] == qb_[:, r["acts"]]).all() and (bits(b[:, 6:]) == 0).all()
    assert error(b[:, g["mot"]], r["bias"]).max() < 1e-5   # (and jaco_query's bias is the oracle's: test_query_emu / test_gpu_query)
    return error(u[:, g["mot"]], r["u"]).max()


MASKS = (0b000100, 0b001111, 0b101001)   # one dof, dofs 0-3, a non-contiguous set


def case_masks_and_pass_through(run, run_alias):
    """dof_mask subsets against the reference; a random ctrl_in comes back bit for bit on every other word (finger commands, special
    values); ctrl_out = ctrl_in gives the same bits.  run_alias: run with ctrl_out aliasing ctrl_in."""
    g = regular_inputs()
    cin = np.random.default_rng(4).normal(size=(B, 9)).astype(np.float32)
    w = bits(cin)
    w[:, 6], w[:, 7], w[:, 8], w[:3, :6] = 0x7fc12345, 0x80000000, 0x00000123, 0xffc00001   # a NaN with a payload, -0, a denormal
    worst = 0.0
    for mask in (0,) + MASKS:
        r = reference(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], dof_mask=mask)
        mot = motors(MODEL, r["acts"])
        other = [a for a in range(9) if a not in mot]
        u = run(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], cin, dof_mask=mask)
        assert (bits(u[:, other]) == w[:, other]).all(), mask
        assert (bits(run_alias(MODEL, g["q"], g["v"], g["t"], g["tv"], g["ff"], cin, dof_mask=mask)) == bits(u)).all(), mask
        worst = max(worst, error(u[:, mot], r["u"]).max())
    return worst


def case_two_arms(run):
    """jaco2_dual_torque, B = 9: all twelve motor dofs in one call; then one arm's six with the other arm's words untouched."""
    model, n = "jaco2_dual_torque", 9
    q, v = ob.states(model, n)
    t, tv, ff = targets(model, q), rates(model, n, 14, 0.5), rates(model, n, 15, 2.0)
    r = reference(model, q, v, t, tv, ff)
    assert len(r["acts"]) == 12 and off_the_wrap_edge(r)
    cin = np.random.default_rng(6).normal(size=(n, 18)).astype(np.float32)
    u = run(model, q, v, t, tv, ff, cin)
    mot = motors(model, r["acts"])
    assert (bits(u[:, [a for a in range(18) if a not in mot]]) == bits(cin[:, [a for a in range(18) if a not in mot]])).all()
    worst = error(u[:, mot], r["u"]).max()
    arm1 = r["acts"][:6]
    r1 = reference(model, q, v, t, tv, ff, dof_mask=sum(1 << d for d in arm1))
    u1 = run(model, q, v, t, tv, ff, cin, dof_mask=sum(1 << d for d in arm1))
    m1 = motors(model, arm1)
    rest = [a for a in range(18) if a not in m1]
    assert (bits(u1[:, rest]) == bits(cin[:, rest])).all()
    # (the arms are separate trees: M is block diagonal across them, so one arm's torques are the same in both calls)
    assert np.abs(r1["u"] - r["u"][:, :6]).max() < 1e-12
    return max(worst, error(u1[:, m1], r1["u"]).max())


def case_other_layout(run, model="jaco2_curtain_torque_old", n=9):
    q, v = ob.states(model, n)
    t, tv, ff = targets(model, q), rates(model, n, 14, 0.5), rates(model, n, 15, 2.0)
    r = reference(model, q, v, t, tv, ff)
    assert off_the_wrap_edge(r)
    u = run(model, q, v, t, tv, ff, None)
    return error(u[:, motors(model, r["acts"])], r["u"]).max()
