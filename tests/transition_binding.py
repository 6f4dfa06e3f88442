"""The transition-Jacobian kernel (mujoco_jaco_amd/csrc/transition.h, jaco_transition_fd) under the wavefront emulator (emu_transition_fd
of tests/emu_transition/libjaco_emu_transition{,_d12,_d30}.so) -- TEST INFRASTRUCTURE ONLY.

Also: the inputs (rollout_binding.inputs on one knot), the dof / ctrl-word sets, the references -- jaco_rollout(nknots = 1) from the
explicitly perturbed fp32 rows, and central differences of the fp64 oracle's contact-free rollout on the same actually-rounded perturbed
inputs, both in the increment form --, the cases shared by the CPU and the GPU tier, the refusals, and EmuTransitionSim: emu_sim.EmuSim plus
the one launch method `_transition`, so that BatchedMujoco.transition_fd and robot_config.linearize_rollout run on the emulated call.

A tier hands the cases
  run(model, qpos [n, nq], qvel [n, nv], ctrl [n, nu] or None, dofs, acts, want=OUTS, hold=1, centered=1, groups=0, handle=None, **eps)
      -> {output: array}      (every output handed in sentinel-filled)
  roll(model, qpos, qvel, ctrl [n, nu], hold) -> {"qpos" [n, nq], "qvel" [n, nv], "status" [n]}: jaco_rollout(nknots = 1, hold, final_only)
"""
import ctypes
import os
import subprocess

import numpy as np

import emu_binding
import fd_binding as fb
import ik_binding as ib
import osc_binding as ob
import rollout_binding as rb
from emu_sim import EmuSim, _np, _tensors
from fd_binding import bits, merr
from mujoco_jaco_amd import _lib as product_lib
from mujoco_jaco_amd.physics import BatchedMujoco

OUTS = ("A", "B", "next_qpos", "next_qvel", "status")
DEFAULTS = dict(product_lib.JacoTransitionOptions.DEFAULTS)
EMU_DIR = os.path.join(emu_binding.ROOT, "tests", "emu_transition")
_libs = {}


def lib(layout=""):
    """The emulator build that holds emu_transition_fd, per layout (built on first use, as emu_binding.lib builds its own)."""
    if layout not in _libs:
        name = "libjaco_emu_transition%s.so" % layout
        subprocess.check_call(["make", "-s", "-C", EMU_DIR, name])
        L = ctypes.CDLL(os.path.join(EMU_DIR, name))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.emu_transition_fd.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, ci, vp, vp, vp, vp, ci, vp, vp]
        L.emu_last_error.restype = ctypes.c_char_p
        _libs[layout] = L
    return _libs[layout]


def shapes(n, nq, nv, nd, na):
    return {"A": (n, 2 * nd, 2 * nd), "B": (n, 2 * nd, na), "next_qpos": (n, nq), "next_qvel": (n, nv), "status": (n,)}


def options(dofs, acts, patch=None, **fields):
    """The options record of a call; patch: fields set by hand after the record is built (counts the constructor would not let through)."""
    opt = product_lib.JacoTransitionOptions(dofs=dofs, acts=acts, **fields)
    for k, x in (patch or {}).items():
        setattr(opt, k, x)
    return opt


def transition(model, qpos, qvel, ctrl, dofs, acts, want=OUTS, hold=1, centered=1, groups=0, handle=None, n=None, no_opt=False, no_out=False, patch=None, **eps):
    """Emulated jaco_transition_fd: {output: array} in the C ABI's layout.  qpos / qvel None: the handle's state, handle = (qpos
    [num_envs, nq], qvel [num_envs, nv]); n: override what the arrays say (refusals); no_opt / no_out hand NULL pointers.  Raises
    ValueError with the library's message when the call is refused, with the outputs it was handed in .outputs."""
    blob, layout, nu = ob._model_info(model)
    L = lib(layout)
    M = ib.load_model(model)
    nq, nv = int(M["nq"][0]), int(M["nv"][0])
    H, p = rb.HOST, rb.HOST.ptr
    q, v, c = H.f32(qpos), H.f32(qvel), H.f32(ctrl)
    hq, hv = (None, None) if handle is None else (H.f32(handle[0]), H.f32(handle[1]))
    rows = next((a.shape[0] for a in (q, v, c) if a is not None), 0 if hq is None else hq.shape[0])   # (the outputs' rows: what the arrays say, whatever n a refusal case hands)
    n = rows if n is None else n
    sh = shapes(rows, nq, nv, len(dofs), len(acts))
    res = {k: H.blank(sh[k], k == "status") for k in want}
    out = product_lib.JacoTransitionOut(*[p(res.get(k)) for k in OUTS])
    opt = options(dofs, acts, patch, hold=hold, centered=centered, groups=groups, **eps)
    rc = L.emu_transition_fd(blob, len(blob), rb.ref(opt, no_opt), n, p(q), p(v), p(c), rb.ref(out, no_out), 0 if hq is None else hq.shape[0], p(hq), p(hv))
    return rb.checked(L, rc, "emu_transition_fd", res)


def emu_roll(model, qpos, qvel, ctrl, hold):
    """jaco_rollout(nknots = 1, hold, final_only) on the emulator, one knot row squeezed."""
    r = rb.rollout(model, np.asarray(ctrl, np.float32)[:, None], qpos, qvel, want=("qpos", "qvel", "status"), hold=hold, final_only=1)
    return {"qpos": r["qpos"][:, 0], "qvel": r["qvel"][:, 0], "status": r["status"]}


class EmuTransitionSim(EmuSim):
    """emu_sim.EmuSim with jaco_transition_fd: the product's transition_fd over the emulated launch."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches["jaco_transition_fd"] = 0

    def _transition(self, ctrl, qpos, qvel, n, want, **options):
        self.launches["jaco_transition_fd"] += 1
        o = dict(options)
        return _tensors(transition(self.model, _np(qpos), _np(qvel), _np(ctrl), o.pop("dofs"), o.pop("acts"), tuple(want), handle=self._state(None, None), n=n, **o))

    transition_fd = BatchedMujoco.transition_fd


# ---- inputs and sets
MODELS = (rb.MODEL,) + rb.SMALL
N, HOLDS = 9, (3, 1)
SMALL_DOFS = (0, 3, 5)


def inputs(model):
    """(qpos [9, nq], qvel [9, nv], ctrl [9, nu]) fp32: rollout_binding.inputs on one knot -- pairs 0, 3, 6 with a limit row from the
    start, pairs 1, 4, 7 at least 0.15 rad inside every limit, pairs 2, 5, 8 as drawn."""
    q, v, c = rb.inputs(model, N, 1)
    return q, v, np.ascontiguousarray(c[:, 0])


def small_set(model):
    """(dofs, acts): hinge dofs 0, 3, 5 and the motor words of dofs 0 and 3."""
    T = fb.tables(model)
    motor = {int(d): a for a, d in enumerate(T["dof"]) if not T["position"][a]}
    return list(SMALL_DOFS), [motor[0], motor[3]]


def full_set(model):
    """(dofs, acts): the arm's full set -- every motor-driven hinge dof and its motor word (both arms of the two-arm model).  The
    servo-driven finger joints stay out: kp eps_ctrl = 20 * 2^-6 = 0.31 is more than the whole forcerange of +-0.3, and kp eps_qpos =
    0.078 takes a perturbed evaluation inside the 1.25 kp eps_qpos that fd_binding.off_the_knife_edges asks of every evaluation: a
    finger column straddles or grazes the force clamp from any state, where no finite difference has a reference."""
    T = fb.tables(model)
    acts = [a for a in range(len(T["dof"])) if not T["position"][a]]
    return [int(T["dof"][a]) for a in acts], acts


def every_set(model):
    """(dofs, acts): every hinge dof (at most 18) and every ctrl word, the servos' included -- for the cases that need no fp64 reference
    (bit for bit, and the formula recomputed from jaco_rollout): nx = 36 lanes and 54 columns on the two-arm model."""
    T = fb.tables(model)
    return [int(d) for d in T["hinge"]][:product_lib.JACO_ROLLOUT_FB_MAX_DOFS], list(range(len(T["dof"])))


EVERY_MODELS = (rb.MODEL, "jaco2_dual_torque")


def same(a, b, keys=None):
    for k in (keys or a):
        assert a[k].shape == b[k].shape and (bits(a[k]) == bits(b[k])).all(), k


def columns(model, dofs, acts):
    """Per column: (array index: 0 qpos / 1 qvel / 2 ctrl, word, eps name)."""
    T = fb.tables(model)
    return [(0, T["hinge_qadr"][d], "eps_qpos") for d in dofs] + [(1, d, "eps_qvel") for d in dofs] + [(2, a, "eps_ctrl") for a in acts]


def x_of(model, dofs, q, v):
    T = fb.tables(model)
    return np.concatenate([q[..., [T["hinge_qadr"][d] for d in dofs]], v[..., list(dofs)]], -1)


# ---- the cases: bit for bit
def case_nominal(run, roll, model, hold):
    """1: next_qpos / next_qvel / status = jaco_rollout(nknots = 1, hold, final_only) from the same rows, limit rows included."""
    q, v, c = inputs(model)
    dofs, acts = small_set(model)
    r = run(model, q, v, c, dofs, acts, want=("next_qpos", "next_qvel", "status"), hold=hold)
    ref = roll(model, q, v, c, hold)
    same(r, {"next_qpos": ref["qpos"], "next_qvel": ref["qvel"], "status": ref["status"]})
    assert not (bits(r["next_qpos"]) == bits(np.float32(rb.SENTINEL))).all(1).any()


def case_invariance(run, model, hold=HOLDS[0], centered=1, sets=small_set):
    """2 - 5: groups 1, 2, ncol; each output alone and A + B; pair i alone; two identical calls."""
    q, v, c = inputs(model)
    dofs, acts = sets(model)
    ncol = 2 * len(dofs) + len(acts)
    full = run(model, q, v, c, dofs, acts, hold=hold, centered=centered, groups=1)
    for k in ("A", "B"):
        assert np.isfinite(full[k]).all() and not (bits(full[k]) == bits(np.float32(rb.SENTINEL))).any(), k   # every entry written
    same(full, run(model, q, v, c, dofs, acts, hold=hold, centered=centered, groups=1))
    for groups in (2, ncol, 0):
        same(full, run(model, q, v, c, dofs, acts, hold=hold, centered=centered, groups=groups))
    for want in [(k,) for k in OUTS] + [("A", "B"), ("B", "status")]:
        r = run(model, q, v, c, dofs, acts, want=want, hold=hold, centered=centered, groups=2)
        assert set(r) == set(want)
        same(r, full, want)
    i = 3   # (a pair with a limit row)
    one = run(model, q[i:i + 1], v[i:i + 1], c[i:i + 1], dofs, acts, hold=hold, centered=centered)
    same(one, {k: x[i:i + 1] for k, x in full.items()})
    alone = run(model, q, v, c, dofs, acts, want=("status",), hold=hold, centered=centered)   # (no column asked for: the library's groups = 1)
    same(alone, full, ("status",))
    return full


def case_subset_of_full(run, model, hold=HOLDS[0]):
    """6: entries (r, c) on the dof set [0, 3, 5] equal the corresponding entries on the full set."""
    q, v, c = inputs(model)
    dofs, acts = small_set(model)
    fd_, fa = full_set(model)
    small = run(model, q, v, c, dofs, acts, want=("A", "B"), hold=hold)
    full = run(model, q, v, c, fd_, fa, want=("A", "B"), hold=hold)
    nf = len(fd_)
    ix = [fd_.index(d) for d in dofs] + [nf + fd_.index(d) for d in dofs]
    assert (bits(small["A"]) == bits(full["A"][:, ix][:, :, ix])).all()
    assert (bits(small["B"]) == bits(full["B"][:, ix][:, :, [fa.index(a) for a in acts]])).all()
    ed, ea = every_set(model)
    every = run(model, q, v, c, ed, ea, want=("A", "B"), hold=hold)
    ne = len(ed)
    ix = [ed.index(d) for d in dofs] + [ne + ed.index(d) for d in dofs]
    assert (bits(small["A"]) == bits(every["A"][:, ix][:, :, ix])).all()
    assert (bits(small["B"]) == bits(every["B"][:, ix][:, :, [ea.index(a) for a in acts]])).all()
    return full


def case_clamped_ctrl(run, model=rb.MODEL, hold=1):
    """7: a ctrl word more than eps_ctrl beyond its limited ctrlrange: a B column of exactly 0.0f; the others' columns are not zero."""
    q, v, c = inputs(model)
    T = fb.tables(model)
    dofs, acts = small_set(model)
    servo = int(np.flatnonzero(T["position"] & T["ctrllimited"])[0])
    acts = acts + [servo]
    c = c.copy()
    c[:, servo] = T["ctrlrange"][servo, 1] + 2 * DEFAULTS["eps_ctrl"]
    c[::2, servo] = T["ctrlrange"][servo, 0] - 2 * DEFAULTS["eps_ctrl"]
    r = run(model, q, v, c, dofs, acts, want=("B",), hold=hold)
    assert (bits(r["B"][:, :, 2]) == 0).all()
    assert (np.abs(r["B"][:, :, :2]).max((0, 1)) > 0).all()


# ---- the formula, recomputed from jaco_rollout on the explicitly perturbed rows
_perturbed = {}


def perturbed_rollouts(roll, tier, model, dofs, acts, hold):
    """jaco_rollout(nknots = 1, hold) from x0 + eps and x0 - eps formed in float32 numpy, every pair and column, in ONE call of the
    tier's `roll`: (c(+), c(-) [n, ncol] fp32, x'(+), x'(-) [n, ncol, nx] fp32 high words, start words xs(+), xs(-) [n, ncol, nx] fp32).
    Computed once per (tier, model, set, hold)."""
    key = (tier, model, tuple(dofs), tuple(acts), hold)
    if key not in _perturbed:
        q, v, c = inputs(model)
        cols = columns(model, dofs, acts)
        n, ncol = len(q), len(cols)
        rows = [np.repeat(a[:, None, None], ncol, 1).repeat(2, 2).copy() for a in (q, v, c)]   # [n, ncol, 2, width]
        cpm = np.zeros((n, ncol, 2), np.float32)
        for j, (which, word, eps) in enumerate(cols):
            e = np.float32(DEFAULTS[eps])
            rows[which][:, j, 0, word] = rows[which][:, j, 0, word] + e
            rows[which][:, j, 1, word] = rows[which][:, j, 1, word] - e
            cpm[:, j] = rows[which][:, j, :, word]
        flat = [a.reshape(n * ncol * 2, -1) for a in rows]
        r = roll(model, flat[0], flat[1], flat[2], hold)
        xe = x_of(model, dofs, r["qpos"], r["qvel"]).reshape(n, ncol, 2, -1)
        xs = x_of(model, dofs, flat[0], flat[1]).reshape(n, ncol, 2, -1)
        _perturbed[key] = (cpm[..., 0], cpm[..., 1], xe[:, :, 0], xe[:, :, 1], xs[:, :, 0], xs[:, :, 1])
    return _perturbed[key]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def high_word_columns(P, nx):
    """[A | B] [n, nx, ncol] in fp64 from the high words jaco_rollout returns, in the increment form: I + (D(+) - D(-)) / (c(+) - c(-))."""
    cp, cm, xp, xm, sp, sm = [a.astype(np.float64) for a in P]
    D = ((xp - sp) - (xm - sm)) / (cp - cm)[:, :, None]          # [n, ncol, nx]
    J = np.transpose(D, (0, 2, 1)).copy()
    J[:, np.arange(nx), np.arange(nx)] += 1.0
    return J


def case_formula(run, roll, tier, model, dofs, acts, hold, compensated=True):
    """The kernel's A and B against the columns formed in fp64 from jaco_rollout's high words at the explicitly perturbed rows.  The
    two may differ by the low words, at most half a spacing of x' per side, and by the device reciprocal and one product:
        |kernel - fp64| <= (ulp32(x'(+)) + ulp32(x'(-))) / 2 / |c(+) - c(-)| + 4 * 2^-23 * |entry|      per entry
    (the 4: 2.5 ulp for the build's divide, a rounding each for the difference and the product; derived, not measured); with
    compensated = 0 the first term drops.  Nothing is allowed for the subtraction x'.hi - xs: the kernel keeps its rounding error in
    the increment's second word.  Returns the largest ratio of a difference to its bound."""
    q, v, c = inputs(model)
    r = run(model, q, v, c, dofs, acts, want=("A", "B"), hold=hold)
    P = perturbed_rollouts(roll, tier, model, dofs, acts, hold)
    nx = 2 * len(dofs)
    ref = high_word_columns(P, nx)
    got = np.concatenate([r["A"], r["B"]], 2).astype(np.float64)
    sides = (ulp32(P[2]) + ulp32(P[3])) / 2 if compensated else np.zeros(P[2].shape)
    low = sides / np.abs(P[0].astype(np.float64) - P[1].astype(np.float64))[:, :, None]
    bound = np.transpose(low, (0, 2, 1)) + 4 * 2.0 ** -23 * np.abs(ref)
    assert np.isfinite(got).all()
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    worst = float(np.where(np.abs(got - ref) == 0, 0.0, ratio).max())
    print("MEASURE formula %s hold %d (%d dofs, compensated %d): largest |kernel - fp64 of the high words| / bound %.3g" % (model, hold, len(dofs), compensated, worst))
    assert worst <= 1.0, worst
    return worst


# ---- against fp64
_oracle = {}


def oracle_columns(model, dofs, acts, hold):
    """Central differences of rollout_binding.oracle_rollout(model, q, v, ctrl[:, None], hold) with the kernel's own eps on the same
    actually-rounded perturbed inputs, in the increment form in fp64: ([A | B] [n, nx, ncol], kept [n], limited [n]).  A pair is kept if
    the oracle's set of limit rows (nefc and which joints, per substep) is the same in the nominal and in every perturbed evaluation and
    fd_binding.off_the_knife_edges holds for all of them; limited: the nominal has a limit row at some substep."""
    key = (model, tuple(dofs), tuple(acts), hold)
    if key not in _oracle:
        q, v, c = inputs(model)
        cols = columns(model, dofs, acts)
        n, ncol, nx = len(q), len(cols), 2 * len(dofs)
        adr, lo, hi = rb.limit_table(model)

        def evaluate(q_, v_, c_):
            r = rb.oracle_rollout(model, q_, v_, c_[:, None], hold)
            ql = r["before"][:, :, adr]
            rows = np.concatenate([ql < lo, ql > hi], 2)                          # [n, hold, 2 nlim]: which limit rows, per substep
            assert (rows.sum(2) == r["nefc"]).all()
            edge = np.array([all(fb.off_the_knife_edges(model, r["before"][i:i + 1, s], c_[i:i + 1]) for s in range(hold)) for i in range(len(q_))])
            return x_of(model, dofs, r["qpos"][:, 0], r["qvel"][:, 0]), rows, edge
        _, rows0, kept = evaluate(q, v, c)
        J = np.zeros((n, nx, ncol))
        for j, (which, word, eps) in enumerate(cols):
            e = np.float32(DEFAULTS[eps])
            side = []
            for sgn in (1, -1):
                a = [q.copy(), v.copy(), c.copy()]
                a[which][:, word] = a[which][:, word] + e if sgn > 0 else a[which][:, word] - e
                xe, rows, edge = evaluate(*a)
                kept = kept & edge & (rows == rows0).all((1, 2))
                side.append((a[which][:, word].astype(np.float64), xe - x_of(model, dofs, a[0], a[1]).astype(np.float64)))
            J[:, :, j] = (side[0][1] - side[1][1]) / (side[0][0] - side[1][0])[:, None]
        J[:, np.arange(nx), np.arange(nx)] += 1.0
        limited = rows0.any((1, 2))
        # the conditions the inputs must meet, on the fp64 side
        assert (~kept).mean() <= 1 / 3 + 1e-9, (model, kept)
        assert (limited & kept).sum() >= kept.sum() / 5 and (~limited & kept).sum() >= kept.sum() / 5, (model, kept, limited)
        _oracle[key] = (J, kept, limited)
    return _oracle[key]


def case_fp64(run, roll, tier, model, dofs, acts, hold):
    """A and B against the fp64 central differences, on the kept pairs: (merr over A, merr over B, the position rows' error of the
    kernel, the same rows' error formed from jaco_rollout's high words alone) -- the last two on the kept pairs without a limit row,
    where the increment form must leave at most a quarter of the error."""
    q, v, c = inputs(model)
    J, kept, limited = oracle_columns(model, dofs, acts, hold)
    r = run(model, q, v, c, dofs, acts, want=("A", "B"), hold=hold)
    nd, nx = len(dofs), 2 * len(dofs)
    ea, eb = merr(r["A"][kept], J[kept][:, :, :nx]), merr(r["B"][kept], J[kept][:, :, nx:])
    free = kept & ~limited
    P = perturbed_rollouts(roll, tier, model, dofs, acts, hold)
    cp, cm, xp, xm = [a.astype(np.float64) for a in P[:4]]
    naive = np.transpose((xp - xm) / (cp - cm)[:, :, None], (0, 2, 1))[:, :nd, :nx]      # the difference of the end states' high words
    mine = merr(r["A"][free][:, :nd], J[free][:, :nd, :nx])
    theirs = merr(naive[free], J[free][:, :nd, :nx])
    print("MEASURE fp64 %s hold %d (%d dofs): A %.3g B %.3g over %d kept pairs (%d with a limit row); position rows of A on the %d without: "
          "increment form %.3g, end states' high words %.3g" % (model, hold, nd, ea, eb, kept.sum(), (kept & limited).sum(), free.sum(), mine, theirs))
    return ea, eb, mine, theirs


# ---- against the existing path (robot_config.linearize over jaco_fd), hold = 1, no limit row
def case_linearize(make_sim):
    """A, B of transition_fd against robot_config.linearize's A, Bm on fd_binding.stepper_inputs(), the pairs the oracle reports with
    nefc == 0: independent code, the same derivative.  Returns (merr over A, merr over B)."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    q, v, c = fb.stepper_inputs()
    assert fb.off_the_knife_edges(fb.STEP_MODEL, q, c)
    _, _, nefc = fb.oracle_substep(fb.STEP_MODEL, q, v, c)
    ok = nefc == 0
    assert ok.mean() >= 0.9
    sim = make_sim(fb.STEP_MODEL, q, v)
    cfg = BatchedMujocoConfig(sim)
    ctrl = torch.as_tensor(c, device=sim.device)
    A, Bm, _ = [t.cpu().numpy() for t in cfg.linearize(ctrl=ctrl)]
    dofs, _, acts = cfg._joint_subset(None, "test")
    r = sim.transition_fd(ctrl, dofs=dofs, acts=acts, hold=1)
    return merr(r["A"].cpu().numpy()[ok], A[ok]), merr(r["B"].cpu().numpy()[ok], Bm[ok])


# ---- the refusals: one argument set per message of jaco_transition_resolve, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"   # dofs 0-8 hinges, 9-20 free joints; 9 ctrl words
REFUSAL_N, REFUSAL_ENVS = 4, 5
REFUSALS = {
    "null_options": "the options are required",
    "hold_0": "hold 0 outside [1, 1024]",
    "hold_1025": "hold 1025 outside [1, 1024]",
    "centered_2": "centered must be 0 or 1",
    "n_negative": "n -1 is negative",
    "null_out": "the output record is required",
    "no_outputs": "at least one of the outputs A, B, next_qpos, next_qvel and status is required",
    "qpos_alone": "qpos and qvel are given together or not at all",
    "qvel_alone": "qpos and qvel are given together or not at all",
    "n_not_num_envs": "n 4 with the handle's state of 5 envs",
    "eps_qpos_zero": "eps_qpos, eps_qvel and eps_ctrl must be finite and positive",
    "eps_qvel_nan": "eps_qpos, eps_qvel and eps_ctrl must be finite and positive",
    "eps_ctrl_inf": "eps_qpos, eps_qvel and eps_ctrl must be finite and positive",
    "eps_ctrl_negative": "eps_qpos, eps_qvel and eps_ctrl must be finite and positive",
    "no_dofs": "ndofs 0 outside [1, 18]",
    "dof_beyond_nv": "dof 21 outside [0, 21)",
    "dof_free": "dof 9 belongs to a free joint",
    "dof_twice": "dof 3 is listed twice",
    "act_beyond_nu": "ctrl word 9 outside [0, 9)",
    "act_negative": "ctrl word -1 outside [0, 9)",
    "act_twice": "ctrl word 2 is listed twice",
    "B_without_acts": "B needs at least one ctrl word",
    "ndofs_19": "ndofs 19 outside [1, 18]",
    "nacts_19": "nacts 19 outside [0, 18]",
    "grid_too_large": "n 2147483647 x groups 8 is beyond the largest grid",
    "groups_negative": "groups -1 outside [0, 8]",
    "groups_beyond_ncol": "groups 9 outside [0, 8]",
}


def refusal_args(case):
    """Keyword arguments of one refused call of `transition` / the GPU tier's twin on REFUSAL_MODEL: REFUSAL_N pairs."""
    q, v, c = inputs(REFUSAL_MODEL)
    n = REFUSAL_N
    dofs, acts = small_set(REFUSAL_MODEL)
    k = dict(qpos=q[:n], qvel=v[:n], ctrl=c[:n], dofs=dofs, acts=acts, want=("A", "B", "status"))
    k.update({"null_options": dict(no_opt=True), "hold_0": dict(hold=0), "hold_1025": dict(hold=1025), "centered_2": dict(centered=2), "n_negative": dict(n=-1),
              "null_out": dict(no_out=True), "no_outputs": dict(want=()), "qpos_alone": dict(qvel=None), "qvel_alone": dict(qpos=None),
              "n_not_num_envs": dict(qpos=None, qvel=None, n=n, handle=(q[:REFUSAL_ENVS], v[:REFUSAL_ENVS])),
              "eps_qpos_zero": dict(eps_qpos=0.0), "eps_qvel_nan": dict(eps_qvel=float("nan")), "eps_ctrl_inf": dict(eps_ctrl=float("inf")),
              "eps_ctrl_negative": dict(eps_ctrl=-0.5), "no_dofs": dict(dofs=[]), "dof_beyond_nv": dict(dofs=[0, 21]), "dof_free": dict(dofs=[0, 9]),
              "dof_twice": dict(dofs=[3, 0, 3]), "act_beyond_nu": dict(acts=[0, 9]), "act_negative": dict(acts=[-1]), "act_twice": dict(acts=[2, 0, 2]),
              "B_without_acts": dict(acts=[]), "ndofs_19": dict(patch=dict(ndofs=19)), "nacts_19": dict(patch=dict(nacts=19)),
              "grid_too_large": dict(n=0x7fffffff, groups=8), "groups_negative": dict(groups=-1), "groups_beyond_ncol": dict(groups=9)}[case])
    return k
