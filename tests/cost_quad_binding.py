"""The cost-expansion kernel (mujoco_jaco_amd/csrc/cost_quad.h, jaco_cost_quad) under the wavefront emulator (emu_cost_quad of
tests/emu_cost_quad/libjaco_emu_cost_quad{,_d12,_d30}.so) -- TEST INFRASTRUCTURE ONLY.

Also: the inputs (rollout_binding.inputs' states as R = 3 trajectories of T = 4 knots, seeded goals and weights), the dof / ctrl-word sets
(transition_binding.small_set and every hinge dof; on the two-arm model dofs of BOTH arms with the frame on arm 1), the fp64 reference
(the header's formulas in fp64 on jaco_query's fp32 xpos / jac at the same 12 states and the same frame with point = 0) with the derived
per-entry bounds, the cases shared by the CPU and the GPU tier, the refusals, and EmuCostQuadSim: EmuTransitionSim plus the one launch
method `_cost_quad`, so that BatchedMujoco.cost_quad, robot_config.ilqr_expand and robot_config.ilqr run on the emulated calls.

A tier hands the cases
  run(model, qpos [R, T, nq], qvel [R, T, nv], ctrl [R, T, nu] or None, dofs, acts, frame=None, xgoal=None, pgoal=None, goal_idx=None,
      weights=None, goal_per_knot=0, want=OUTS) -> {output: array}      (every output handed in sentinel-filled)
  query(model, qpos [n, nq], qvel [n, nv], frame) -> (xpos [n, 3], jac [n, 6, nv]) fp32: jaco_query on that one frame
"""
import ctypes
import os
import subprocess

import numpy as np

import emu_binding
import ik_binding as ib
import osc_binding as ob
import query_binding as qb
import rollout_binding as rb
import transition_binding as tb
from emu_sim import _np, _tensors
from fd_binding import bits
from mujoco_jaco_amd import _lib as product_lib
from mujoco_jaco_amd.physics import BatchedMujoco
from rollout_binding import SENTINEL, STATUS_SENTINEL

OUTS = ("lx", "lxx", "lu", "Vx", "Vxx", "l", "status")
FLAG_NAN, BAD_INDEX = product_lib.JACO_FLAG_NAN, product_lib.JACO_ROLLOUT_BAD_INDEX
EMU_DIR = os.path.join(emu_binding.ROOT, "tests", "emu_cost_quad")
_libs = {}


def lib(layout=""):
    """The emulator build that holds emu_cost_quad, per layout (built on first use, as emu_binding.lib builds its own)."""
    if layout not in _libs:
        name = "libjaco_emu_cost_quad%s.so" % layout
        subprocess.check_call(["make", "-s", "-C", EMU_DIR, name])
        L = ctypes.CDLL(os.path.join(EMU_DIR, name))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.emu_cost_quad.argtypes = [ctypes.c_char_p, ctypes.c_long, vp, vp, ci, vp, vp, vp, vp, vp]
        L.emu_last_error.restype = ctypes.c_char_p
        _libs[layout] = L
    return _libs[layout]


def shapes(R, T, nd, na):
    nx = 2 * nd
    return {"lx": (R, T, nx), "lxx": (R, T, nx, nx), "lu": (R, T, na), "Vx": (R, nx), "Vxx": (R, nx, nx), "l": (R, T), "status": (R, T)}


def weight_options(weights):
    w = dict(weights or {})
    return {k: w[k] for k in ("wx", "wxT", "wu", "wp", "wpT") if k in w}


def records(tier, outs, dofs, acts, T, xgoal, pgoal, goal_idx, weights, goal_per_knot, ngoals=None, patch=None):
    """(options, goal, out) records of one call on the tier's arrays."""
    opt = product_lib.JacoCostQuadOptions(nknots=T, goal_per_knot=goal_per_knot, dofs=dofs, acts=acts, **weight_options(weights))
    for k, x in (patch or {}).items():
        setattr(opt, k, x)
    if ngoals is None:
        ngoals = next((int(a.shape[0]) for a in (xgoal, pgoal) if a is not None), 0)
    goal = product_lib.JacoCostQuadGoal(tier.ptr(xgoal), tier.ptr(pgoal), tier.ptr(goal_idx), ngoals)
    out = product_lib.JacoCostQuadOut(*[tier.ptr(outs.get(k)) for k in OUTS])
    return opt, goal, out


def prelude(tier, qpos, qvel, ctrl, dofs, acts, want, R=None, nknots=None):
    """(R, T, the sentinel-filled outputs) of one call: what the arrays say unless overridden (refusals)."""
    lead = next((tuple(a.shape[:2]) for a in (qpos, qvel, ctrl) if a is not None), (0, 1))
    sh = shapes(max(lead[0], tier.min_rows), max(lead[1], 1), max(len(dofs), 1), max(len(acts), 1))
    return (lead[0] if R is None else R), (lead[1] if nknots is None else nknots), {k: tier.blank(sh[k], k == "status") for k in want}


def cost_quad(model, qpos, qvel, ctrl, dofs, acts, frame=None, xgoal=None, pgoal=None, goal_idx=None, weights=None, goal_per_knot=0, want=OUTS, R=None,
              nknots=None, ngoals=None, no_opt=False, no_out=False, no_goal=False, patch=None):
    """Emulated jaco_cost_quad: {output: array} in the C ABI's layout.  R / nknots / ngoals override what the arrays say (refusals);
    no_* hand NULL pointers; patch: option fields set by hand.  Raises ValueError with the library's message when the call is refused,
    with the outputs it was handed in .outputs."""
    blob, layout, nu = ob._model_info(model)
    L = lib(layout)
    H = rb.HOST
    q, v, c, xg, pg = [H.f32(a) for a in (qpos, qvel, ctrl, xgoal, pgoal)]
    gi = H.i32(goal_idx)
    R, T, res = prelude(H, q, v, c, dofs, acts, want, R, nknots)
    opt, goal, out = records(H, res, dofs, acts, T, xg, pg, gi, weights, goal_per_knot, ngoals, patch)
    rc = L.emu_cost_quad(blob, len(blob), rb.ref(opt, no_opt), rb.ref(frame), R, H.ptr(q), H.ptr(v), H.ptr(c), rb.ref(goal, no_goal), rb.ref(out, no_out))
    return rb.checked(L, rc, "emu_cost_quad", res)


def emu_query(model, qpos, qvel, frame):
    r = qb.query(model, qpos, qvel, [frame], ("xpos", "jac"))
    return r["xpos"][:, 0], r["jac"][:, 0]


class EmuCostQuadSim(tb.EmuTransitionSim):
    """EmuTransitionSim with jaco_cost_quad: the product's cost_quad over the emulated launch."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches["jaco_cost_quad"] = 0

    def _cost_quad(self, qpos, qvel, ctrl, goal, frame, R, T, want, **options):
        self.launches["jaco_cost_quad"] += 1
        o = dict(options)
        w = {k: o.pop(k) for k in ("wx", "wxT", "wu", "wp", "wpT")}
        return _tensors(cost_quad(self.model, _np(qpos), _np(qvel), _np(ctrl), o["dofs"], o["acts"], frame, _np(goal.get("xgoal")), _np(goal.get("pgoal")),
                                  _np(goal.get("goal_idx")), w, o["goal_per_knot"], tuple(want), R=R, nknots=T, ngoals=goal.get("ngoals", 0)))

    cost_quad = BatchedMujoco.cost_quad


# ---- inputs and sets
MODELS = (rb.MODEL,) + rb.SMALL
R, T = 3, 4
GOAL_DQ, GOAL_DV, GOAL_P = 0.3, 1.0, 0.25


def frame_of(model):
    """The EE frame (arm 1's on the two-arm model) with a NON-ZERO point: the kernel must ignore it."""
    return rb.frames(model)[1]


def query_frame(model):
    """The same frame with point = 0, for jaco_query: its Jacobian point is then the frame's origin, the kernel's pos."""
    return ib.table_of(model).jaco_frame(rb.ee_name(model), point=np.zeros(3))


def small_set(model):
    return tb.small_set(model)


def every_set(model):
    """Every hinge dof (at most 18) and every ctrl word: on the two-arm model dofs of BOTH arms, the frame on arm 1."""
    return tb.every_set(model)


SETS = {"small": small_set, "every": every_set}
_inputs = {}


def inputs(model, which="small"):
    """The shared inputs of a model and set, drawn once: q [R, T, nq], v, c [R, T, nu] (rollout_binding.inputs' 12 states and first ctrl
    rows), goals per trajectory and knot xgoal [R, T, nx] (the states displaced by up to GOAL_DQ rad / GOAL_DV rad/s) and pgoal [R, T, 3],
    weights distinct per word with the last knot's ten times the running ones."""
    key = (model, which)
    if key not in _inputs:
        q, v, c = rb.inputs(model, R * T, 1)
        nq, nv, nu = q.shape[1], v.shape[1], c.shape[2]
        dofs, acts = SETS[which](model)
        nd = len(dofs)
        rng = np.random.default_rng(113)
        x = tb.x_of(model, dofs, q, v).reshape(R, T, 2 * nd)
        d = rng.uniform(-1, 1, (R, T, 2 * nd)) * np.concatenate([np.full(nd, GOAL_DQ), np.full(nd, GOAL_DV)])
        wx = np.concatenate([rng.uniform(1.0, 3.0, nd), rng.uniform(0.02, 0.06, nd)])
        _inputs[key] = dict(q=q.reshape(R, T, nq), v=v.reshape(R, T, nv), c=np.ascontiguousarray(c.reshape(R, T, nu)), dofs=dofs, acts=acts,
                            xgoal=(x.astype(np.float64) + d).astype(np.float32),
                            pgoal=(np.array([0.3, 0.0, 0.5]) + rng.uniform(-GOAL_P, GOAL_P, (R, T, 3))).astype(np.float32),
                            weights=dict(wx=wx, wxT=10 * wx, wu=rng.uniform(0.01, 0.03, len(acts)), wp=4.0, wpT=40.0), frame=frame_of(model))
    return _inputs[key]


def call_args(g, goal_per_knot=1, pose=True, **more):
    """The keyword arguments of `run` on the shared inputs g; pose=False: the pose weights zero."""
    pick = (lambda a: a) if goal_per_knot else (lambda a: np.ascontiguousarray(a[:, :1]))
    w = g["weights"] if pose else {**g["weights"], "wp": 0.0, "wpT": 0.0}
    k = dict(qpos=g["q"], qvel=g["v"], ctrl=g["c"], dofs=g["dofs"], acts=g["acts"], frame=g["frame"], xgoal=pick(g["xgoal"]), pgoal=pick(g["pgoal"]),
             weights=w, goal_per_knot=goal_per_knot)
    k.update(more)
    return k


def same(a, b, keys=None):
    for k in (keys or a):
        assert a[k].shape == b[k].shape and (bits(a[k]) == bits(b[k])).all(), k


# ---- the fp64 reference and its bounds
U = 2.0 ** -24   # the unit roundoff of fp32
SLACK = 1.0 + 2.0 ** -20   # second-order terms of the first-order counts below


def reference(model, g, query, goal_per_knot=1, weights=None):
    """The header's formulas in fp64 on jaco_query's fp32 xpos / jac (same frame, point = 0) at the R * T states, the weights as the fp32
    words the options hold: {"gx" [R, T, nx], "H" [R, T, nx, nx], "l" [R, T]: per work item, "lu" [R, T, na]} and the per-entry bounds
    {"gx", "H", "l"} = c * 2^-24 * sum |terms|, c counted from cost_quad.h's chain (pos and Jp taken as jaco_query's words):
      gx_j = fma(Wp, fma(j2, e2, fma(j1, e1, j0 * e0)), W_j * d_j):  d_j and e_c are one rounded subtraction each, which the products carry
             on (2 |W d| with the product's own rounding; 1 on every |Jp e|), the chain's three roundings each act on a partial sum no
             larger than sum_c |Jp e|, the outer fma rounds a value no larger than the sum of all terms:  2 |W d| + (1 + 3 + 1) Wp sum_c
             |Jp e| + |W d|  <=  5 (|W d| + Wp sum_c |Jp_c e_c|).  Without the pose term: 2 |W d|.
      H_ji = fma(Wp, fma(j2 i2, fma(j1 i1, j0 i0)), delta W):  three roundings on partial sums no larger than sum_c |Jp Jp|, one on the
             result:  4 (Wp sum_c |Jp_cj Jp_ci| + delta_ji W_j).  Without the pose term the entry is W_j or 0.0f exactly.
      l:     a state or pose term (0.5 w) (d d): the rounded subtraction twice, the square, the product: 4; a ctrl term: 2; every term is
             non-negative and passes the six levels of wave_sum's tree and the two final additions, each rounding a partial sum no larger
             than l:  (4 + 6 + 2) l = 12 l."""
    f64 = lambda a: np.asarray(a, np.float64)
    w = weights or g["weights"]
    dofs, acts = g["dofs"], g["acts"]
    nd, nx, na = len(dofs), 2 * len(dofs), len(acts)
    pad = lambda a, m: np.concatenate([f64(np.asarray(a, np.float32)), np.zeros(m)])[:m]
    wx, wxT, wu = pad(w.get("wx", ()), nx), pad(w.get("wxT", ()), nx), pad(w.get("wu", ()), na)
    wp, wpT = float(np.float32(w.get("wp", 0.0))), float(np.float32(w.get("wpT", 0.0)))
    q, v = g["q"], g["v"]
    x = f64(tb.x_of(model, dofs, q, v))
    knots = np.arange(T) if goal_per_knot else np.zeros(T, int)
    d = x - f64(g["xgoal"])[:, knots]
    last = np.arange(T) == T - 1
    W = np.where(last[:, None], wxT, wx)[None]                              # [1, T, nx]
    Wp = np.where(last, wpT, wp)[None, :, None]                             # [1, T, 1]
    pose = bool(wp or wpT)
    xpos, jac = query(model, q.reshape(R * T, -1), v.reshape(R * T, -1), query_frame(model))
    Jp = f64(jac)[:, :3][:, :, list(dofs)].reshape(R, T, 3, nd) * pose
    e = (f64(xpos).reshape(R, T, 3) - f64(g["pgoal"])[:, knots]) * pose
    gx, gxb = W * d, 2 * np.abs(W * d)
    je = np.abs(Jp * e[..., None]).sum(2)                                   # sum_c |Jp e| [R, T, nd]
    gx[..., :nd] += Wp * (Jp * e[..., None]).sum(2)
    posed = np.broadcast_to(Wp != 0, je.shape)
    gxb[..., :nd] = np.where(posed, 5 * (np.abs(W * d)[..., :nd] + Wp * je), gxb[..., :nd])
    H = np.zeros((R, T, nx, nx))
    H[..., np.arange(nx), np.arange(nx)] = np.broadcast_to(W, (R, T, nx))
    Hb = np.zeros_like(H)
    jj = np.einsum("rtcj,rtci->rtji", Jp, Jp)
    H[..., :nd, :nd] += Wp[..., None] * jj
    Hb[..., :nd, :nd] = np.where(Wp[..., None] != 0, 4 * (Wp[..., None] * np.einsum("rtcj,rtci->rtji", np.abs(Jp), np.abs(Jp)) + np.eye(nd) * W[..., :nd, None]), 0.0)
    u = f64(g["c"])[..., list(acts)] if na else np.zeros((R, T, 0))
    parts = np.stack([0.5 * (wu * u ** 2).sum(2), 0.5 * (W * d ** 2).sum(2), 0.5 * Wp[..., 0] * (e ** 2).sum(2)], 2)
    l = parts.sum(2)
    return dict(gx=gx, H=H, l=l, parts=parts, lu=wu * u, Jp=Jp, bound=dict(gx=gxb * U * SLACK, H=Hb * U * SLACK, l=12 * l * U * SLACK))


def items(r):
    """A call's lx / Vx and lxx / Vxx back as per-work-item arrays [R, T, ..] (item k < T - 1 is row k + 1; the last is Vx / Vxx)."""
    return np.concatenate([r["lx"][:, 1:], r["Vx"][:, None]], 1), np.concatenate([r["lxx"][:, 1:], r["Vxx"][:, None]], 1)


def case_reference(run, query, model, which, goal_per_knot=1):
    """1: every entry of lx, lxx, Vx, Vxx, l against the fp64 reference within its derived bound; lu bit for bit.  Returns the largest
    measured / bound over the three."""
    g = inputs(model, which)
    r = run(model, **call_args(g, goal_per_knot))
    ref = reference(model, g, query, goal_per_knot)
    gx, H = items(r)
    worst = {}
    for name, got, want in (("gx", gx, ref["gx"]), ("H", H, ref["H"]), ("l", r["l"], ref["l"])):
        err, bound = np.abs(got.astype(np.float64) - want), ref["bound"][name]
        assert np.isfinite(got).all()
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        worst[name] = float(ratio.max())
    print("MEASURE reference %s %s set (goal per knot %d): largest measured / bound: lx, Vx %.3g  lxx, Vxx %.3g  l %.3g"
          % (model, which, goal_per_knot, worst["gx"], worst["H"], worst["l"]))
    assert not r["status"].any()
    assert (bits(r["lu"]) == bits((np.asarray(g["weights"]["wu"], np.float32) * g["c"][..., list(g["acts"])]).astype(np.float32))).all()
    if model == "jaco2_dual_torque" and which == "every":   # arm 2's dofs do not move arm 1's frame: exact zero columns, rows and entries
        nd = len(g["dofs"])
        off = np.flatnonzero(~ref["Jp"].any((0, 1, 2)))
        assert len(off) >= nd // 2 - 1 and len(off) < nd, off
        on = np.setdiff1d(np.arange(nd), off)
        blk = H[..., :nd, :nd]
        assert (bits(blk[..., off, :][..., on]) == 0).all() and (bits(blk[..., on, :][..., off]) == 0).all()
    assert max(worst.values()) <= 1.0, worst
    return worst


def case_exact(run, model, which="small"):
    """3: the properties that hold bit for bit."""
    g = inputs(model, which)
    nd, nx = len(g["dofs"]), 2 * len(g["dofs"])
    f32 = np.float32
    w = g["weights"]
    wx, wxT, wu = [np.asarray(w[k], f32) for k in ("wx", "wxT", "wu")]
    x = tb.x_of(model, g["dofs"], g["q"], g["v"]).astype(f32)
    # -- the pose weights zero: one subtraction and one multiplication; lxx = diag(w); cross blocks zero
    r0 = run(model, **call_args(g, 1, pose=False))
    gx, H = items(r0)
    W = np.where((np.arange(T) == T - 1)[:, None], wxT, wx)
    assert (bits(gx) == bits((W * (x - g["xgoal"])).astype(f32))).all()
    assert (bits(r0["lu"]) == bits((wu * g["c"][..., list(g["acts"])]).astype(f32))).all()
    assert (bits(H) == bits(np.broadcast_to(W[:, :, None] * np.eye(nx, dtype=f32), H.shape).astype(f32))).all()
    # -- with the pose term
    full = run(model, **call_args(g, 1))
    gx, H = items(full)
    for k in ("lx", "lxx"):                                                  # row 0: exact zeros
        assert (bits(full[k][:, 0]) == 0).all(), k
    for k in ("lxx", "Vxx"):                                                 # symmetric bit for bit
        assert (bits(full[k]) == bits(np.swapaxes(full[k], -1, -2))).all(), k
    off = ~np.eye(nd, dtype=bool)
    for blk in (H[..., :nd, nd:], H[..., nd:, :nd], H[..., nd:, nd:][..., off]):   # the cross blocks and the off-diagonal velocity entries
        assert (bits(blk) == 0).all()
    assert (bits(H[..., nd:, nd:][..., ~off]) == bits(np.broadcast_to(W[:, nd:], (R, T, nd)).astype(f32))).all()
    assert (bits(H[..., :nd, :nd]) != bits(np.broadcast_to(W[:, :nd, None] * np.eye(nd, dtype=f32), H[..., :nd, :nd].shape).astype(f32))).any()   # the pose term is in
    # -- the last item lands in Vx / Vxx with the final weights and nowhere in lx / lxx: with only final weights lx / lxx are all zero
    final = run(model, **call_args(g, 1, weights={**w, "wx": np.zeros(nx), "wp": 0.0, "wu": np.zeros(len(g["acts"]))}))
    assert not final["lx"].any() and (bits(final["lxx"]) == 0).all() and (bits(final["l"][:, :-1]) == 0).all()
    same(final, full, ("Vx", "Vxx"))
    assert final["Vx"].any() and (np.diagonal(final["Vxx"], axis1=1, axis2=2) > 0).all()
    # -- any subset of the outputs gives the same words
    for want in [(k,) for k in OUTS] + [("lx", "Vxx"), ("lxx", "l", "status")]:
        r = run(model, **call_args(g, 1, want=want))
        assert set(r) == set(want)
        same(r, full, want)
    # -- goal_idx sharing = materialised goals; goal_per_knot picks goal k for x_(k+1)
    idx = np.array([2, 0, 2], np.int32)
    shared = run(model, **call_args(g, 1, goal_idx=idx))
    mat = run(model, **call_args({**g, "xgoal": g["xgoal"][idx], "pgoal": g["pgoal"][idx]}, 1))
    same(shared, mat)
    one = run(model, **call_args(g, 0))
    for k in range(T):
        held = run(model, **call_args({**g, "xgoal": np.repeat(g["xgoal"][:, k:k + 1], T, 1), "pgoal": np.repeat(g["pgoal"][:, k:k + 1], T, 1)}, 1))
        a, b = items(held), items(full)
        assert (bits(a[0][:, k]) == bits(b[0][:, k])).all() and (bits(a[1][:, k]) == bits(b[1][:, k])).all() and (bits(held["l"][:, k]) == bits(full["l"][:, k])).all()
        if k == 0:
            same(one, held)
    # -- two runs are identical; a NULL ctrl is zeros
    same(full, run(model, **call_args(g, 1)))
    none = run(model, **call_args(g, 1, ctrl=None))
    assert (bits(none["lu"]) == 0).all()
    same(none, full, ("lx", "lxx", "Vx", "Vxx", "status"))
    return full


def case_bad_index(run, model=rb.MODEL):
    """A goal_idx entry out of range: that trajectory's items write their status word and nothing else; the others are untouched by it."""
    g = inputs(model)
    good = run(model, **call_args(g, 1, goal_idx=np.array([0, 1, 2], np.int32)))
    for wrong in (-1, R):
        r = run(model, **call_args(g, 1, goal_idx=np.array([0, wrong, 2], np.int32)))
        assert (r["status"][1] == BAD_INDEX).all() and not r["status"][[0, 2]].any()
        for k in ("lx", "lxx", "lu", "l"):
            assert (bits(r[k][1]) == bits(np.float32(SENTINEL))).all(), k
            assert (bits(r[k][[0, 2]]) == bits(good[k][[0, 2]])).all(), k
        for k in ("Vx", "Vxx"):
            assert (bits(r[k][1]) == bits(np.float32(SENTINEL))).all() and (bits(r[k][[0, 2]]) == bits(good[k][[0, 2]])).all(), k


def case_non_finite(run, model=rb.MODEL):
    """An input word that is not finite sets JACO_FLAG_NAN in that item's status word, and in no other's."""
    g = inputs(model)
    for name, at in (("q", (1, 2, 0)), ("v", (0, 3, 1)), ("c", (2, 0, 2)), ("xgoal", (1, 1, 0)), ("pgoal", (2, 2, 1))):
        a = g[name].copy()
        a[at] = np.nan if name != "v" else np.inf
        r = run(model, **call_args({**g, name: a}, 1, want=("status",)))
        want = np.zeros((R, T), np.uint32)
        want[at[:2]] = FLAG_NAN
        assert (r["status"] == want).all(), (name, r["status"])


def case_empty(run, model=rb.MODEL):
    """R = 0 is accepted after every check and writes nothing: the call is handed three trajectories' arrays and outputs with R
    overridden to 0, and every output word keeps its sentinel."""
    g = inputs(model)
    r = run(model, **call_args(g, 1, R=0))
    assert r["lxx"].shape[0] == R
    for k, a in r.items():
        assert (a == (STATUS_SENTINEL if k == "status" else SENTINEL)).all(), k


def case_stray_weights(run, model=rb.MODEL):
    """State weights behind the first 2 ndofs words are not used: with them set and nothing else, no goal and no state row is asked
    for, and the call equals the one without them."""
    g = inputs(model)
    nx = 2 * len(g["dofs"])
    k = dict(qpos=None, qvel=None, ctrl=g["c"], dofs=g["dofs"], acts=g["acts"], want=("lu", "l", "status"))
    wu = g["weights"]["wu"]
    plain = run(model, **k, weights={"wu": wu})
    stray = run(model, **k, weights={"wu": wu, "wx": [0.0] * nx + [2.0], "wxT": [0.0] * (nx + 1) + [3.0]})
    same(plain, stray)
    assert not plain["status"].any() and plain["l"].all()


# ---- against the existing kernel
def case_rollout_cost(run, run_cost, model):
    """2: jaco_rollout_cost on 3 plans x 4 knots x hold 2 with all three weights on, a per-knot goal and distinct final weights; its qpos,
    qvel, ctrl outputs fed to jaco_cost_quad: sum_k l[r][k] = cost[r] within rollout_cost_binding.cap, and each of the three parts (the
    call with only that weight on) against `terms`.  run_cost: rollout_cost_binding's `run` on the same tier."""
    import rollout_cost_binding as cb
    g = inputs(model)
    dofs, acts = g["dofs"], g["acts"]
    nu = g["c"].shape[2]
    wu_full = np.zeros(nu)
    wu_full[list(acts)] = g["weights"]["wu"]
    wr = {**g["weights"], "wu": wu_full}
    rc = run_cost(model, g["c"], qpos0=g["q"][:, 0], qvel0=g["v"][:, 0], xgoal=g["xgoal"], pgoal=g["pgoal"], weights=wr, goal_per_knot=1, dofs=dofs,
                  frame=g["frame"], want=("qpos", "qvel", "ctrl", "cost", "terms", "status"), hold=2)
    assert not rc["status"].any()
    traj = {**g, "q": rc["qpos"], "v": rc["qvel"], "c": rc["ctrl"]}
    r = run(model, **call_args(traj, 1, want=("l", "status")))
    assert not r["status"].any()
    cap = cb.cap(T, 2 * len(dofs), nu)
    J = r["l"].astype(np.float64).sum(1)
    eJ = float((np.abs(J - rc["cost"]) / rc["cost"]).max())
    zero = {"wx": np.zeros(2 * len(dofs)), "wxT": np.zeros(2 * len(dofs)), "wu": np.zeros(len(acts)), "wp": 0.0, "wpT": 0.0}
    eT = 0.0
    for part, keys in enumerate((("wu",), ("wx", "wxT"), ("wp", "wpT"))):
        one = run(model, **call_args(traj, 1, want=("l",), weights={**zero, **{k: g["weights"][k] for k in keys}}))
        eT = max(eT, float((np.abs(one["l"].astype(np.float64).sum(1) - rc["terms"][:, part]) / rc["cost"]).max()))
    print("MEASURE rollout_cost %s: |sum l - cost| / cost %.3g, largest |part - term| / cost %.3g, cap %.3g" % (model, eJ, eT, cap))
    assert (rc["terms"] > 0).all()
    assert eJ <= cap and eT <= cap, (eJ, eT, cap)


# ---- the refusals: one argument set per message of jaco_cost_quad_resolve, for the emulator's entry and the library's alike
REFUSAL_MODEL = "jaco2_curtain_torque"   # dofs 0-8 hinges, 9-20 free joints; 9 ctrl words; 11 fused bodies
REFUSALS = {
    "null_options": "the options are required",
    "null_out": "the output record is required",
    "no_outputs": "at least one of the outputs lx, lxx, lu, Vx, Vxx, l and status is required",
    "R_negative": "R -1 is negative",
    "nknots_0": "nknots 0 is below 1",
    "goal_per_knot_2": "goal_per_knot must be 0 or 1",
    "grid_too_large": "R 2147483647 x nknots 4 is beyond the largest grid",
    "no_dofs": "ndofs 0 outside [1, 18]",
    "ndofs_19": "ndofs 19 outside [1, 18]",
    "dof_beyond_nv": "dof 21 outside [0, 21)",
    "dof_free": "dof 9 belongs to a free joint",
    "dof_twice": "dof 3 is listed twice",
    "nacts_19": "nacts 19 outside [0, 18]",
    "act_beyond_nu": "ctrl word 9 outside [0, 9)",
    "act_negative": "ctrl word -1 outside [0, 9)",
    "act_twice": "ctrl word 2 is listed twice",
    "wx_negative": "weight wx[1] is negative or not finite",
    "wxT_nan": "weight wxT[0] is negative or not finite",
    "wu_inf": "weight wu[1] is negative or not finite",
    "wp_negative": "weight wp is negative or not finite",
    "wpT_nan": "weight wpT is negative or not finite",
    "state_weight_without_xgoal": "a non-zero state weight needs xgoal",
    "state_weight_without_goal_record": "a non-zero state weight needs xgoal",
    "pose_weight_without_pgoal": "a non-zero pose weight needs pgoal",
    "pose_weight_without_frame": "a non-zero pose weight needs a frame",
    "pose_weight_world_frame": "a non-zero pose weight needs a frame on a body: a world-fixed frame has no Jacobian",
    "pose_weight_bad_body": "frame body 11 outside [0, 11)",
    "lu_without_acts": "lu needs at least one ctrl word",
    "qpos_alone": "qpos and qvel are given together or not at all",
    "qvel_alone": "qpos and qvel are given together or not at all",
    "qpos_alone_without_weights": "qpos and qvel are given together or not at all",
    "weights_without_states": "a non-zero state or pose weight needs qpos and qvel",
    "no_goals": "ngoals 0: at least one goal is required",
    "more_trajectories_than_goals": "R 3 trajectories from 2 goals without a goal index",
}


def refusal_args(case):
    """Keyword arguments of one refused call of `cost_quad` / the GPU tier's twin on REFUSAL_MODEL."""
    g = inputs(REFUSAL_MODEL)
    w = g["weights"]
    nx = 2 * len(g["dofs"])
    world, far = rb.frames(REFUSAL_MODEL)[0], frame_of(REFUSAL_MODEL)
    far = type(far).from_buffer_copy(far)
    far.body = 11
    no_state = {**w, "wx": np.zeros(nx), "wxT": np.zeros(nx)}
    k = call_args(g, 1)
    k.update({"null_options": dict(no_opt=True), "null_out": dict(no_out=True), "no_outputs": dict(want=()), "R_negative": dict(R=-1), "nknots_0": dict(nknots=0),
              "goal_per_knot_2": dict(goal_per_knot=2), "grid_too_large": dict(R=0x7fffffff), "no_dofs": dict(dofs=[]), "ndofs_19": dict(patch=dict(ndofs=19)),
              "dof_beyond_nv": dict(dofs=[0, 21, 5]), "dof_free": dict(dofs=[0, 9, 5]), "dof_twice": dict(dofs=[3, 0, 3]), "nacts_19": dict(patch=dict(nacts=19)),
              "act_beyond_nu": dict(acts=[0, 9]), "act_negative": dict(acts=[-1, 0]), "act_twice": dict(acts=[2, 2]),
              "wx_negative": dict(weights={**w, "wx": [1.0, -1.0]}), "wxT_nan": dict(weights={**w, "wxT": [float("nan")]}),
              "wu_inf": dict(weights={**w, "wu": [0.0, float("inf")]}), "wp_negative": dict(weights={**w, "wp": -1.0}),
              "wpT_nan": dict(weights={**w, "wpT": float("nan")}), "state_weight_without_xgoal": dict(xgoal=None),
              "state_weight_without_goal_record": dict(no_goal=True), "pose_weight_without_pgoal": dict(pgoal=None, weights={**w, "wp": 0.0}),
              "pose_weight_without_frame": dict(frame=None), "pose_weight_world_frame": dict(frame=world), "pose_weight_bad_body": dict(frame=far),
              "lu_without_acts": dict(acts=[], weights={**w, "wu": []}), "qpos_alone": dict(qvel=None), "qvel_alone": dict(qpos=None),
              "qpos_alone_without_weights": dict(qvel=None, weights={**no_state, "wp": 0.0, "wpT": 0.0}, want=("lu", "l", "status")),
              "weights_without_states": dict(qpos=None, qvel=None, weights={**no_state, "wpT": 0.0}), "no_goals": dict(ngoals=0),
              "more_trajectories_than_goals": dict(ngoals=2)}[case])
    return k


# ---- the Python layer: ilqr_expand and ilqr on jaco2_reaching_torque (the inputs of test_gpu_transition.py's one-iteration test)
def ilqr_problem(make_sim, B, T):
    """(cfg, u [B, T, m], ubar [B, nu], goal [B, n], q0 [B, n]) on lqr_binding.ARM_MODEL around gravity compensation, from osc_binding.states."""
    import lqr_binding as lb
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    model = lb.ARM_MODEL
    q, _ = ob.states(model, B)
    sim = make_sim(model, q.astype(np.float32), np.zeros((B, int(ib.load_model(model)["nv"][0])), np.float32))
    cfg = BatchedMujocoConfig(sim, ee="EE")
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    ubar = cfg.joint(joints=None).gravity_compensation()
    u = ubar[:, None, acts].expand(-1, T, -1).contiguous()
    qpos0, _, _ = sim.get_state()
    q0 = qpos0[:, qadr]
    return cfg, u, ubar, q0 + lb.GOAL_OFF, q0


def case_ilqr_expand(make_sim, launches, B, T, hold):
    """5a: ilqr_expand with joint-space weights only against the one-iteration test's hand-built torch arrays, bit for bit: lx rows
    1 .. T - 1 = w * (x_t - goal) (row 0, the start state, is not costed by rollout_cost: exact zeros here), lu = WU * u, Vx = wf * (x_T -
    goal); A, B, x, u, status = linearize_rollout's bit for bit; three launches."""
    import torch
    import lqr_binding as lb
    cfg, u, ubar, goal, _ = ilqr_problem(make_sim, B, T)
    n = goal.shape[1]
    A, Bm, X, ua, status = cfg.linearize_rollout(u, ctrl=ubar, hold=hold)
    launches()
    e = cfg.ilqr_expand(u, ctrl=ubar, hold=hold, q_goal=goal, dq_goal=torch.zeros_like(goal), w_q=lb.WQ, w_dq=lb.WV, w_u=lb.WU, w_q_final=lb.WF)
    assert launches() == 3
    for k, t in (("A", A), ("B", Bm), ("x", X), ("u", ua), ("status", status)):
        assert e[k].dtype == t.dtype and torch.equal(e[k].view(torch.int32), t.view(torch.int32)), k
    w = torch.tensor([lb.WQ] * n + [lb.WV] * n, device=X.device)
    wf = torch.tensor([lb.WF] * n + [lb.WV] * n, device=X.device)
    D = X.clone()
    D[..., :n] -= goal[:, None]
    assert torch.equal(e["lx"][:, 1:], (w * D[:, :-1])[:, 1:]) and not e["lx"][:, 0].any()
    assert torch.equal(e["lu"], lb.WU * ua) and torch.equal(e["Vx"], wf * D[:, -1])
    assert torch.equal(e["lxx"][:, 1:], torch.diag(w).expand(B, T - 1, -1, -1)) and not e["lxx"][:, 0].any()
    assert torch.equal(e["Vxx"], torch.diag(wf).expand(B, -1, -1)) and torch.equal(e["luu"], lb.WU * torch.eye(ua.shape[2], device=X.device))
    assert e["l"].shape == (B, T)


ILQR_COST = dict(w_ee_final=400.0, w_dq=0.02, w_u=1e-3)


def case_ilqr(make_sim, launches, B, T, hold, iterations):
    """5b: ilqr with an EE goal (the hand's position at q0 + GOAL_OFF), w_ee_final > 0, a small w_dq and w_u: 5 launches per iteration and
    one rollout_feedback launch at the end; cost non-increasing per env, bit for bit; at least one accepted step per env; the final
    cost below the nominal's; no status flag; the returned plan re-costed by rollout_cost gives cost[-1] bit for bit."""
    import torch
    cfg, u, ubar, goal, q0 = ilqr_problem(make_sim, B, T)
    ee = cfg.Tx("EE", q=goal).clone()
    cost = dict(ee_goal=ee, dq_goal=torch.zeros_like(goal), **ILQR_COST)
    launches()
    r = cfg.ilqr(u, iterations, ctrl=ubar, hold=hold, **cost)
    assert launches() == 5 * iterations + 1
    c = r["cost"].cpu().numpy()
    assert c.shape == (iterations + 1, B) and np.isfinite(c).all()
    assert (c[1:] <= c[:-1]).all(), c
    acc = r["accepted"].cpu().numpy()
    assert acc.shape == (iterations, B) and acc.any(0).all(), acc
    assert (c[-1] < c[0]).all() and not r["status"].cpu().numpy().any()
    assert ((c[1:] < c[:-1]) == acc).all()
    again = cfg.rollout_cost(r["u"], ctrl=ubar, hold=hold, **cost)
    assert torch.equal(again["cost"], r["cost"][-1])
    print("MEASURE ilqr: %d envs x %d knots x hold %d, %d iterations: cost / nominal's per iteration %s; accepted %s; mu %s"
          % (B, T, hold, iterations, " | ".join(" ".join("%.4f" % x for x in row) for row in (c / c[0])), acc.sum(0), r["mu"].cpu().numpy()))
    return r
