"""The backward-pass kernel (mujoco_jaco_amd/csrc/lqr.h, jaco_lqr) under the wavefront emulator (tests/emu_lqr/libjaco_emu_lqr.so, built
on demand as emu_binding.lib builds its libraries) -- TEST INFRASTRUCTURE ONLY.

Also: the input sets, the fp64 recursion (numpy, from the formulas of include/jaco_env.h) with the condition the inputs must meet
asserted on it, the measures, and the cases shared by the CPU and the GPU tier.  A tier hands the cases a `sim`: a BatchedMujoco (GPU)
or emu_sim.EmuSim (the product's own lqr_backward with only the one launch replaced), and for the refusals the raw entry.
Every output is handed in filled with FILL (status: STATUS_FILL), so what a call leaves untouched shows.
"""
import ctypes
import os
import subprocess

import numpy as np

from mujoco_jaco_amd import _lib as product_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu_lqr")
OUTS = ("gain", "kff", "dV", "Vxx0", "Vx0", "status")
VALUES = OUTS[:5]
FILL, STATUS_FILL = np.float32(-1234.5), np.uint32(0xDEADBEEF)
BAD_INDEX, NOT_PD = product_lib.JACO_LQR_BAD_INDEX, product_lib.JACO_LQR_NOT_PD
_lib = []


def lib():
    if not _lib:
        subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libjaco_emu_lqr.so"])
        L = ctypes.CDLL(os.path.join(EMU_DIR, "libjaco_emu_lqr.so"))
        L.emu_lqr.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.emu_last_error.restype = ctypes.c_char_p
        _lib.append(L)
    return _lib[0]


def raw(opt, n, prob, out):
    """The entry as it is, on ctypes records (None: a NULL pointer): (return code, the message it left)."""
    cast = lambda s: None if s is None else ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)
    L = lib()
    rc = L.emu_lqr(cast(opt), int(n), cast(prob), cast(out))
    return rc, L.emu_last_error().decode()


def lqr(opt, prob, out, n):
    """Emulated jaco_lqr on what BatchedMujoco._lqr is handed (CPU tensors), written in place.  Raises ValueError with the library's
    message when the call is refused."""
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    o = product_lib.JacoLqrOptions(**opt)
    p = product_lib.JacoLqrProblem(*[ptr(prob.get(k)) for k in ("A", "B", "lxx", "luu", "lux", "lx", "lu", "Vxx", "Vx", "mu", "prob_idx")], int(prob["nprob"]))
    r = product_lib.JacoLqrOut(*[ptr(out.get(k)) for k in OUTS])
    rc, why = raw(o, n, p, r)
    if rc != 0:
        raise ValueError("emu_lqr returned %d: %s" % (rc, why))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, keys=OUTS):
    return all((bits(a[k]) == bits(b[k])).all() for k in keys)


def shapes(n, T, rows, nx):
    return {"gain": (n, T, rows, nx), "kff": (n, T, rows), "dV": (n, 2), "Vxx0": (n, nx, nx), "Vx0": (n, nx), "status": (n,)}


def call(sim, inp, n=None, rows=None, rows_out=None, **over):
    """sim.lqr_backward on the input set `inp` (numpy; keys of lqr_backward's arguments; `over` replaces or adds entries) into outputs
    pre-filled with FILL: {output: numpy array}, status as uint32."""
    import torch
    a = {**inp, **over}
    P, T, nx, nu = a["A"].shape[0], a["A"].shape[1], a["A"].shape[2], a["B"].shape[3]
    if n is None:
        n = len(a["problem_index"]) if a.get("problem_index") is not None else (len(a["mu"]) if np.ndim(a.get("mu")) == 1 else P)
    sh = shapes(n, T, nu if rows_out is None else rows_out, nx)
    out = {k: torch.full(sh[k], float(FILL), dtype=torch.float32, device=sim.device) for k in VALUES}
    out["status"] = torch.from_numpy(np.full(sh["status"], STATUS_FILL, np.uint32).view(np.int32)).to(sim.device)
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x), device=sim.device)
    r = sim.lqr_backward(*[t(a[k]) for k in ("A", "B", "lxx", "luu")], **{k: t(a.get(k)) for k in ("lux", "lx", "lu", "Vxx", "Vx", "mu", "problem_index")},
                         rows=rows, rows_out=rows_out, out=out)
    res = {k: r[k].cpu().numpy() for k in OUTS}
    res["status"] = res["status"].view(np.uint32)
    return res


# ---- inputs: everything rounded to fp32 first; the same fp32 numbers go to the kernel and to the reference
H = 0.002
SHAPES = {"2x1x1": (2, 1, 1, 3), "10x3x7": (10, 3, 7, 3), "18x6x50": (18, 6, 50, 3), "36x12x50": (36, 12, 50, 3), "36x18x50": (36, 18, 50, 3),
          "7x2x3": (7, 2, 3, 3), "10x3x7x67": (10, 3, 7, 67)}
SETS = tuple(SHAPES) + ("default_model",)
LUX = 2e-3        # lux ~ LUX U(-1, 1): lux' luu^-1 lux stays below lxx (||lux||_2 <= 6 LUX at 18 x 36; 1e3 (6 LUX)^2 = 0.14 < 1)
MIN_PIVOT = 1e-2  # every knot's smallest Cholesky pivot^2 over max diag(Quu), in the fp64 reference
_inputs, _refs = {}, {}


def inputs(name):
    """The input set `name` as fp32 arrays: A [P, T, nx, nx], B [P, T, nx, nu], lxx [nx, nx], luu [nu, nu], lux [P, T, nu, nx], lx [P, T,
    nx], lu [P, T, nu], Vxx [nx, nx], Vx [P, nx]."""
    if name in _inputs:
        return _inputs[name]
    if name == "default_model":
        g = real_inputs()
    else:
        nx, nu, T, P = SHAPES[name]
        rng = np.random.default_rng([nx, nu, T, P])
        U = rng.uniform
        if nx % 2 == 0:   # x = [q, dq] of nd joints, one substep of H: the structure linearize gives
            nd = nx // 2
            S = U(-5, 5, (P, T, nd, nd)) - U(0, 50, (P, T, nd))[..., None] * np.eye(nd)
            D = U(-0.2, 0.2, (P, T, nd, nd)) - U(0.5, 5, (P, T, nd))[..., None] * np.eye(nd)
            G = U(-1, 1, (P, T, nd, nu))
            lead = U(2, 20, (P, T, min(nd, nu)))
            for a in range(min(nd, nu)):
                G[..., a, a] += lead[..., a]
            I = np.eye(nd)
            A = np.concatenate([np.concatenate([I + H * H * S, H * (I + H * D)], -1), np.concatenate([H * S, I + H * D], -1)], -2)
            Bm = np.concatenate([H * H * G, H * G], -2)
            w = np.array([100.0] * nd + [1.0] * nd)
        else:             # no structure: a random stable A (spectral radius 0.9)
            A = U(-1, 1, (P, T, nx, nx))
            A *= 0.9 / np.abs(np.linalg.eigvals(A)).max(-1)[..., None, None]
            Bm = U(-1, 1, (P, T, nx, nu))
            w = np.array([100.0] * (nx // 2) + [1.0] * (nx - nx // 2))
        g = dict(A=A, B=Bm, lxx=np.diag(w), luu=1e-3 * np.eye(nu), lux=LUX * U(-1, 1, (P, T, nu, nx)), lx=U(-1, 1, (P, T, nx)),
                 lu=1e-3 * U(-1, 1, (P, T, nu)), Vxx=10.0 * np.diag(w), Vx=U(-1, 1, (P, nx)))
    _inputs[name] = {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}
    return _inputs[name]


ARM_MODEL = "jaco2_reaching_torque"   # the robot_config cases (case_config, case 7): the model rollout_fb_binding's posture-hold case runs on
REAL_MODEL, REAL_T = "jaco2_curtain_torque", 50


def real_inputs():
    """The realistic set: A, B of the emulated linearize (emu_sim.EmuSim) of the default model's nine hinge joints -- the arm's six
    and the three fingers, whose position servos are part of A; u is the six motor words, linearize's convention -- at
    rollout_fb_binding's posture-hold states around gravity compensation, repeated over REAL_T knots, with that case's weights on the
    angles, the velocities and the torques; the gradients drawn as in the other sets.  (nx, nu) = (18, 6)."""
    import rollout_fb_binding as fbb
    from emu_sim import EmuSim
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    q, v = fbb.hold_postures(REAL_MODEL)
    cfg = BatchedMujocoConfig(EmuSim(REAL_MODEL, q, v), ee="EE")
    M, names = cfg.table.M, cfg.table.names["joint"]
    hinge = [names[j] for j in range(len(names)) if M["jnt_type"][j] == 3]
    A, Bm, _ = cfg.linearize(joints=hinge, ctrl=cfg.joint(joints=None).gravity_compensation())
    A, Bm = A.numpy()[:3], Bm.numpy()[:3]
    n, m = A.shape[1] // 2, Bm.shape[2]
    assert (n, m) == (9, 6)
    rng = np.random.default_rng(97)
    Q = np.diag([fbb.HOLD_Q] * n + [fbb.HOLD_QV] * n)
    return dict(A=np.repeat(A[:, None], REAL_T, 1), B=np.repeat(Bm[:, None], REAL_T, 1), lxx=Q, luu=fbb.HOLD_R * np.eye(m),
                lux=np.zeros((3, REAL_T, m, 2 * n)), lx=rng.uniform(-1, 1, (3, REAL_T, 2 * n)), lu=1e-3 * rng.uniform(-1, 1, (3, REAL_T, m)), Vxx=Q,
                Vx=rng.uniform(-1, 1, (3, 2 * n)))


def full(inp, problem_index=None):
    """Every array of an input set with all its axes, fp64: A [P, T, ..], the cost arrays [P, T, ..], the terminal ones [P, ..]; None: zeros.
    problem_index: the problems gathered, one per solve."""
    A = np.asarray(inp["A"], np.float64)
    P, T, nx, nu = A.shape[0], A.shape[1], A.shape[2], inp["B"].shape[3]
    tails = dict(lxx=(nx, nx), luu=(nu, nu), lux=(nu, nx), lx=(nx,), lu=(nu,), Vxx=(nx, nx), Vx=(nx,))
    F = dict(A=A, B=np.asarray(inp["B"], np.float64))
    for k, tail in tails.items():
        lead = (P,) if k in ("Vxx", "Vx") else (P, T)
        a = inp.get(k)
        if a is None and k == "Vxx":
            a = F["lxx"][:, -1]
        a = np.zeros(tail) if a is None else np.asarray(a, np.float64)
        missing = len(lead) + len(tail) - a.ndim
        F[k] = np.broadcast_to(a.reshape(a.shape[:a.ndim - len(tail)] + (1,) * missing + tail) if a.ndim > len(tail) else a, lead + tail).copy()
    if problem_index is not None:
        F = {k: v[np.asarray(problem_index)] for k, v in F.items()}
    return F


def reference(inp, mu=None, problem_index=None):
    """The recursion in fp64: {"gain" [n, T, nu, nx], "kff", "dV", "Vxx0", "Vx0", "pivot" [n, T]: each knot's smallest Cholesky pivot^2
    over max diag(Quu)}.  numpy.linalg.LinAlgError where Quu + mu I is not positive definite."""
    F = full(inp, problem_index)
    n, T, nx, nu = F["A"].shape[0], F["A"].shape[1], F["A"].shape[2], F["B"].shape[3]
    mu = np.broadcast_to(np.zeros(()) if mu is None else np.asarray(mu, np.float64), (n,))
    R = dict(gain=np.zeros((n, T, nu, nx)), kff=np.zeros((n, T, nu)), dV=np.zeros((n, 2)), Vxx0=np.zeros((n, nx, nx)), Vx0=np.zeros((n, nx)),
             pivot=np.zeros((n, T)))
    for i in range(n):
        Vxx, Vx = F["Vxx"][i], F["Vx"][i]
        for t in range(T - 1, -1, -1):
            A, B = F["A"][i, t], F["B"][i, t]
            Qx, Qu = F["lx"][i, t] + A.T @ Vx, F["lu"][i, t] + B.T @ Vx
            Qxx, Qux, Quu = F["lxx"][i, t] + A.T @ Vxx @ A, F["lux"][i, t] + B.T @ Vxx @ A, F["luu"][i, t] + B.T @ Vxx @ B
            M = Quu + mu[i] * np.eye(nu)
            R["pivot"][i, t] = (np.diag(np.linalg.cholesky(M)) ** 2).min() / np.abs(np.diag(Quu)).max()
            K, k = -np.linalg.solve(M, Qux), -np.linalg.solve(M, Qu)
            R["dV"][i] += (k @ Qu, 0.5 * k @ Quu @ k)
            Vx = Qx + K.T @ Quu @ k + K.T @ Qu + Qux.T @ k
            Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
            Vxx = 0.5 * (Vxx + Vxx.T)
            R["gain"][i, t], R["kff"][i, t] = K, k
        R["Vxx0"][i], R["Vx0"][i] = Vxx, Vx
    return R


def ref(name):
    """The fp64 reference of an input set at mu = 0, computed once, the inputs' condition asserted."""
    if name not in _refs:
        _refs[name] = reference(inputs(name))
        assert _refs[name]["pivot"].min() >= MIN_PIVOT, (name, _refs[name]["pivot"].min())
    return _refs[name]


# ---- measures
QUANT = ("gain", "kff", "Vxx0", "Vx0", "dV")


def rel(x, r, axes):
    """max over the leading axes of  max |x - ref| / max |ref|  over the trailing `axes`."""
    ax = tuple(range(-axes, 0))
    return float((np.abs(x.astype(np.float64) - r).max(ax) / np.abs(r).max(ax)).max())


def measures(res, r):
    """Case 1's five figures: K and k per knot, Vxx0 and Vx0 per solve, |dV / dV_ref - 1| per entry."""
    return dict(gain=rel(res["gain"], r["gain"], 2), kff=rel(res["kff"], r["kff"], 1), Vxx0=rel(res["Vxx0"], r["Vxx0"], 2), Vx0=rel(res["Vx0"], r["Vx0"], 1),
                dV=float(np.abs(res["dV"].astype(np.float64) / r["dV"] - 1).max()))


# ---- cases
def case_reference(sim, name):
    """Case 1: against the fp64 recursion."""
    res = call(sim, inputs(name))
    assert (res["status"] == 0).all(), res["status"]
    return measures(res, ref(name))


def lqr_form(name):
    """The degenerate form of an input set: no gradients, no cross term, Q, R and Qf."""
    g = inputs(name)
    return dict(A=g["A"], B=g["B"], lxx=g["lxx"], luu=g["luu"], Vxx=g["Vxx"])


def case_lqr(sim, name):
    """Case 2: K against robot_config.lqr_gains evaluated in fp64; k, dV and Vx0 are exactly zero."""
    import torch
    from mujoco_jaco_amd.robot_config import lqr_gains
    g = lqr_form(name)
    res = call(sim, g)
    assert (res["status"] == 0).all()
    D = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    K = lqr_gains(D(g["A"]), D(g["B"]), D(g["lxx"]), D(g["luu"]), D(g["Vxx"])).numpy()
    assert not res["kff"].any() and not res["dV"].any() and not res["Vx0"].any()
    return rel(res["gain"], K, 2)


def policy_cost(F, K, k, x0):
    """The fp64 cost of u = k + K x on problem i of the full arrays F from x0 [n, nx]: [n]."""
    n, T = F["A"].shape[:2]
    J = np.zeros(n)
    for i in range(n):
        x = x0[i].astype(np.float64)
        for t in range(T):
            u = k[i, t] + K[i, t] @ x
            J[i] += 0.5 * x @ F["lxx"][i, t] @ x + 0.5 * u @ F["luu"][i, t] @ u + u @ F["lux"][i, t] @ x + F["lx"][i, t] @ x + F["lu"][i, t] @ u
            x = F["A"][i, t] @ x + F["B"][i, t] @ u
        J[i] += 0.5 * x @ F["Vxx"][i] @ x + F["Vx"][i] @ x
    return J


def case_optimality(sim, name):
    """Case 3: the linear system simulated in fp64 under the kernel's (k, K) at alpha = 1, from dx0 = 0 and from a random dx0.  Returns
    (the smallest and the largest relative excess of its cost over the fp64 optimum -- the reference's policy simulated the same way --,
    the largest |cost change from dx0 = 0 / (dV1 + dV2) - 1|)."""
    g, r = inputs(name), ref(name)
    res = call(sim, g)
    F = full(g)
    n, nx = F["A"].shape[0], F["A"].shape[2]
    K, k = res["gain"].astype(np.float64), res["kff"].astype(np.float64)
    excess = []
    for x0 in (np.zeros((n, nx)), np.random.default_rng(5).uniform(-0.1, 0.1, (n, nx))):
        J, Jopt = policy_cost(F, K, k, x0), policy_cost(F, r["gain"], r["kff"], x0)
        excess.append((J - Jopt) / np.abs(Jopt))
    J0 = policy_cost(F, K, k, np.zeros((n, nx)))
    return float(np.min(excess)), float(np.max(excess)), float(np.abs(J0 / res["dV"].astype(np.float64).sum(1) - 1).max())


def case_layout(sim, name="10x3x7"):
    """Case 4: the scatter, the fan-out, the shared axes, the same call twice, NULL against zeros -- all bit for bit."""
    g = inputs(name)
    P, T, nx, nu = g["A"].shape[0], g["A"].shape[1], g["A"].shape[2], g["B"].shape[3]
    dense = call(sim, g)
    assert (dense["status"] == 0).all()
    assert same(dense, call(sim, g)), "the same call twice"
    # rows_out / row: a gather of the dense result; the other rows keep the fill
    R = nu + 3
    rows = [int(r) for r in np.random.default_rng(3).permutation(R)[:nu]]
    assert len(set(rows)) == nu and min(rows) >= 0 and max(rows) < R
    sc = call(sim, g, rows=rows, rows_out=R)
    assert (bits(sc["gain"][:, :, rows]) == bits(dense["gain"])).all() and (bits(sc["kff"][:, :, rows]) == bits(dense["kff"])).all()
    rest = [r for r in range(R) if r not in rows]
    assert (bits(sc["gain"][:, :, rest]) == bits(FILL)).all() and (bits(sc["kff"][:, :, rest]) == bits(FILL)).all()
    assert same(sc, dense, ("dV", "Vxx0", "Vx0", "status"))
    # prob_idx fan-out with a mu per solve against materialised problems
    idx, mu = np.array([2, 0, 1, 0, 2], np.int32), np.array([0.0, 1e-3, 0.0, 0.0, 5e-4], np.float32)
    fan = call(sim, g, problem_index=idx, mu=mu)
    mat = {k: (v[idx] if k in ("A", "B", "lux", "lx", "lu", "Vx") else v) for k, v in g.items()}
    assert (fan["status"] == 0).all() and same(fan, call(sim, mat, mu=mu)), "fan-out"
    assert same({k: v[[3]] for k, v in fan.items()}, {k: v[[0]] for k, v in dense.items()}) and not same({k: v[[1]] for k, v in fan.items()}, {k: v[[0]] for k, v in dense.items()})
    # shared axes against materialised arrays: none, the knot axis, the problem axis (a leading 1), both
    F = {k: v.astype(np.float32) for k, v in full(g).items()}
    assert same(dense, call(sim, F)), "shared axes: lxx, luu, Vxx without axes against [P, T, ..] / [P, ..]"
    per_prob = dict(F, lx=F["lx"][:, 0].copy(), lu=F["lu"][:, 0].copy(), lux=F["lux"][:, 0].copy())
    m1 = call(sim, per_prob)
    assert same(m1, call(sim, {k: (np.repeat(v[:, None], T, 1) if k in ("lx", "lu", "lux") else v) for k, v in per_prob.items()})), "no knot axis"
    per_knot = dict(F, lx=F["lx"][:1].copy(), lu=F["lu"][:1].copy(), lux=F["lux"][:1].copy(), lxx=F["lxx"][:1].copy(), Vx=F["Vx"][:1].copy())
    m2 = call(sim, per_knot)
    assert same(m2, call(sim, {k: (np.repeat(v, P, 0) if k in ("lx", "lu", "lux", "lxx", "Vx") else v) for k, v in per_knot.items()})), "no problem axis"
    assert not same(m1, dense, VALUES) and not same(m2, dense, VALUES)
    # an axis of length 1 is the dropped axis: [P, 1, ..] = [P, ..], [1, 1, ..] = [..]
    one_knot = {k: (v[:, None].copy() if k in ("lx", "lu", "lux") else v) for k, v in per_prob.items()}
    assert one_knot["lx"].shape == (P, 1, nx) and same(m1, call(sim, one_knot)), "a knot axis of length 1"
    both = dict(g, lx=g["lx"][:1, :1].copy(), lu=g["lu"][0, 0].copy(), lxx=g["lxx"][None, None].copy(), luu=g["luu"][None].copy(), Vxx=None)
    flat = dict(g, lx=np.broadcast_to(g["lx"][:1, :1], (P, T, nx)).copy(), lu=np.broadcast_to(g["lu"][0, 0], (P, T, nu)).copy(), Vxx=g["lxx"])
    assert both["lx"].shape == (1, 1, nx) and both["lxx"].shape == (1, 1, nx, nx) and same(call(sim, both), call(sim, flat)), "both axes of length 1"
    # a NULL lux / lx / lu / Vx against explicit zeros
    none = dict(g, lux=None, lx=None, lu=None, Vx=None)
    zero = dict(g, lux=np.zeros_like(g["lux"]), lx=np.zeros_like(g["lx"]), lu=np.zeros_like(g["lu"]), Vx=np.zeros_like(g["Vx"]))
    assert same(call(sim, none), call(sim, zero)), "NULL against zeros"
    some = dict(g, lux=None, Vx=None)
    assert same(call(sim, some), call(sim, dict(zero, lx=g["lx"], lu=g["lu"]))), "NULL lux and Vx against zeros"


FAIL_MU = 2.0


def case_failure(sim, bounds, name="10x3x7"):
    """Case 5: regularisation and failure.  Returns the measures of the regularised solve."""
    g = inputs(name)
    P, T, nx, nu = g["A"].shape[0], g["A"].shape[1], g["A"].shape[2], g["B"].shape[3]
    dense = call(sim, g)
    untouched = lambda r, i, keys=VALUES: all((bits(r[k][i]) == bits(FILL)).all() for k in keys)
    others = lambda r, i: same({k: np.delete(v, i, 0) for k, v in r.items()}, {k: np.delete(v, i, 0) for k, v in dense.items()})
    # luu = -I on problem 1 of three
    luu = np.repeat(g["luu"][None], P, 0)
    luu[1] = -np.eye(nu, dtype=np.float32)
    neg = dict(g, luu=luu)
    try:
        reference(neg)
        raise AssertionError("the fp64 recursion found luu = -I positive definite")
    except np.linalg.LinAlgError:
        pass
    r = call(sim, neg)
    assert r["status"][1] == (NOT_PD | (T - 1)), hex(r["status"][1])
    assert untouched(r, 1) and others(r, 1)
    # ... and with mu large enough, against the fp64 recursion at that mu
    mu = np.array([0.0, FAIL_MU, 0.0], np.float32)
    rm = reference(neg, mu=mu.astype(np.float64))
    assert rm["pivot"].min() >= MIN_PIVOT, rm["pivot"].min()
    r = call(sim, neg, mu=mu)
    assert (r["status"] == 0).all() and others(r, 1)
    m = measures({k: v[[1]] for k, v in r.items()}, {k: v[[1]] for k, v in rm.items()})
    # a NaN in A at knot t: the rows of the knots > t stand, nothing else is written
    t = 3
    A = g["A"].copy()
    A[1, t, 2, 5] = np.nan
    r = call(sim, dict(g, A=A))
    assert r["status"][1] == (NOT_PD | t), hex(r["status"][1])
    assert (bits(r["gain"][1, t + 1:]) == bits(dense["gain"][1, t + 1:])).all() and (bits(r["kff"][1, t + 1:]) == bits(dense["kff"][1, t + 1:])).all()
    assert (bits(r["gain"][1, :t + 1]) == bits(FILL)).all() and (bits(r["kff"][1, :t + 1]) == bits(FILL)).all() and untouched(r, 1, ("dV", "Vxx0", "Vx0"))
    assert others(r, 1)
    # a bad index: its status word and nothing else
    idx = np.array([0, P, -1, 2], np.int32)
    r = call(sim, g, problem_index=idx)
    assert (r["status"] == [0, BAD_INDEX, BAD_INDEX, 0]).all(), r["status"]
    assert untouched(r, 1) and untouched(r, 2)
    assert same({k: v[[0, 3]] for k, v in r.items()}, {k: v[[0, 2]] for k, v in dense.items()})
    return m


# ---- case 6: the refusals.  (what to change in the records of a good call, what the message says)
REFUSALS = {
    "no_options": (lambda c: c.update(opt=None), "the options, the problem and the outputs are required"),
    "no_problem": (lambda c: c.update(prob=None), "the options, the problem and the outputs are required"),
    "no_out": (lambda c: c.update(out=None), "the options, the problem and the outputs are required"),
    "nknots_0": (lambda c: setattr(c["opt"], "nknots", 0), r"nknots 0 outside \[1, 16384\]"),
    "nknots_big": (lambda c: setattr(c["opt"], "nknots", 16385), r"nknots 16385 outside \[1, 16384\]"),
    "nx_0": (lambda c: setattr(c["opt"], "nx", 0), r"nx 0 outside \[1, 36\]"),
    "nx_big": (lambda c: setattr(c["opt"], "nx", 37), r"nx 37 outside \[1, 36\]"),
    "nu_0": (lambda c: setattr(c["opt"], "nu", 0), r"nu 0 outside \[1, 18\]"),
    "nu_big": (lambda c: setattr(c["opt"], "nu", 19), r"nu 19 outside \[1, 18\]"),
    "n_negative": (lambda c: c.update(n=-1), "n -1 is negative"),
    "nprob_0": (lambda c: setattr(c["prob"], "nprob", 0), "nprob 0: at least one problem is required"),
    "n_over_nprob": (lambda c: c.update(n=3), "n 3 solves of 2 problems without a problem index"),
    "no_A": (lambda c: setattr(c["prob"], "A", None), "A, B, lxx, luu and the terminal Vxx are required"),
    "no_B": (lambda c: setattr(c["prob"], "B", None), "A, B, lxx, luu and the terminal Vxx are required"),
    "no_lxx": (lambda c: setattr(c["prob"], "lxx", None), "A, B, lxx, luu and the terminal Vxx are required"),
    "no_luu": (lambda c: setattr(c["prob"], "luu", None), "A, B, lxx, luu and the terminal Vxx are required"),
    "no_Vxx": (lambda c: setattr(c["prob"], "Vxx", None), "A, B, lxx, luu and the terminal Vxx are required"),
    "status_only": (lambda c: [setattr(c["out"], k, None) for k in VALUES], "at least one of the outputs gain, kff, dV, Vxx0 and Vx0 is required"),
    "rows_out_small": (lambda c: setattr(c["opt"], "rows_out", 1), r"rows_out 1 outside \[nu = 2, 64\]"),
    "rows_out_big": (lambda c: setattr(c["opt"], "rows_out", 65), r"rows_out 65 outside \[nu = 2, 64\]"),
    "row_out_of_range": (lambda c: (setattr(c["opt"], "rows_out", 4), c["opt"].row.__setitem__(1, 4)), r"row 4 outside \[0, 4\)"),
    "row_negative": (lambda c: (setattr(c["opt"], "rows_out", 4), c["opt"].row.__setitem__(0, -1)), r"row -1 outside \[0, 4\)"),
    "row_twice": (lambda c: (setattr(c["opt"], "rows_out", 4), c["opt"].row.__setitem__(0, 3), c["opt"].row.__setitem__(1, 3)), "row 3 is listed twice"),
    "mask_knots": (lambda c: setattr(c["opt"], "shared_knots", 128), "a shared-axis mask has a bit outside the seven named"),
    "mask_probs": (lambda c: setattr(c["opt"], "shared_probs", 1 | 256), "a shared-axis mask has a bit outside the seven named"),
}


def case_refusal(sim, case):
    """One refusal through sim.raw (the entry as it is) on a good call's records: JACO_EINVAL, the entry's name and the reason in the
    message, no output touched.  Returns the message."""
    import re
    import torch
    g = inputs("7x2x3")
    P, T, nx, nu = 2, 3, 7, 2
    rows = 4   # (room for the scattered cases)
    dev = {k: torch.as_tensor(np.ascontiguousarray(v[:P] if v.ndim > 2 else v), device=sim.device) for k, v in g.items()}
    sh = shapes(P + 1, T, rows, nx)
    out = {k: torch.full(sh[k], float(FILL), dtype=torch.float32, device=sim.device) for k in VALUES}
    out["status"] = torch.from_numpy(np.full(sh["status"], STATUS_FILL, np.uint32).view(np.int32)).to(sim.device)
    S = product_lib.JACO_LQR_SHARED
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    c = dict(opt=product_lib.JacoLqrOptions(nknots=T, nx=nx, nu=nu, shared_knots=S["lxx"] | S["luu"], shared_probs=S["lxx"] | S["luu"] | S["Vxx"]),
             prob=product_lib.JacoLqrProblem(*[ptr(dev[k]) for k in ("A", "B", "lxx", "luu", "lux", "lx", "lu", "Vxx", "Vx")], None, None, P),
             out=product_lib.JacoLqrOut(*[ptr(out[k]) for k in OUTS]), n=P)
    change, message = REFUSALS[case]
    change(c)
    rc, why = sim.raw(c["opt"], c["n"], c["prob"], c["out"])
    assert rc == -1, (case, rc)   # JACO_EINVAL
    assert why.startswith("jaco_lqr: ") and re.search(message, why), (case, why)
    for k in VALUES:
        assert (bits(out[k].cpu().numpy()) == bits(FILL)).all(), (case, k)
    assert (out["status"].cpu().numpy().view(np.uint32) == STATUS_FILL).all(), case
    return why


# ---- the robot_config tier.  make_sim(model, qpos, qvel) -> a BatchedMujoco (GPU tier) or emu_sim.EmuSim.
CONFIG_T = 12


def case_config(make_sim):
    """BatchedMujocoConfig.lqr against lqr_gains in fp64 on the arm's linearisation at rollout_fb_binding's posture-hold states (that
    case's weights, CONFIG_T knots), and ilqr_backward with and without full=True: the scattered rows are the dense ones bit for bit,
    the other rows zero.  Returns case 1's measure of K."""
    import torch
    import rollout_fb_binding as fbb
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, lqr_gains
    q, v = fbb.hold_postures(ARM_MODEL)
    sim = make_sim(ARM_MODEL, q, v)
    cfg = BatchedMujocoConfig(sim, ee=fbb.HOLD_MODELS[ARM_MODEL])
    A, Bm, _ = cfg.linearize(ctrl=cfg.joint(joints=None).gravity_compensation())
    Bn, nx, m = A.shape[0], A.shape[1], Bm.shape[2]
    acts = cfg._joint_subset(None, "case_config")[2]
    At, Bt = A[:, None].expand(-1, CONFIG_T, -1, -1).contiguous(), Bm[:, None].expand(-1, CONFIG_T, -1, -1).contiguous()
    Q = torch.diag(torch.tensor([fbb.HOLD_Q] * (nx // 2) + [fbb.HOLD_QV] * (nx // 2), dtype=torch.float64))
    R = fbb.HOLD_R * torch.eye(m, dtype=torch.float64)
    K = cfg.lqr(At, Bt, Q, R, Q)
    assert K.shape == (Bn, CONFIG_T, m, nx) and K.dtype == torch.float32
    Kref = lqr_gains(At.double().cpu(), Bt.double().cpu(), Q, R, Q).numpy()
    K2, st = cfg.lqr(At, Bt, Q, R, Q, status=True)
    assert st.shape == (Bn,) and not st.cpu().numpy().any() and (bits(K2.cpu().numpy()) == bits(K.cpu().numpy())).all()
    Kbad, st = cfg.lqr(At, Bt, Q, -R, Q, status=True)   # R = -1e-3 I against B'P B of the order of 1e-5: not positive definite at the last knot
    assert (st.cpu().numpy().view(np.uint32) == (NOT_PD | (CONFIG_T - 1))).all() and not Kbad.cpu().numpy().any()
    lx = torch.as_tensor(np.random.default_rng(12).uniform(-1, 1, (Bn, CONFIG_T, nx)).astype(np.float32), device=sim.device)
    args = (At, Bt, Q.float(), R.float())
    Kd, kd, dV, st = cfg.ilqr_backward(*args, lx=lx, mu=1e-3 * fbb.HOLD_R)
    Kf, kf, dVf, stf = cfg.ilqr_backward(*args, lx=lx, mu=1e-3 * fbb.HOLD_R, full=True)
    N = lambda t: t.cpu().numpy()
    assert Kd.shape == (Bn, CONFIG_T, m, nx) and kd.shape == (Bn, CONFIG_T, m) and dV.shape == (Bn, 2) and st.shape == (Bn,)
    assert Kf.shape == (Bn, CONFIG_T, sim.nu, nx) and kf.shape == (Bn, CONFIG_T, sim.nu)
    assert not N(st).any() and not N(stf).any() and (N(dV)[:, 0] < 0).all()
    rest = [a for a in range(sim.nu) if a not in acts]
    assert (bits(N(Kf)[:, :, acts]) == bits(N(Kd))).all() and (bits(N(kf)[:, :, acts]) == bits(N(kd))).all() and (bits(N(dVf)) == bits(N(dV))).all()
    assert not N(Kf)[:, :, rest].any() and not N(kf)[:, :, rest].any()
    return rel(N(K), Kref, 2)


# ---- case 7: the loop closed through robot_config (the GPU tier runs these)
def case_hold(make_sim):
    """Case 7a: rollout_fb_binding.case_hold_posture's plan, the gains from robot_config.lqr instead of lqr_gains.  Returns fd_binding.verr
    of the two closed loops' joint angles and velocities."""
    import torch
    import rollout_fb_binding as fbb
    from fd_binding import verr
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig, lqr_gains
    model = ARM_MODEL
    q, v = fbb.hold_postures(model)
    sim = make_sim(model, q, v)
    cfg = BatchedMujocoConfig(sim, ee=fbb.HOLD_MODELS[model])
    arm, qadr = list(cfg.arm), list(cfg.arm_qadr)
    n = len(arm)
    ubar_full = cfg.joint(joints=None).gravity_compensation()
    A, Bm, _ = cfg.linearize(ctrl=ubar_full)
    acts = cfg._joint_subset(None, "test")[2]
    m = len(acts)
    Q = torch.diag(torch.tensor([fbb.HOLD_Q] * n + [fbb.HOLD_QV] * n, dtype=torch.float64))
    R = fbb.HOLD_R * torch.eye(m, dtype=torch.float64)
    At, Bt = A[:, None].expand(-1, fbb.HOLD_HORIZON, -1, -1), Bm[:, None].expand(-1, fbb.HOLD_HORIZON, -1, -1)
    tail = lambda K: torch.cat([K, K[:, -1:].expand(-1, fbb.HOLD_KNOTS - fbb.HOLD_HORIZON, -1, -1)], 1).float().to(sim.device).contiguous()
    K64, K32 = tail(lqr_gains(At.double(), Bt.double(), Q.to(sim.device), R.to(sim.device), Q.to(sim.device))), tail(cfg.lqr(At, Bt, Q, R, Q))
    u = ubar_full[:, acts][:, None].expand(-1, fbb.HOLD_KNOTS, -1).contiguous()
    xbar = torch.cat([torch.as_tensor(q[:, qadr]), torch.as_tensor(v[:, arm])], 1).to(sim.device)
    x_ref = xbar[:, None].expand(-1, fbb.HOLD_KNOTS, -1).contiguous()
    q0 = torch.as_tensor(q[:, qadr] + np.float32(fbb.HOLD_OFF)).to(sim.device)
    k = dict(ctrl=ubar_full, hold=fbb.HOLD_SUBSTEPS, per_substep=True, q=q0)
    r64, r32 = cfg.rollout_feedback(u, K=K64, x_ref=x_ref, **k), cfg.rollout_feedback(u, K=K32, x_ref=x_ref, **k)
    N = lambda t: t.cpu().numpy()
    assert not N(r64["status"]).any() and not N(r32["status"]).any()
    last = np.abs(N(r32["q"])[:, -1].astype(np.float64) - q[:, qadr]).max(1)
    assert (last < fbb.HOLD_OFF).all(), last
    eq, ev = verr(N(r32["q"]), N(r64["q"])), verr(N(r32["dq"]), N(r64["dq"]))
    getattr(sim, "close", lambda: None)()
    return eq, ev


ILQR_B, ILQR_T = 8, 16
WQ, WV, WU, WF, GOAL_OFF = 100.0, 1.0, 1e-2, 1000.0, 0.1


def case_ilqr(make_sim):
    """Case 7b: linearize -> ilqr_backward(full=True) -> rollout_feedback with eight step sizes on jaco2_reaching_torque, 8 envs x 16 knots x
    hold 1, around gravity compensation at the workload's reset postures (no status flag: no joint limit is met), under a quadratic
    joint-space goal cost plus effort: the backward pass succeeds, predicts a decrease (dV1 < 0), and for every env at least one
    step size lowers the TRUE cost of the nonlinear rollout below the nominal's (asserted by the caller).  Returns (the nominal's cost
    [B], the cost at every step size [B, 8], dV [B, 2], the backward pass's status [B])."""
    import torch
    import osc_binding as ob
    import rollout_fb_binding as fbb
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    model = ARM_MODEL
    q, _ = ob.states(model, ILQR_B)
    q, v = q.astype(np.float32), np.zeros((ILQR_B, int(fbb.ib.load_model(model)["nv"][0])), np.float32)
    sim = make_sim(model, q, v)
    cfg = BatchedMujocoConfig(sim, ee="EE")
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    n, m, nu, dev = len(dofs), len(acts), sim.nu, sim.device
    ubar = cfg.joint(joints=None).gravity_compensation()                      # [B, nu]
    nominal = ubar[:, None].expand(-1, ILQR_T, -1).contiguous()               # [B, T, nu]
    r0 = sim.rollout(nominal)
    assert not r0["status"].cpu().numpy().any()
    qpos0, qvel0, _ = sim.get_state()
    # the state BEFORE each knot (x_0 .. x_{T-1}) and after the last (x_T)
    qk = torch.cat([qpos0[:, None], r0["qpos"]], 1)                           # [B, T + 1, nq]
    vk = torch.cat([qvel0[:, None], r0["qvel"]], 1)
    X = torch.cat([qk[..., qadr], vk[..., dofs]], -1)                         # [B, T + 1, 2 n]
    goal = qpos0[:, qadr] + GOAL_OFF

    def cost(X, U):
        """[..] true cost of states X [.., T + 1, 2 n] under the motor words U [.., T, m], in fp64."""
        X, U, g = X.double(), U.double(), goal.double()
        while g.dim() < X.dim() - 1:
            g = g[:, None]
        e = X[..., :n] - g[..., None, :]
        run = 0.5 * WQ * (e[..., :-1, :] ** 2).sum(-1) + 0.5 * WV * (X[..., :-1, n:] ** 2).sum(-1) + 0.5 * WU * (U ** 2).sum(-1)
        return run.sum(-1) + 0.5 * WF * (e[..., -1, :] ** 2).sum(-1) + 0.5 * WV * (X[..., -1, n:] ** 2).sum(-1)
    J0 = cost(X, nominal[..., acts])
    # the linearisation at every knot state: a second handle of B x T envs holding them
    sim2 = make_sim(model, qk[:, :-1].reshape(-1, sim.nq).cpu().numpy(), vk[:, :-1].reshape(-1, sim.nv).cpu().numpy())
    A, Bm, _ = BatchedMujocoConfig(sim2, ee="EE").linearize(ctrl=nominal.reshape(-1, nu))
    A, Bm = A.reshape(ILQR_B, ILQR_T, 2 * n, 2 * n), Bm.reshape(ILQR_B, ILQR_T, 2 * n, m)
    getattr(sim2, "close", lambda: None)()
    # the cost's expansion along the nominal
    w = torch.tensor([WQ] * n + [WV] * n, device=dev)
    wf = torch.tensor([WF] * n + [WV] * n, device=dev)
    D = X.clone()
    D[..., :n] -= goal[:, None]
    luu = WU * torch.eye(m, device=dev)
    gain, kff, dV, status = cfg.ilqr_backward(A, Bm, torch.diag(w), luu, lx=w * D[:, :-1], lu=WU * nominal[..., acts], Vxx=torch.diag(wf), Vx=wf * D[:, -1],
                                              mu=1e-3 * WU, full=True)
    assert gain.shape == (ILQR_B, ILQR_T, nu, 2 * n) and kff.shape == (ILQR_B, ILQR_T, nu)
    dV, status = dV.cpu().numpy(), status.cpu().numpy()
    # the line search: every env's plan at eight step sizes, plan and state shared through the indices
    alphas = torch.tensor([2.0 ** -i for i in range(8)], device=dev)
    idx = torch.arange(ILQR_B, dtype=torch.int32, device=dev).repeat_interleave(len(alphas))
    r = sim.rollout_feedback(nominal, gain=gain, x_ref=X[:, :-1].contiguous(), dofs=dofs, feedforward=kff, alpha=alphas.repeat(ILQR_B), plan_index=idx,
                             state_index=idx)
    assert not r["status"].cpu().numpy().any()
    Xa = torch.cat([torch.cat([qpos0[idx.long()][:, None], r["qpos"]], 1)[..., qadr], torch.cat([qvel0[idx.long()][:, None], r["qvel"]], 1)[..., dofs]], -1)
    goal = goal[idx.long()]
    J = cost(Xa, r["ctrl"][..., acts]).reshape(ILQR_B, len(alphas)).cpu().numpy()
    getattr(sim, "close", lambda: None)()
    return J0.cpu().numpy(), J, dV, status
