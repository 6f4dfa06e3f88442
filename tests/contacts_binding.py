"""The oracle side of the contact record, and how to read the emulator's (emu_binding.EmuEnv.step_rec) -- TEST INFRASTRUCTURE ONLY.
Shared by the CPU tests (tests/test_contacts_emu.py) and the GPU tests (tests/test_gpu_contacts.py).

Record layout: include/jaco_env.h JacoContact = 19 floats (dist, pos[3], frame[9], force[6]) then 5 int32 (geom[2], body[2], dim)."""
import numpy as np

NF = 19   # float words of a record; then geom[2], body[2], dim


def unpack(rec, ncon):
    """[nenv][cap][24] float32 words -> dict of numpy fields (all slots; slot < min(ncon, cap) is valid)."""
    f = rec[..., :NF]
    i = rec.view(np.int32)[..., NF:]
    return {"ncon": ncon.copy(), "dist": f[..., 0], "pos": f[..., 1:4], "frame": f[..., 4:13].reshape(*f.shape[:-1], 3, 3), "force": f[..., 13:19],
            "geom": i[..., 0:2], "body": i[..., 2:4], "dim": i[..., 4]}


def oracle_contacts(o, M):
    """The oracle's contacts after its forward(): {"ncon", "dist", "pos", "normal", "geom" (MJCF, [n, 2]), "dim", "force" [n, 6]} -- force is
    mj_contactForce for the pyramidal cone restated from efc_force / efc_address / dim and the pair's friction (element-wise max of the
    two geoms' geom_friction: mu = (f0, f0, f1, f2, f2))."""
    C = o.get("contact").reshape(-1, 11)
    ef = o.get("efc_force") if o.nefc else np.zeros(0)
    fr = M["geom_friction"].reshape(-1, 3)
    n = len(C)
    force = np.zeros((n, 6))
    for c in range(n):
        g1, g2, dim, adr = int(C[c, 7]), int(C[c, 8]), int(C[c, 9]), int(C[c, 10])
        f3 = np.maximum(fr[g1], fr[g2])
        mu = [f3[0], f3[0], f3[1], f3[2], f3[2]]
        if dim == 1:
            force[c, 0] = ef[adr]
        else:
            p = ef[adr:adr + 2 * (dim - 1)]
            force[c, 0] = p.sum()
            for k in range(1, dim):
                force[c, k] = mu[k - 1] * (p[2 * k - 2] - p[2 * k - 1])
    return {"ncon": n, "dist": C[:, 0], "pos": C[:, 1:4], "normal": C[:, 4:7], "geom": C[:, 7:9].astype(int), "dim": C[:, 9].astype(int), "force": force}


def match(rec_env, ncon, oc, gmap, geom_type):
    """Pairs every recorded contact of one env with an oracle contact: same MJCF geom pair (either order: equal-type pairs may be listed
    the other way round, then the normal is flipped), then the nearest position.  Returns a list of (record slot, oracle index, sign)."""
    out, used = [], set()
    for k in range(ncon):
        g = tuple(int(gmap[x]) for x in rec_env["geom"][k])
        best = None
        for j in range(oc["ncon"]):
            if j in used:
                continue
            og = tuple(oc["geom"][j])
            if og == g:
                s = 1.0
            elif og == g[::-1]:
                s = -1.0
            else:
                continue
            d = np.abs(oc["pos"][j] - rec_env["pos"][k]).max()
            if best is None or d < best[0]:
                best = (d, j, s)
        assert best is not None, ("no oracle contact for recorded pair", g)
        used.add(best[1])
        out.append((k, best[1], best[2]))
    return out


# ---- the seeded states of the parity tests (jaco2_curtain_torque), fp32-rounded: the kernel and the oracle get the same numbers.  The
# pedestal sits 0.1 mm into the floor: at the XML's 0.09 its bottom face is exactly at z = 0, a knife edge that fp32 rounding of the
# height decides (workload.reset_states)
GRASP_CTRL = np.array([0, 0, 0, 0, 0, 0, 1.0, 1.0, 1.0])


def _f32(q):
    return np.asarray(q, np.float64).astype(np.float32).astype(np.float64)


def rest_states(M, n, seed=3):
    """The picking reset: object on its holder (box on box, 4 contacts), pedestal on the floor (plane-box, 4)."""
    q = workload_reset(M, n, seed)
    q[:, 18] = 0.0899
    return _f32(q)


def workload_reset(M, n, seed):
    from mujoco_jaco_amd import workload
    return workload.reset_states(M["qpos0"], n, seed=seed, f32_draws=True)


def grasp_state(M, names, substeps=40):
    """Fingers closed on the object: the placing reset's hold pose (object in the grasp frame EE_obj, 4 cm back), then `substeps` oracle
    substeps with the grip closing (hull contacts of condim 6 on the finger pads, box contacts on the holder)."""
    from mujoco_jaco_amd.modelc import rot
    from oracle_binding import Oracle
    o = Oracle()
    q = M["qpos0"].copy()
    q[:6] = [1.3, 3.85, 1.05, 2.05, 1.5, -1.15]; q[6:9] = 0.6; q[16:18] = [.4, .3]; q[18] = 0.0899
    o.set("qpos", q); o.forward()
    b = names["body"].index("EE_obj")
    xp = o.get("xpos").reshape(-1, 3)[b]; xq = o.get("xquat").reshape(-1, 4)[b]
    q[9:12] = xp + rot.quat_to_mat(xq) @ np.array([-0.04, 0, 0]); q[12:16] = xq
    o.set("qpos", q)
    o.step(GRASP_CTRL, n=substeps)
    return _f32(o.get("qpos"))


def deep_state(M):
    """A picking reset that spawns the hand inside the pedestal: 68 contacts / 308 rows, beyond the heavy tier (huge tier)."""
    q = workload_reset(M, 256, 41)[200]
    q[18] = 0.0899
    return _f32(q)


def oracle_forward(model, q, ctrl):
    """Oracle at state q (zero velocity and warm start) after forward() with ctrl: its contacts (oracle_contacts)."""
    from oracle_binding import Oracle
    o = Oracle(model)
    o.set("qpos", q); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv)); o.set("ctrl", _f32(ctrl)); o.forward()
    return o


def compare(R, ncon, oc, M):
    """Worst differences of one env's record against the oracle's contacts: {"analytic" | "hull": [dist, pos, normal, force / largest normal
    force]}.  "analytic": condim-3 box / plane contacts; "hull": MPR contacts, "hull_deep" those more than 5 mm deep."""
    gmap, gtype = M["f_geom_orig"], M["geom_type"]
    assert ncon == oc["ncon"], (ncon, oc["ncon"])
    fmax = max(np.abs(oc["force"][:, 0]).max() if oc["ncon"] else 0.0, 1e-9)
    worst = {k: np.zeros(4) for k in BOUNDS}
    for k, j, s in match(R, ncon, oc, gmap, gtype):
        t1, t2 = gtype[gmap[R["geom"][k][0]]], gtype[gmap[R["geom"][k][1]]]
        kind = "analytic" if (R["dim"][k] == 3 and t1 in (0, 6) and t2 == 6) else ("hull" if oc["dist"][j] > -0.005 else "hull_deep")
        assert R["dim"][k] == oc["dim"][j]
        d = [abs(R["dist"][k] - oc["dist"][j]), np.abs(R["pos"][k] - oc["pos"][j]).max(), np.abs(R["frame"][k][0] - s * oc["normal"][j]).max(),
             np.abs(R["force"][k] - oc["force"][j]).max() / fmax]
        worst[kind] = np.maximum(worst[kind], d)
    return worst


# dist / pos / normal bounds of the seeded states (tests/test_contacts_emu.py): analytic contacts as
# tests/test_gpu_parity.py::test_stage_dump_and_counts_match holds them, MPR contacts tighter (what the finger pads of the grasp states
# reach).  The normal of an MPR contact more than 5 mm deep (an arm link inside the pedestal in one reset draw: 12 mm) comes from a portal that
# stopped at MPR's tolerance on a wide facet: 3.9e-6 measured, bound 3x.  Force, relative to the env's largest normal force: 3x the emulator's
# worst (3.5e-6).
BOUNDS = {"analytic": (1e-6, 1e-6, 1e-5), "hull": (3e-7, 3e-7, 2e-6), "hull_deep": (3e-7, 3e-7, 1.2e-5)}
FORCE_BOUND = 1e-5
# ... and of the 1 024 picking reset draws of tests/test_gpu_contacts.py, which reach further into the MPR regimes: a pad or link grazing a
# box leaves normals up to 2.1e-5 from the portal's stopping point, contacts more than 5 mm deep (hands inside the pedestal) 6.3e-5 and
# dist 2.6e-6; forces 3.9e-6 in envs whose deepest overlap is below 10.5 mm, 6.6e-5 in the 7 % beyond it (tens of ill-conditioned rows).
# Emulator and MI355X measured the same worst values; bounds 3x.
BOUNDS_SWEEP = {"analytic": (1e-6, 1e-6, 1e-5), "hull": (3e-7, 4e-7, 6.5e-5), "hull_deep": (8e-6, 2e-6, 2e-4)}
FORCE_SWEEP, FORCE_SWEEP_DEEP, DEEP = 1.2e-5, 2e-4, 0.0105


def check_sweep(res):
    """Asserts BOUNDS_SWEEP on a list of (deepest overlap, compare() result), one per env; returns the worst per kind and the force worsts."""
    worst = {k: np.zeros(4) for k in BOUNDS_SWEEP}
    fclean = fdeep = 0.0
    for deep, w in res:
        for k in worst:
            worst[k] = np.maximum(worst[k], w[k])
        f = max(v[3] for v in w.values())
        if deep > DEEP:
            fdeep = max(fdeep, f)
        else:
            fclean = max(fclean, f)
    for kind, (bd, bp, bn) in BOUNDS_SWEEP.items():
        d, p, n, _ = worst[kind]
        assert d < bd and p < bp and n < bn, (kind, worst[kind])
    assert fclean < FORCE_SWEEP and fdeep < FORCE_SWEEP_DEEP, (fclean, fdeep)
    return worst, fclean, fdeep


def deepest(oc):
    return -oc["dist"].min() if oc["ncon"] else 0.0


# ---------------------------------------------------------------- placed-object states: the narrowphase regimes the reset draws do not reach
REGIMES = ("pedestal top", "pedestal rim", "gap", "holder", "floor", "holder yawed", "arm")
PEDESTAL_TOP = 0.09 + 0.07 + 0.16
HOLDER_HALF = 0.15   # the holder's top face: 0.3 x 0.3 about (0, 0.6) at z = 0.17; the object box is 0.054 x 0.054 x 0.06


def _quat_axis_angle(ax, th):
    return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * ax / np.linalg.norm(ax)])


def placed_states(M, n, seed):
    """jaco2_curtain_torque with the arm at qpos0, the pedestal next to the holder at (0, 0.345) and the object box (free joint q[9:16])
    placed in seven regimes, cycled: (states [n, nq] fp32-rounded, regime index [n] into REGIMES).
    0 on the pedestal's top face; 1 over its rim (edge-edge contacts); 2 in the gap between pedestal and holder (a pedestal pair and a holder
    pair in one pass); 3 on the holder; 4 on the floor (plane-box, 1 to 4 corners down); 5 flat over a corner or a rim of the holder's top face,
    yawed, tilted ~0.01 rad and sunk 1.5 to 5.5 mm (reference corners and edge crossings: five and six contacts per pair); 6 against the arm (box-hull MPR contacts from grazing to centimetres
    deep).  The attitude of regimes 0-4 and 6 is a uniform random rotation, in every third state scaled to 0.15 of its angle."""
    from mujoco_jaco_amd.modelc import kin, rot
    rng = np.random.default_rng(seed)
    xpos = kin.fk(M, M["qpos0"])[0]
    hullbody = sorted({int(b) for b, t in zip(M["geom_bodyid"], M["geom_type"]) if t == 7 and xpos[b][2] > 0.3})
    q = np.tile(M["qpos0"], (n, 1))
    q[:, 16:19] = [0.0, 0.345, 0.0899]
    regime = np.arange(n) % len(REGIMES)
    u = rng.uniform
    for i in range(n):
        w = rng.normal(size=4); w /= np.linalg.norm(w)
        th = 2 * np.arccos(min(1.0, abs(w[0])))
        ax = w[1:] * (1 if w[0] >= 0 else -1)
        quat = _quat_axis_angle(ax, th * (0.15 if i % 3 == 0 else 1.0)) if np.linalg.norm(ax) > 0 else np.array([1.0, 0, 0, 0])
        r = regime[i]
        if r == 0: pos = [u(-0.06, 0.06), 0.345 + u(-0.06, 0.06), PEDESTAL_TOP + 0.03]
        elif r == 1: pos = [0.1 + u(-0.01, 0.01), 0.345 + u(-0.05, 0.05), PEDESTAL_TOP + 0.02]
        elif r == 2: pos = [u(-0.05, 0.05), 0.447 + u(-0.004, 0.004), 0.2]
        elif r == 3: pos = [u(-0.1, 0.1), 0.6 + u(-0.1, 0.1), 0.205]
        elif r == 4: pos = [0.4 + u(-0.1, 0.1), u(-0.1, 0.1), u(0.0, 0.04)]
        elif r == 5:
            cx, cy = HOLDER_HALF * rng.choice([-1, 1], 2) * (1, rng.integers(2))   # a corner of the holder's top face, or the middle of a rim
            pos = [cx + u(-0.03, 0.03), 0.6 + cy + u(-0.03, 0.03), 0.17 + 0.0245 + u(0.0, 0.004)]
            tilt = rng.normal(size=2) * 0.01
            quat = rot.quat_mul(_quat_axis_angle(np.array([0, 0, 1.0]), u(-np.pi, np.pi)), _quat_axis_angle(np.array([tilt[0], tilt[1], 1e-12]), np.linalg.norm(tilt)))
        else: pos = xpos[hullbody[rng.integers(len(hullbody))]] + rng.normal(size=3) * 0.03
        q[i, 9:12] = pos; q[i, 12:16] = quat
    return _f32(q), regime


def twins(q, free=9):
    """The ten neighbours of a state that decide whether it sits on a knife edge: the free body's position +-3e-7 m per axis, its
    quaternion +-3e-7 in four directions, renormalised."""
    out = []
    for k in range(3):
        for s in (-1, 1):
            t = q.copy(); t[free + k] += s * 3e-7; out.append(t)
    for k in range(4):
        t = q.copy(); t[free + 3 + k] += (1 if k % 2 == 0 else -1) * 3e-7
        t[free + 3:free + 7] /= np.linalg.norm(t[free + 3:free + 7]); out.append(t)
    return out


def _pairs(o):
    C = o.get("contact").reshape(-1, 11)
    return sorted((int(a), int(b)) for a, b in C[:, 7:9])


_tls = None


def oracle_states(model, M, qs, ctrl, knife=False, free=9):
    """The oracle's forward() at every state of qs ([n, nq]; ctrl [n, nu] or one row): a list of oracle_contacts() dicts, each with the geom
    poses "xpos" [ngeom, 3] / "xmat" [ngeom, 3, 3] added, and -- knife=True -- "knife": whether the multiset of contact geom pairs changes
    under any of the ten twins() of the state (a criterion on the reference alone).  One oracle per worker thread."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import os
    from oracle_binding import Oracle
    global _tls
    if _tls is None:
        _tls = threading.local()
    ctrl = np.broadcast_to(_f32(ctrl), (len(qs), np.shape(ctrl)[-1]))

    def one(i):
        d = _tls.__dict__.setdefault("o", {})
        if model not in d:
            d[model] = Oracle(model)
        o = d[model]

        def fwd(q):
            o.reset(); o.set("qpos", q); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv)); o.set("ctrl", ctrl[i]); o.forward()
        fwd(qs[i])
        oc = oracle_contacts(o, M)
        oc["xpos"], oc["xmat"] = o.get("geom_xpos").reshape(-1, 3), o.get("geom_xmat").reshape(-1, 3, 3)
        if knife:
            base = _pairs(o)
            oc["knife"] = False
            for t in twins(qs[i], free):
                fwd(t)
                if _pairs(o) != base:
                    oc["knife"] = True
                    break
        return oc
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(one, range(len(qs))))


def census(ocs, M, bodies=()):
    """From the oracle's contacts: {((type1, type2), contacts in the pair): number of pairs}, and how many states hold three or more contact
    pairs on one of `bodies` (MJCF body ids)."""
    from collections import Counter
    cnt, multi = Counter(), 0
    gtype, gbody = M["geom_type"], M["geom_bodyid"]
    for oc in ocs:
        per = Counter((int(a), int(b)) for a, b in oc["geom"])
        for (a, b), k in per.items():
            cnt[((int(gtype[a]), int(gtype[b])), k)] += 1
        multi += sum(1 for a, b in per if gbody[a] in bodies or gbody[b] in bodies) >= 3
    return cnt, multi


# ---- a portal-independent fp64 check of an MPR contact: support functions of the centred geoms, poses from the oracle
def support_h(M, g, xmat, d):
    """h_g(d) = max over the geom (about its centre) of x . d; d in world coordinates."""
    l = xmat[g].T @ d
    t, sz = M["geom_type"][g], M["geom_size"].reshape(-1, 3)[g]
    if t == 6:
        return float(np.abs(l) @ sz)
    if t == 5:
        return float(sz[0] * np.hypot(l[0], l[1]) + sz[1] * abs(l[2]))
    if t == 2:
        return float(sz[0] * np.linalg.norm(l))
    assert t == 7, t
    md = M["geom_dataid"][g]
    V = M["mesh_vert"].reshape(-1, 3)[M["mesh_vertadr"][md]:M["mesh_vertadr"][md] + M["mesh_vertnum"][md]]
    return float((V @ l).max())


def overlap(M, oc, g1, g2, n):
    """How far geoms g1 and g2 overlap along the unit direction n (from g1 towards g2): h1(n) + h2(-n) - n . (p2 - p1).  An MPR contact's
    dist is minus this at its own normal, whatever portal the refinement ended on."""
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n)
    return support_h(M, g1, oc["xmat"], n) + support_h(M, g2, oc["xmat"], -n) - n @ (oc["xpos"][g2] - oc["xpos"][g1])


def is_mpr(M, g1, g2):
    """The pair goes through the convex-convex path: neither a plane pair nor box-box."""
    t1, t2 = sorted((M["geom_type"][g1], M["geom_type"][g2]))
    return t1 != 0 and not (t1 == 6 and t2 == 6)


def oracle_consistency(M, oc):
    """|dist + overlap at the normal| of the oracle's own MPR contacts: the check of the criterion itself."""
    return [abs(oc["dist"][j] + overlap(M, oc, oc["geom"][j][0], oc["geom"][j][1], oc["normal"][j])) for j in range(oc["ncon"])
            if is_mpr(M, *oc["geom"][j])]


def contact_table(R, ncon, oc, M, gmap=None):
    """One env's record against the oracle's contacts, contact by contact: exact count, match() pairing, equal dim; a list of dicts
    {"kind" (compare()'s), "diff" [dist, pos, normal, force / largest normal force], "depth" (the oracle's), "geoms" (MJCF, record order),
    and for MPR contacts "cons" (a: |recorded dist + overlap at the recorded normal|) and "opt" (b: overlap at the recorded normal minus
    overlap at the oracle's)}."""
    gmap = M["f_geom_orig"] if gmap is None else gmap
    gtype = M["geom_type"]
    assert ncon == oc["ncon"], (ncon, oc["ncon"])
    fmax = max(np.abs(oc["force"][:, 0]).max() if oc["ncon"] else 0.0, 1e-9)
    rows = []
    for k, j, s in match(R, ncon, oc, gmap, gtype):
        g1, g2 = int(gmap[R["geom"][k][0]]), int(gmap[R["geom"][k][1]])
        t1, t2 = gtype[g1], gtype[g2]
        kind = "analytic" if (R["dim"][k] == 3 and t1 in (0, 6) and t2 == 6) else ("hull" if oc["dist"][j] > -0.005 else "hull_deep")
        assert (kind == "analytic") == (not is_mpr(M, g1, g2)), (g1, g2, t1, t2, R["dim"][k])
        assert R["dim"][k] == oc["dim"][j], (g1, g2, R["dim"][k], oc["dim"][j])
        row = {"kind": kind, "depth": -oc["dist"][j], "geoms": (g1, g2),
               "diff": np.array([abs(R["dist"][k] - oc["dist"][j]), np.abs(R["pos"][k] - oc["pos"][j]).max(),
                                 np.abs(R["frame"][k][0] - s * oc["normal"][j]).max(), np.abs(R["force"][k] - oc["force"][j]).max() / fmax])}
        if kind != "analytic":
            n = R["frame"][k][0].astype(np.float64)
            ov = overlap(M, oc, g1, g2, n)
            row["cons"] = abs(float(R["dist"][k]) + ov)
            row["opt"] = ov - overlap(M, oc, g1, g2, s * oc["normal"][j])
        rows.append(row)
    return rows


# ---- bounds of the contact-by-contact comparisons beyond the reset draws: the placed-object sweep (placed_states) and the golden poses of
# the two-arm and the sensor model.  All 3x the emulator's worst against the fp64 oracle (the device must meet the same numbers).
# The verdict they rest on: an MPR contact the kernel places beyond BOUNDS_SWEEP of the oracle's (normal up to 6.7e-4, pos up to 3.2e-5 off)
# is another portal of equal quality, not an error.  With the oracle's geom poses and fp64 support functions, every recorded MPR contact
# satisfies  (a) consistency: |dist + overlap(own normal)| <= 1.8e-7, and  (b) optimality: overlap(own normal) - overlap(oracle's normal)
# in [-5.1e-7, +9.5e-7], i.e. inside MPR's tolerance (opt_mpr_tolerance = 1e-6) -- and the contacts beyond BOUNDS_SWEEP no worse than the
# rest (a 7.7e-8, b 8.1e-7 against 1.8e-7, 9.5e-7).  The oracle's own contacts satisfy (a) to 2e-16.  fp32 stops the refinement on another
# triangle of a nearly coplanar facet fan, or at another rim point of a cylinder; both answers are within tolerance of the deepest overlap
# along the centre ray.
# Emulator, worst of: 2 800 placed states seed 7 (939 MPR contacts: a 1.7e-7, b 9.5e-7), the 13 two-arm poses (257: a 1.8e-7, b 5.9e-7 /
# 8.1e-7 for the one beyond), the 14 sensor-model poses (37 cylinder contacts: a 8.5e-8, b 3.3e-7).
HULL_CONSISTENCY = 5.4e-7   # (a), 3 x 1.8e-7
HULL_OPTIMALITY = 2.8e-6    # |b|, 3 x 9.5e-7
# dist / pos / normal of a contact beyond BOUNDS_SWEEP against the oracle's (pose-matched): emulator worst dist 7.3e-7 (two-arm), pos 3.2e-5
# (a cylinder rim; 3.1e-5 box on hull), normal 6.7e-4 (two-arm, 5.5 mm deep box on hull)
HULL_ALT = (2.2e-6, 9.6e-5, 2.0e-3)
# per set: the share of MPR contacts allowed beyond BOUNDS_SWEEP (3 x the emulator's: 1 of 939 placed -- none in the first 1 024 states --,
# 1 of 257 two-arm, 7 of 37 cylinder contacts) and the force bounds, relative to the env's largest normal force, split at DEEP as
# check_sweep splits them (emulator: placed 3.3e-6 / 3.8e-5; two-arm poses, all deeper than DEEP, 1.14e-4; sensor poses, none deeper, 8.4e-4:
# a load split over near-redundant contacts of one finger part, tests/test_kernel_emu.py)
PLACED = {"share": 3 / 939, "force": 1.0e-5, "force_deep": 1.13e-4}
DUAL_POSES = {"share": 3 / 257, "force": FORCE_SWEEP, "force_deep": 3.4e-4}
SENSOR_POSES = {"share": 21 / 37, "force": 2.5e-3, "force_deep": 2.5e-3}
# the device's record against the emulated kernel's at the first 210 placed states, [dist, pos, normal, force / largest normal force]
# (tests/test_gpu_contacts.py; counts, geom pairs and their order are identical): 3 x what the MI355X measured on its first run, 3.0e-8,
# 3.6e-7, 1.15e-6, 9.9e-7 -- the device compiler contracts multiply-adds that the host build of the emulator keeps apart
DEVICE_VS_EMU = (9.0e-8, 1.1e-6, 3.5e-6, 3.0e-6)
KNIFE_CAP = 0.01   # at most this share of a sweep's states may be left out as knife edges (oracle_states(knife=True)); 0 of 2 800 were


def tabulate(R, ocs, M, gmap=None, skip=()):
    """contact_table() of every env not in `skip`, each row with "env" and "deep" (the env's deepest overlap) added."""
    rows = []
    for i, oc in enumerate(ocs):
        if i in skip:
            continue
        for row in contact_table({k: v[i] for k, v in R.items()}, int(R["ncon"][i]), oc, M, gmap):
            row["env"], row["deep"] = i, deepest(oc)
            rows.append(row)
    return rows


def summarise(rows):
    """What check_contacts() bounds, measured: print it before asserting."""
    s = {"n": len(rows), "analytic": np.zeros(3), "inside": np.zeros(3), "beyond": np.zeros(3), "cons": 0.0, "opt": 0.0, "nmpr": 0, "nbeyond": 0,
         "cons_beyond": 0.0, "opt_beyond": 0.0, "force": 0.0, "force_deep": 0.0}
    for r in rows:
        k = "force_deep" if r["deep"] > DEEP else "force"
        s[k] = max(s[k], r["diff"][3])
        if r["kind"] == "analytic":
            s["analytic"] = np.maximum(s["analytic"], r["diff"][:3])
            continue
        s["nmpr"] += 1
        s["cons"], s["opt"] = max(s["cons"], r["cons"]), max(s["opt"], abs(r["opt"]))
        if (r["diff"][:3] < BOUNDS_SWEEP[r["kind"]]).all():
            s["inside"] = np.maximum(s["inside"], r["diff"][:3])
        else:
            s["nbeyond"] += 1
            s["beyond"] = np.maximum(s["beyond"], r["diff"][:3])
            s["cons_beyond"], s["opt_beyond"] = max(s["cons_beyond"], r["cons"]), max(s["opt_beyond"], abs(r["opt"]))
    return s


def check_contacts(s, B):
    """Analytic contacts inside BOUNDS_SWEEP; every MPR contact consistent and optimal; those beyond BOUNDS_SWEEP of the oracle's (alternative
    portals) inside HULL_ALT and no more than B["share"] of the MPR contacts; forces inside B's bounds."""
    assert (s["analytic"] < BOUNDS_SWEEP["analytic"]).all(), s["analytic"]
    assert s["cons"] < HULL_CONSISTENCY and s["opt"] < HULL_OPTIMALITY, (s["cons"], s["opt"])
    assert (s["beyond"] < HULL_ALT).all(), s["beyond"]
    assert s["nbeyond"] <= B["share"] * s["nmpr"], (s["nbeyond"], s["nmpr"])
    assert s["force"] < B["force"] and s["force_deep"] < B["force_deep"], (s["force"], s["force_deep"])


def print_summary(label, s):
    print("%s: %d contacts, %d MPR (%d beyond BOUNDS_SWEEP) | analytic dist/pos/normal %s | MPR inside %s beyond %s | consistency %.2e (beyond %.2e) "
          "optimality %.2e (beyond %.2e) | force rel clean %.2e deep %.2e" % (label, s["n"], s["nmpr"], s["nbeyond"], s["analytic"], s["inside"], s["beyond"],
                                                                               s["cons"], s["cons_beyond"], s["opt"], s["opt_beyond"], s["force"], s["force_deep"]))


def check_census(cnt, multi, scale=1):
    """The regimes the sweep has to contain (from the oracle's contacts): box-box pairs of 1, 2, 3, 4 contacts, pairs of five and more (edge
    crossings), object-floor pairs with 1, 2, 3 corners down, box-hull MPR contacts, states with three contact pairs on the free bodies."""
    bb = {k: sum(v for (t, c), v in cnt.items() if t == (6, 6) and c == k) for k in range(1, 9)}
    fl = {k: sum(v for (t, c), v in cnt.items() if t == (0, 6) and c == k) for k in range(1, 5)}
    hull = sum(v * c for (t, c), v in cnt.items() if t == (6, 7))
    print("census: box-box pairs by contact count %s | plane-box %s | box-hull contacts %d | states with >= 3 pairs on object / pedestal %d" % (bb, fl, hull, multi))
    assert all(bb[k] >= 5 * scale for k in (1, 2, 3, 4)), bb
    assert sum(bb[k] for k in range(5, 9)) >= 3 * scale and max(k for k in bb if bb[k]) <= 8, bb
    assert all(fl[k] >= scale for k in (1, 2, 3)), fl
    assert hull >= 30 * scale and multi >= 10 * scale, (hull, multi)
