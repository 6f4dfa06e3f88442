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
