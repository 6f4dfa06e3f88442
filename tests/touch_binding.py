"""Stage T (csrc/collision.h stage_touch / ray_hits_site) against an fp64 restatement fed the kernel's own contact record -- TEST
INFRASTRUCTURE ONLY.  Shared by the CPU tests (tests/test_touch_emu.py) and the GPU tests (tests/test_gpu_touch.py).

The record (jaco_set_contact_record) holds the positions, normals, original body ids and decoded forces of the very substep whose touch
values sensordata holds; force[0] is the sum of the pyramid rows, which is what the stage's c_fn is.  Recomputing the readings from it in
fp64 takes the solver's conditioning out of the comparison: what remains is the fp32 sum of a contact's rows and the fp32 sum of a
sensor's contacts.  Body poses of the substep's forward pass come from the oracle's forward() at the same fp32-rounded state (one
substep from set_state, zero velocity and warm start), so a hit-or-miss decision can differ from the kernel's only where a point or ray
passes within fp32 rounding of the grown site boundary: those readings are flagged `knife` on the reference alone and left out."""
import os
from collections import Counter

import numpy as np

import contacts_binding as cb
from mujoco_jaco_amd.modelc import blob, rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MINVAL = 1e-15       # JMINVAL (physics_kernel.h) / MINVAL (jaco_oracle.c)
SITE_EPS = 1e-5      # the slack both grow a site volume by
# fp32 positions near 1 m have an ulp of 6e-8 to 1.2e-7; a point taken into a site frame is a difference of two such positions through a
# rotation of three products, ~5e-7 at worst: four times that.  Derived, not measured.
KNIFE_D = 2e-6
KNIFE_SHARE = 0.02   # knife readings among all non-zero readings
BOX, CYLINDER, SPHERE = 6, 5, 2
LAYOUT = {"jaco2_curtain_torque": "", "jaco2_reaching_torque": "", "jaco2_curtain_torque_sensor": "_d12", "jaco2_curtain_torque_old": "_d12",
          "jaco2_dual_torque": "_d30"}


def model(name):
    return blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", name + ".jacomdl"))


def ray_hits_site(type, size, p, d, slack=SITE_EPS):
    """Does the ray p + t d, t >= 0, meet the site volume grown by `slack`?  (p, d in the site frame; box half sizes, cylinder radius /
    half height about z, sphere radius.)  A coordinate in which the ray does not move (|d_i| < MINVAL) only has to lie inside its slab."""
    sz = np.asarray(size, np.float64) + slack
    t0, t1 = 0.0, np.inf
    if type == BOX:
        for i in range(3):
            if abs(d[i]) < MINVAL:
                if abs(p[i]) > sz[i]:
                    return False
                continue
            a, b = sorted(((-sz[i] - p[i]) / d[i], (sz[i] - p[i]) / d[i]))
            t0, t1 = max(t0, a), min(t1, b)
        return t1 >= t0
    if type == CYLINDER:
        if abs(d[2]) < MINVAL:
            if abs(p[2]) > sz[1]:
                return False
        else:
            a, b = sorted(((-sz[1] - p[2]) / d[2], (sz[1] - p[2]) / d[2]))
            t0, t1 = max(t0, a), min(t1, b)
        A, B, C = d[0] * d[0] + d[1] * d[1], p[0] * d[0] + p[1] * d[1], p[0] * p[0] + p[1] * p[1] - sz[0] * sz[0]
        if A < MINVAL:
            if C > 0:
                return False
        else:
            disc = B * B - A * C
            if disc < 0:
                return False
            t0, t1 = max(t0, (-B - np.sqrt(disc)) / A), min(t1, (-B + np.sqrt(disc)) / A)
        return t1 >= t0
    assert type == SPHERE, type
    A, B, C = d @ d, p @ d, p @ p - sz[0] * sz[0]
    if A < MINVAL:
        return C <= 0
    disc = B * B - A * C
    return disc >= 0 and (-B + np.sqrt(disc)) / A >= 0


def inside(type, size, p, slack=SITE_EPS):
    sz = np.asarray(size, np.float64) + slack
    if type == BOX:
        return bool((np.abs(p) <= sz).all())
    if type == CYLINDER:
        return bool(abs(p[2]) <= sz[1] and p[0] * p[0] + p[1] * p[1] <= sz[0] * sz[0])
    return bool(p @ p <= sz[0] * sz[0])


def touch_reference(M, xpos, xmat, pos, normal, body, fn):
    """fp64 restatement of the stage from the blob's unfused tables.  xpos [nbody, 3] / xmat [nbody, 3, 3]: body poses of the forward pass;
    pos [n, 3], normal [n, 3], body [n, 2] (MJCF ids), fn [n]: its contacts.  A contact counts for a sensor when one of its bodies is the
    site's body and fn > MINVAL; the ray runs from the contact point along the normal, negated when the site's body is the second one;
    point and ray go into the site frame and are tested against the site volume grown by SITE_EPS; the reading is the sum of the fn that
    hit.  Returns {"sens" [ns], "count" [ns] (contributing contacts), "load" [ns] (= sens: the sum the error bound scales with),
    "knife" [ns] (an incidence changes its answer between slack SITE_EPS - KNIFE_D and SITE_EPS + KNIFE_D),
    "inc": one (sensor, contact, site type, second body?, inside?, hit?, hit with the ray flipped?, fn) per incidence, zero-force ones
    included (fn <= MINVAL: they count for nothing)}."""
    xpos, xmat = np.asarray(xpos, np.float64).reshape(-1, 3), np.asarray(xmat, np.float64).reshape(-1, 3, 3)
    pos, normal, fn = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(normal, np.float64).reshape(-1, 3), np.asarray(fn, np.float64).reshape(-1)
    body = np.asarray(body).reshape(-1, 2)
    sid = M["sensor_siteid"]
    ns = len(sid)
    out = {"sens": np.zeros(ns), "count": np.zeros(ns, int), "knife": np.zeros(ns, bool), "inc": []}
    for s in range(ns):
        site = int(sid[s])
        sb, type, size = int(M["site_bodyid"][site]), int(M["site_type"][site]), M["site_size"].reshape(-1, 3)[site]
        on = np.nonzero((body == sb).any(1))[0]
        if not len(on):
            continue
        R = xmat[sb] @ rot.quat_to_mat(M["site_quat"].reshape(-1, 4)[site])
        p0 = xpos[sb] + xmat[sb] @ M["site_pos"].reshape(-1, 3)[site]
        for c in on:
            second = bool(body[c, 1] == sb)
            p, d = R.T @ (pos[c] - p0), R.T @ (normal[c] * (-1.0 if second else 1.0))
            hit = ray_hits_site(type, size, p, d)
            out["inc"].append((s, int(c), type, second, inside(type, size, p), hit, ray_hits_site(type, size, p, -d), float(fn[c])))
            if not fn[c] > MINVAL:
                continue
            if ray_hits_site(type, size, p, d, SITE_EPS - KNIFE_D) != ray_hits_site(type, size, p, d, SITE_EPS + KNIFE_D):
                out["knife"][s] = True
            if hit:
                out["sens"][s] += fn[c]
                out["count"][s] += 1
    out["load"] = out["sens"]
    return out


CENSUS_KEYS = ("incidences", "cylinder", "box", "sphere", "outside hit", "outside miss", "outside second", "flip matters", "zero force")


def census(refs):
    """What the incidences of a set of touch_reference() results exercise (those with fn > MINVAL, but for "zero force")."""
    c = Counter({k: 0 for k in CENSUS_KEYS})
    for r in refs:
        for s, k, type, second, ins, hit, fhit, fn in r["inc"]:
            if not fn > MINVAL:
                c["zero force"] += 1
                continue
            c["incidences"] += 1
            c[{BOX: "box", CYLINDER: "cylinder", SPHERE: "sphere"}[type]] += 1
            if not ins:
                c["outside hit" if hit else "outside miss"] += 1
                c["outside second"] += second
            c["flip matters"] += hit != fhit
    return c


def body_poses(o):
    return o.get("xpos").reshape(-1, 3), np.array([rot.quat_to_mat(q) for q in o.get("xquat").reshape(-1, 4)])


_tls = None


def oracle_states(name, M, qs, ctrl):
    """The oracle's forward() at every fp32-rounded state (zero velocity and warm start): per state {"xpos", "xmat" (body poses, from
    xquat), "sens" (its sensordata), "ncon", "pos", "normal", "body" [n, 2] (MJCF ids, from geom_bodyid), "fn" (normal force: the sum of
    the contact's rows of efc_force), "late": contacts past the 64th on a sensor body with fn > 0}.  One oracle per worker thread."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from oracle_binding import Oracle
    global _tls
    if _tls is None:
        _tls = threading.local()
    ctrl = np.broadcast_to(cb._f32(ctrl), (len(qs), np.shape(ctrl)[-1]))
    sbody = set(int(b) for b in M["site_bodyid"][M["sensor_siteid"]])

    def one(i):
        d = _tls.__dict__.setdefault("o", {})
        if name not in d:
            d[name] = Oracle(name)
        o = d[name]
        o.reset(); o.set("qpos", qs[i]); o.set("qvel", np.zeros(o.nv)); o.set("qacc_warmstart", np.zeros(o.nv)); o.set("ctrl", ctrl[i]); o.forward()
        oc = cb.oracle_contacts(o, M)
        xpos, xmat = body_poses(o)
        body = M["geom_bodyid"][oc["geom"]].reshape(-1, 2)
        fn = oc["force"][:, 0]
        late = [k for k in range(64, oc["ncon"]) if fn[k] > MINVAL and (int(body[k, 0]) in sbody or int(body[k, 1]) in sbody)]
        return {"xpos": xpos, "xmat": xmat, "sens": o.get("sensordata"), "ncon": oc["ncon"], "nefc": o.nefc, "pos": oc["pos"], "normal": oc["normal"],
                "body": body, "fn": fn, "late": late}
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        return list(ex.map(one, range(len(qs))))


def oracle_reference(M, S):
    """touch_reference() on the oracle's own contacts and forces, one per oracle_states() entry."""
    return [touch_reference(M, s["xpos"], s["xmat"], s["pos"], s["normal"], s["body"], s["fn"]) for s in S]


def check_restatement(M, S, refs=None):
    """The restatement, fed the oracle's contacts and forces, is the oracle's sensordata: worst absolute difference (bound 1e-11)."""
    refs = oracle_reference(M, S) if refs is None else refs
    worst = max(np.abs(r["sens"] - s["sens"]).max() for r, s in zip(refs, S))
    assert worst <= 1e-11, worst
    return worst


def tier(flags, stats):
    """The tier an env's one-substep step ended on, from its flags (the capacity that sent it on from tier 0 / 1 / 2: three bits each
    from bit 8) and its row count: "light", "light+side" (light with more than 64 rows: the pedestal's in the side buffer), "medium",
    "heavy", "huge"."""
    t = sum(1 for k in range(3) if (int(flags) >> (8 + 3 * k)) & 7)
    assert (t > 0) == bool(int(flags) & 32), (flags, stats)
    if t == 0:
        return "light+side" if stats[1] > 64 else "light"
    return ("medium", "heavy", "huge")[t - 1]


def check_stage(M, S, R, sens, label):
    """The stage against its own record.  S: oracle_states() (body poses); R: contacts_binding.unpack() of the raw record (capacity at
    least the largest count); sens [n, ns]: the kernel's sensordata of the same substep.  For every reading that is not knife:
    |sens - ref| <= (10 + n_k) 2^-23 sum(fn of the n_k counted contacts) -- a counted contact's fn is an fp32 sum of at most 10 rows
    (condim 6), which the record repeats bit for bit, and the reading an fp32 sum of n_k of them -- and exactly 0 where n_k = 0.
    Returns {"ratio" (worst error / bound), "knife", "nonzero", "refs"}."""
    n = len(S)
    assert (R["ncon"] <= R["dist"].shape[1]).all(), ("record capacity below the largest count", R["ncon"].max())
    refs, ratio, knife, nonzero = [], 0.0, 0, 0
    for i in range(n):
        k = int(R["ncon"][i])
        r = touch_reference(M, S[i]["xpos"], S[i]["xmat"], R["pos"][i, :k], R["frame"][i, :k, 0], R["body"][i, :k], R["force"][i, :k, 0])
        refs.append(r)
        nonzero += int(((r["sens"] > 0) | (sens[i] > 0)).sum())
        knife += int(r["knife"].sum())
        for s in np.nonzero(~r["knife"])[0]:
            if r["count"][s] == 0:
                assert sens[i, s] == 0, (label, i, s, sens[i, s])
                continue
            bound = (10 + r["count"][s]) * 2.0 ** -23 * r["load"][s]
            err = abs(float(sens[i, s]) - r["sens"][s])
            ratio = max(ratio, err / bound)
            assert err <= bound, (label, "env", i, "sensor", s, "kernel", float(sens[i, s]), "recomputed", r["sens"][s], "contacts", int(r["count"][s]), err / bound)
    print("%s: stage against its record, %d envs, %d non-zero readings, %d knife; worst error / bound %.3f" % (label, n, nonzero, knife, ratio))
    assert knife <= KNIFE_SHARE * max(nonzero, 1), (label, knife, nonzero)
    return {"ratio": ratio, "knife": knife, "nonzero": nonzero, "refs": refs}


def pipeline_figure(S, sens, label):
    """Printed, not asserted: the kernel's sensordata against the oracle's (solver conditioning included), relative to the largest reading."""
    so = np.array([s["sens"] for s in S])
    fig = float(np.abs(sens - so).max() / max(so.max(), 1e-9))
    print("%s: |kernel sensordata - oracle sensordata| / largest reading %.2e" % (label, fig))
    return fig


# ---------------------------------------------------------------- the state sets (tests/golden/touch_states.npz, make_touch_states.py) and what each must exercise
SETS = {"default": "jaco2_curtain_torque", "old": "jaco2_curtain_torque_old", "sensor": "jaco2_curtain_torque_sensor", "dual": "jaco2_dual_torque"}
_cache = {}


def states(key):
    """(model name, M, qpos [n, nq] fp32-rounded, ctrl [n, nu], oracle_states(), oracle_reference()) of one set, computed once per process.
    "sensor" is the 14 poses of sensor_post_poses.npz then the sphere-site states; "dual" the 13 poses of dual_cross_poses.npz then the
    object-in-hand states (zero ctrl at the golden poses)."""
    if key not in _cache:
        name = SETS[key]
        M = model(name)
        T = np.load(os.path.join(GOLDEN, "touch_states.npz"))
        q, ctrl = T[key + "_qpos"], T[key + "_ctrl"]
        poses = {"sensor": "sensor_post_poses.npz", "dual": "dual_cross_poses.npz"}.get(key)
        if poses:
            p = np.load(os.path.join(GOLDEN, poses))["qpos"]
            q, ctrl = np.concatenate([p, q]), np.concatenate([np.zeros((len(p), ctrl.shape[1])), ctrl])
        q = cb._f32(q)
        assert len(q) < 64
        S = oracle_states(name, M, q, ctrl)
        _cache[key] = (name, M, q, ctrl, S, oracle_reference(M, S))
    return _cache[key]


def site_bodies(M):
    return M["site_bodyid"][M["sensor_siteid"]]


def word2_only(M):
    """Sensor bodies with an id of 64 and above whose bit in word 2 of the stage's body mask has no twin in word 1 (body id - 32 carries no
    sensor site): where only these are touched, the early-out is decided by word 2 alone."""
    sbs = set(int(b) for b in site_bodies(M))
    return sorted(b for b in sbs if b >= 64 and (b - 32) not in sbs)


def check_census(key, M, S, refs, R=None, tiers=None, knife=False):
    """What a set has to exercise, from touch_reference() results (the oracle's contacts, or the kernel's record): a later change of states
    cannot quietly lose a branch.  S gives the contact counts (R["ncon"] when a record is given); tiers (tier() per env) and knife
    (knife readings present: asserted on the oracle's contacts only) are checked when given."""
    c = census(refs)
    ncon = np.array([s["ncon"] for s in S]) if R is None else R["ncon"]
    touched = np.array([(r["sens"] > 0).any() for r in refs])
    print("%s census: %s | envs with more than 64 contacts %d | touched envs %d%s" % (key, dict(c), int((ncon > 64).sum()), int(touched.sum()),
                                                                                      "" if tiers is None else " on tiers %s" % dict(Counter(np.array(tiers)[touched]))))
    if key == "default":
        assert min(c[k] for k in ("cylinder", "box", "outside hit", "outside miss", "outside second", "flip matters")) >= 2, c
        assert (ncon > 64).sum() >= 2
        # a contact past the 64th on a sensor body with positive force, counted by a sensor
        late = sum(1 for r in refs if any(k >= 64 and fn > MINVAL and hit for _, k, _, _, _, hit, _, fn in r["inc"]))
        assert late >= 2, late
        # early-out: envs without a sensor-body contact, and envs whose sensor-body contacts all carry no force or miss (the ballot passes, the sums stay 0)
        assert sum(1 for r in refs if not r["inc"]) >= 3 and sum(1 for r in refs if r["inc"] and not (r["sens"] > 0).any()) >= 1
        if knife:
            assert sum(int(r["knife"].sum()) for r in refs) >= 2
        if tiers is not None:
            assert {"light", "light+side", "heavy", "huge"} <= set(np.array(tiers)[touched]), Counter(tiers)
    elif key == "old":
        assert min(c[k] for k in ("cylinder", "box", "outside hit", "outside miss")) >= 2, c
    elif key == "sensor":
        # the sphere site: a point inside it (hit) and a point outside it whose ray points away (miss; it would hit with the ray flipped)
        sph = [i for r in refs for i in r["inc"] if i[2] == SPHERE and i[7] > MINVAL]
        assert sum(1 for i in sph if i[4] and i[5]) >= 2 and sum(1 for i in sph if not i[4] and not i[5] and i[6]) >= 2, sph
        assert c["box"] >= 2 and sum(int((r["sens"] > 0).sum()) for r in refs[:14]) >= 4, c   # the four golden poses that press a pad
    elif key == "dual":
        assert min(c[k] for k in ("cylinder", "box", "outside hit", "outside miss", "outside second")) >= 2, c
        # sensors of the second arm: bodies above id 64, word 2 of the body mask
        sb = site_bodies(M)
        assert sum(int(((r["sens"] > 0) & (sb >= 64)).sum()) for r in refs) >= 2 and sum(int(((r["sens"] > 0) & (sb < 64) & (sb >= 32)).sum()) for r in refs) >= 2
        # ... and envs that read something while every sensor-body contact is on a body that word 2 alone marks
        w2 = word2_only(M)
        assert sum(1 for r in refs if (r["sens"] > 0).any() and all(int(sb[i[0]]) in w2 for i in r["inc"])) >= 2
    return c


def check_set(key, run, label):
    """One set through the kernel (run(model name, qpos, ctrl) -> (raw record [n, cap, 24] words, ncon, sensordata, flags, stats): one
    substep from set_state, zero velocity and warm start, flags cleared before): nothing overflowed, the stage against its own record
    (check_stage), the census of what the stage really saw, the pipeline figure.  Returns check_stage()'s result with "figure" added."""
    name, M, q, ctrl, S, orefs = states(key)
    rec, ncon, sens, flags, stats = run(name, q, ctrl)
    R = cb.unpack(rec, ncon)
    assert (flags & 7).max() == 0, flags
    assert ncon.max() <= rec.shape[1], (ncon.max(), rec.shape[1])
    res = check_stage(M, S, R, sens, "%s %s" % (label, key))
    tiers = [tier(flags[i], stats[i]) for i in range(len(q))] if key == "default" else None
    check_census(key, M, S, res["refs"], R=R, tiers=tiers)
    res["figure"] = pipeline_figure(S, sens, "%s %s" % (label, key))
    npose = {"sensor": 14, "dual": 13}.get(key)
    if npose:
        pipeline_figure(S[:npose], sens[:npose], "%s %s, golden poses alone" % (label, key))
    return res
