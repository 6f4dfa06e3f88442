"""States for the touch-stage tests (tests/touch_binding.py) -- test inputs, not reference outputs: chosen on the fp64 oracle by what its
own touch computation exercises at them (touch_binding.census), never by what the kernel gives.
Writes tests/golden/touch_states.npz: per model `<key>_qpos` (fp32-representable rows) and `<key>_ctrl`.  Needs oracle/ built.

default (jaco2_curtain_torque): from workload.reset_states(qpos0, 1024, seed=41, f32_draws=True) with the pedestal at 0.0899 --
  every env with a contact past the 64th on a sensor body with positive force, every env with a knife reading, the envs with the most
  non-zero readings, the first few of each capacity class (by the oracle's contact and row counts) that read something, the first few
  light envs whose touched sensor is pressed by the pedestal, four envs without any sensor-body contact and four whose sensor-body
  contacts all carry no force or miss every site -- plus contacts_binding.grasp_state at 20, 30, 40 and 60 closing substeps.
old (jaco2_curtain_torque_old): object at four offsets in the grasp frame, 40 oracle substeps with the grip closing.
sensor (jaco2_curtain_torque_sensor): the object pressed 1 to 16 mm into its holder's disc: its sphere site (radius 0.03 about the centre of
  the 6 cm box; the model's only sensor site of type 2) is met from outside (shallow: the contact point is beyond the radius, the ray
  points away) and from inside (6 mm and deeper, the object 3 mm off the disc's axis: flat on flat, MPR places the contact within 1 cm of
  the face's middle, 2.7 mm and more inside the radius).
dual (jaco2_dual_torque): one object-in-hand state per arm (the second arm's sensor bodies have ids above 64), 25 and 40 closing substeps,
  and three states in which only pads of the second arm's little finger are touched (word 2 of the body mask alone decides the early-out)."""
import os, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import contacts_binding as cb
import touch_binding as tb
from oracle_binding import Oracle
from mujoco_jaco_amd import workload
from mujoco_jaco_amd.modelc import rot


def names_of(model):
    d = {}
    for line in open(os.path.join(ROOT, "mujoco_jaco_amd", "assets", model + ".names.txt")):
        k, v = line.strip().split(": ", 1); d[k] = v.split()
    return d


def report(label, M, model, q, ctrl):
    S = tb.oracle_states(model, M, q, ctrl)
    refs = tb.oracle_reference(M, S)
    print("%s: %d states | census %s | non-zero readings %d, knife %d | contacts %s" % (
        label, len(q), dict(tb.census(refs)), sum(int((r["sens"] > 0).sum()) for r in refs), sum(int(r["knife"].sum()) for r in refs), [s["ncon"] for s in S]))
    return S, refs


out = {}

# ---------------------------------------------------------------- default model
model = "jaco2_curtain_torque"
M, N = tb.model(model), names_of(model)
q = workload.reset_states(M["qpos0"], 1024, seed=41, f32_draws=True); q[:, 18] = 0.0899; q = cb._f32(q)
S = tb.oracle_states(model, M, q, np.zeros(9))
refs = tb.oracle_reference(M, S)
print("1 024 draws:", dict(tb.census(refs)), "| envs with more than 64 contacts", sum(s["ncon"] > 64 for s in S), "| with a late sensor-body contact",
      [i for i, s in enumerate(S) if s["late"]], "| knife readings", sum(int(r["knife"].sum()) for r in refs))
ped = N["body"].index("object_dest")
nz = np.array([(r["sens"] > 0).sum() for r in refs])
rows = np.array([s["nefc"] for s in S]); ncon = np.array([s["ncon"] for s in S])
cls = np.where((ncon > 64) | (rows > 256), 3, np.where((ncon > 32) | (rows > 128), 2, np.where(rows > 64, 1, 0)))   # (a guess at the tier: the tests read the real one)
pedpress = [i for i, (s, r) in enumerate(zip(S, refs)) if cls[i] == 0 and any(hit and fn > tb.MINVAL and ped in s["body"][c] for _, c, _, _, _, hit, _, fn in r["inc"])]
# (a sensor body is on the arm, so its contact with the pedestal reaches two dof blocks: stage_contact_rows moves the pedestal's rows to the
# side buffer only when no contact does -- these envs end on the medium tier, never on the light tier with side rows)
side = [i for i, (s, r) in enumerate(zip(S, refs)) if cls[i] == 1 and ncon[i] <= 32 and any(fn > tb.MINVAL and ped in s["body"][c] for _, c, _, _, _, _, _, fn in r["inc"])]
print("light-class envs whose touched sensor the pedestal presses: %d; envs with 65 .. 128 rows and a sensor-body contact against the pedestal: %d" % (len(pedpress), len(side)))
pick = [i for i, s in enumerate(S) if s["late"]] + [i for i, r in enumerate(refs) if r["knife"].any()] + [int(i) for i in np.argsort(-nz, kind="stable")[:22]]
for c in range(4):
    pick += [i for i in range(len(q)) if cls[i] == c and nz[i] > 0][:3]
pick += pedpress[:3] + side[:2]
pick += [i for i, r in enumerate(refs) if not r["inc"]][:4]
pick += [i for i, r in enumerate(refs) if r["inc"] and not nz[i]][:4]
pick = sorted(set(pick))
grasp = np.array([cb.grasp_state(M, N, n) for n in (20, 30, 40, 60)])
out["default_qpos"] = np.concatenate([q[pick], grasp])
out["default_ctrl"] = np.concatenate([np.zeros((len(pick), 9)), np.tile(cb.GRASP_CTRL, (4, 1))])
out["default_draw"] = np.array(pick + [-1] * 4)
report("default", M, model, out["default_qpos"], out["default_ctrl"])


# ---------------------------------------------------------------- object in the grasp frame, grip closing
def in_hand(model, arm, fingers, obj, ee_obj, ctrl, substeps, arm_pose=(1.3, 3.85, 1.05, 2.05, 1.5, -1.15), offset=(-0.04, 0, 0)):
    o = Oracle(model)
    N = names_of(model)
    q = o.get("qpos").copy()
    q[arm:arm + 6] = arm_pose
    for j, v in fingers:
        q[j] = v
    o.set("qpos", q); o.forward()
    b = N["body"].index(ee_obj)
    xp = o.get("xpos").reshape(-1, 3)[b]; xq = o.get("xquat").reshape(-1, 4)[b]
    q[obj:obj + 3] = xp + rot.quat_to_mat(xq) @ np.array(offset); q[obj + 3:obj + 7] = xq
    res = []
    for n in substeps:
        o.reset(); o.set("qpos", q); o.set("qvel", np.zeros(o.nv))
        o.step(ctrl, n=n)
        res.append(cb._f32(o.get("qpos")))
    return np.array(res)


model = "jaco2_curtain_torque_old"
ctrl = np.array([0, 0, 0, 0, 0, 0, 1.0, 1.0, 1.0])
# (offsets in the grasp frame at which the closing fingers of this hand meet its 4 cm object: the four of a 2 cm grid that press most pads)
out["old_qpos"] = np.concatenate([in_hand(model, 0, [(6, 0.6), (8, 0.6), (10, 0.6)], 12, "EE_obj", ctrl, (40,), offset=d)
                                  for d in ((-0.04, 0.04, -0.06), (-0.02, 0.06, -0.04), (-0.04, -0.06, -0.04), (-0.06, 0.06, -0.04))])
out["old_ctrl"] = np.tile(ctrl, (len(out["old_qpos"]), 1))
report("old", tb.model(model), model, out["old_qpos"], out["old_ctrl"])

model = "jaco2_dual_torque"
c1 = np.zeros(18); c1[6:9] = 1.0
c2 = np.zeros(18); c2[15:18] = 1.0
a = in_hand(model, 0, [(6, 0.6), (7, 0.6), (8, 0.6)], 18, "EE_obj_1", c1, (25, 40))
b = in_hand(model, 9, [(15, 0.6), (16, 0.6), (17, 0.6)], 25, "EE_obj_2", c2, (25, 40))
# ... and three states in which the only touched sensor bodies are pads of the second arm's little finger: ids 74 .. 80, whose bits in word 2
# of the body mask have no twin in word 1 (bodies 42 .. 48 carry no site) -- the stage's early-out is decided by word 2 alone there.
# The second object placed at random 2.5 to 5 cm from such a pad, kept when the oracle reads something and nothing else is touched.
M, o = tb.model(model), Oracle(model)
sbs = set(int(x) for x in tb.site_bodies(M))
word2 = tb.word2_only(M)
q0 = o.get("qpos").copy(); q0[9:15] = (1.3, 3.85, 1.05, 2.05, 1.5, -1.15); q0[15:18] = 0.6
o.set("qpos", q0); o.forward()
xp = o.get("xpos").reshape(-1, 3).copy()
rng = np.random.default_rng(5)
w2 = []
for it in range(4000):
    q = q0.copy()
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    q[25:28] = xp[[75, 79][it % 2]] + d * rng.uniform(0.025, 0.05)
    w = rng.normal(size=4); q[28:32] = w / np.linalg.norm(w)
    q = cb._f32(q)
    o.reset(); o.set("qpos", q); o.set("qvel", np.zeros(30)); o.forward()
    if o.ncon == 0:
        continue
    C = o.get("contact").reshape(-1, 11)
    on = [int(x) for x in M["geom_bodyid"][C[:, 7:9].astype(int)].reshape(-1) if int(x) in sbs]
    if on and all(x in word2 for x in on) and (o.get("sensordata") > 0).any() and C[:, 0].min() > -0.006:
        w2.append(q)
        if len(w2) >= 3:
            break
out["dual_qpos"] = np.concatenate([a, b, np.array(w2)])
out["dual_ctrl"] = np.array([c1, c1, c2, c2] + [np.zeros(18)] * len(w2))
report("dual", tb.model(model), model, out["dual_qpos"], out["dual_ctrl"])

# ---------------------------------------------------------------- the sensor model's sphere site: on the object's body, radius 0.03
model = "jaco2_curtain_torque_sensor"
M = tb.model(model)
P = np.load(os.path.join(tb.GOLDEN, "sensor_post_poses.npz"))
base = P["qpos"][0].copy()
qs = []
for dz, tilt, dx in ((0.001, 0.0, 0.0), (0.002, 0.05, 0.0), (0.006, 0.0, 0.003), (0.008, 0.0, 0.003), (0.016, 0.0, 0.003)):
    t = base.copy(); t[14] -= dz; t[12] += dx
    t[15:19] = [np.cos(tilt / 2), np.sin(tilt / 2), 0, 0]
    qs.append(t)
out["sensor_qpos"] = cb._f32(np.array(qs))
out["sensor_ctrl"] = np.zeros((len(qs), 9))
report("sensor", M, model, out["sensor_qpos"], out["sensor_ctrl"])

np.savez_compressed(os.path.join(tb.GOLDEN, "touch_states.npz"), **out)
print("wrote", {k: v.shape for k, v in out.items()})
