"""Per-stage cycle profile of the physics kernel (diagnostic build libjaco_env_prof.so)."""
import ctypes, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("JACO_ENV_LIB", "libjaco_env_prof.so")
# the diagnostic twin is only built on request (python __graft_entry__.py variant prof): a stale one from an earlier round, with another argument-block
# or handle layout, would pass the loader's symbol check and produce garbage profiles or faults -- refuse anything older than the product library
_pk = os.path.join(ROOT, "mujoco_jaco_amd")
_prof, _main = os.path.join(_pk, os.environ["JACO_ENV_LIB"]), os.path.join(_pk, "libjaco_env.so")
if not os.path.exists(_prof) or os.path.getmtime(_prof) < os.path.getmtime(_main):
    sys.exit("gpu_stage_profile.py: %s is missing or older than libjaco_env.so: build it first (python __graft_entry__.py variant prof)" % _prof)
import numpy as np, torch
from mujoco_jaco_amd.physics import BatchedMujoco
from mujoco_jaco_amd.modelc import blob
from mujoco_jaco_amd import workload
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
nsub = int(sys.argv[2]) if len(sys.argv) > 2 else 50
M = blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
envlevel = "--env" in sys.argv
presteps = int(sys.argv[sys.argv.index("--presteps") + 1]) if "--presteps" in sys.argv else 3   # env steps before the profiled one
prof = np.zeros((B, 16), np.uint64)
if envlevel:
    from mujoco_jaco_amd.env import JacoBatchedEnv
    genv = JacoBatchedEnv(num_envs=B, seed=1000, task="picking", frame_skip=nsub, auto_reset="--policy" in sys.argv)
    env = genv.sim
    genv.reset()
    gen = torch.Generator(device=env.device); gen.manual_seed(2000)
    ascale = float(sys.argv[sys.argv.index("--action-scale") + 1]) if "--action-scale" in sys.argv else 1.0
    acts = [(torch.rand(B, 7, device=env.device, generator=gen) * 2 - 1) * ascale for _ in range(4)]
    pol = None
    if "--policy" in sys.argv:   # actions from the reference's shipped picking policy; episode ages staggered as in bench.py
        from mujoco_jaco_amd.policy import HPCPolicy
        pol = HPCPolicy.load(os.path.join(ROOT, "tests", "golden", "policy_picking.npz"), device=env.device)
        ts = genv.task_state()
        ts[:, 1] = torch.randint(0, genv.task_max_steps, (B,), device=env.device, generator=gen).float()
        genv.set_task_state(ts)
        obs = genv.make_observation()
        for i in range(presteps):
            obs, _, _, _ = genv.step(pol.predict(obs)[0])
        acts = [pol.predict(obs)[0]] * 4
    else:
        for i in range(presteps): genv.step(acts[i % 4])
    torch.cuda.synchronize()
    env._chk(env.L.jaco_stage_profile(env.h, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1))
    env.clear_flags()
    t = time.time(); genv.step(acts[presteps % 4]); torch.cuda.synchronize(); dt = time.time() - t
elif "--arm" in sys.argv:   # BASELINE config 2: arm-only model, contacts off (the contact-free kernel), fresh random torques per launch
    env = BatchedMujoco(B, robot_file="jaco2_reaching_torque")
    env.set_option("disable_contact", 1)
    Ma = blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", "jaco2_reaching_torque.jacomdl"))
    q = torch.tensor(workload.reset_states(Ma["qpos0"], B), dtype=torch.float32, device=env.device)
    env.set_state(q, None, None)
    cs = [torch.tensor(workload.random_ctrl(B, seed=k, scale=0.2)[:, :env.nu].copy(), dtype=torch.float32, device=env.device) for k in range(8)]
    for k in range(6): env.send_forces(cs[k], nsub=nsub)
    torch.cuda.synchronize()
    env._chk(env.L.jaco_stage_profile(env.h, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1))
    t = time.time(); env.send_forces(cs[6], nsub=nsub); torch.cuda.synchronize(); dt = time.time() - t
else:
    env = BatchedMujoco(B)
    q = torch.tensor(workload.reset_states(M["qpos0"], B), dtype=torch.float32, device=env.device)
    c = torch.tensor(workload.random_ctrl(B, scale=0.2), dtype=torch.float32, device=env.device)
    env.set_state(q, None, None)
    env.send_forces(c, nsub=100); torch.cuda.synchronize()   # settle initial interpenetration
    env._chk(env.L.jaco_stage_profile(env.h, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1))
    t = time.time(); env.send_forces(c, nsub=nsub); torch.cuda.synchronize(); dt = time.time() - t
env._chk(env.L.jaco_stage_profile(env.h, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1))
names = ["walk", "geoms+inertia", "accum+mass+act", "limit rows", "collision: narrowphase", "contact rows", "newton: rest (start, qacc_smooth, final)", "touch",
         "euler+integrate", "collision: spheres", "collision: OBB cull", "newton: prologue (M rows, qacc_smooth, start point)", "newton: MFMA H build", "newton: H fetch+LDL", "newton: line search", "OSC (env level only)"]
if "--narrow" in sys.argv:   # a -DJACO_NARROW_PROFILE build of the diagnostic twin (JACO_ENV_LIB names it): the narrowphase by what it ran
    names[11], names[12], names[13], names[14], names[1] = "narrow: candidate records", "narrow: box-box", "narrow: plane-*", "narrow: MPR hits", "narrow: MPR misses + cached-direction tests"
    names[6] = "newton: everything"; names[4] = "narrow: rest (bookkeeping, tail)"
if "--rows" in sys.argv:   # a -DJACO_ROWS_PROFILE build of the diagnostic twin (JACO_ENV_LIB names it): the contact-row stage by its parts
    names[11], names[12], names[13], names[14], names[1] = "rows: per-contact parameters (pair constants)", "rows: row offsets, side-row bookkeeping", "rows: per-contact row writes", "rows: row velocities", "rows: Jacobian passes"
    names[6] = "newton: everything"; names[5] = "rows: rest (entry, tail)"
per = prof[:, :16].astype(np.float64) / nsub
print("B", B, "nsub", nsub, "substeps/s %.3g" % (B * nsub / dt), "flags", int(env.flags().max()))
st = env.stats().cpu().numpy()
print("stats mean", st.mean(0), "max", st.max(0), "line-search iterations mean", (st[:, 3] >> 16).mean(), "cand", (st[:, 3] & 0xffff).mean())
tot = per.sum(1)
for i, n in enumerate(names):
    if n == '-': continue
    print("%-42s mean %9.0f cyc  (%4.1f%%)  p50 %9.0f  p99 %9.0f" % (n, per[:, i].mean(), 100 * per[:, i].mean() / tot.mean(), np.median(per[:, i]), np.percentile(per[:, i], 99)))
if "--slow" in sys.argv:   # what the slowest 2 % of envs spend their time on
    slow = tot >= np.percentile(tot, 98)
    print("slowest 2 %% of envs: total mean %.0f" % tot[slow].mean())
    for i, n in enumerate(names): print("   %-42s mean %9.0f" % (n, per[slow, i].mean()))
    fl = env.flags().cpu().numpy()
    print("   flags: singular %.3f heavy %.3f maxiter %.3f; ncon mean %.1f cand mean %.1f iters mean %.2f" % (((fl[slow] & 64) != 0).mean(), ((fl[slow] & 32) != 0).mean(), ((fl[slow] & 16) != 0).mean(), st[slow, 0].mean(), (st[slow, 3] & 0xffff).mean(), st[slow, 2].mean()))
if "--by-rows" in sys.argv:   # stage split by the env's row count at the end of the step (which tier it lives in)
    for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 100000)):
        sel = (st[:, 1] > lo) & (st[:, 1] <= hi)
        if sel.sum() == 0: continue
        print("rows in (%d, %d]: %d envs, total mean %.0f cycles/substep, newton iters mean %.2f, contacts mean %.1f" % (lo, hi, sel.sum(), tot[sel].mean(), st[sel, 2].mean(), st[sel, 0].mean()))
        for i, n in enumerate(names): print("   %-42s mean %9.0f" % (n, per[sel, i].mean()))
if "--heavy" in sys.argv:   # envs the heavy tier touched in the profiled step (flags are cleared before it)
    fl = env.flags().cpu().numpy()
    hv = (fl & 32) != 0
    print("heavy-tier envs: %d, total mean %.0f cycles/substep" % (hv.sum(), tot[hv].mean() if hv.any() else 0))
    if hv.any():
        for i, n in enumerate(names): print("   %-42s mean %9.0f" % (n, per[hv, i].mean()))
        print("   ncon mean %.1f max %d  nefc mean %.1f max %d  cand mean %.1f iters mean %.2f" % (st[hv, 0].mean(), st[hv, 0].max(), st[hv, 1].mean(), st[hv, 1].max(), (st[hv, 3] & 0xffff).mean(), st[hv, 2].mean()))
        print("   per-env totals:", np.sort(tot[hv]).astype(int))
print("total per substep: mean %.0f cycles, p50 %.0f, p99 %.0f, max %.0f" % (tot.mean(), np.median(tot), np.percentile(tot, 99), tot.max()))
