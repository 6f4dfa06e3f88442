"""Census of the Newton stage's regimes on the headline workload (profiles/newton_regime.txt).

Needs the counting twin of the diagnostic build:
    tools/build_variant.sh census -DJACO_PROFILE_STAGES -DJACO_REGIME_CENSUS
(physics_kernel.h JCENSUS: the profile row holds counts instead of cycle sums).  The workload is bench.py's headline, env for env --
picking task, frame_skip 50, U(-1, 1)^7 actions, episode ages staggered, auto-reset, `--preroll` env steps before the counted ones --
at 16 384 envs, as tools/gpu_stage_profile.py.  Prints, over `--steps` counted env steps: the share of substeps whose solve had rows,
of those the share without a row on the arm/finger dof block ((rowblocks & 1) == 0), of those the share that deliver the damped solve
(have_qdamped), and the mean row count of such solves.  Also prints has_damping of the model as the loader derives it.
"""
import argparse, ctypes, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--preroll", type=int, default=700)
ap.add_argument("--frame-skip", type=int, default=50)
ap.add_argument("--action-scale", type=float, default=1.0)
ap.add_argument("--lib", default="libjaco_env_census.so")
args = ap.parse_args()
os.environ["JACO_ENV_LIB"] = args.lib
_pk = os.path.join(ROOT, "mujoco_jaco_amd")
if not os.path.exists(os.path.join(_pk, args.lib)) or os.path.getmtime(os.path.join(_pk, args.lib)) < os.path.getmtime(os.path.join(_pk, "libjaco_env.so")):
    sys.exit("gpu_regime_census.py: %s is missing or older than libjaco_env.so: tools/build_variant.sh census -DJACO_PROFILE_STAGES -DJACO_REGIME_CENSUS" % args.lib)
import numpy as np, torch
from mujoco_jaco_amd.env import JacoBatchedEnv
from mujoco_jaco_amd.modelc import blob

M = blob.load(os.path.join(_pk, "assets", "jaco2_curtain_torque.jacomdl"))
damp = np.asarray(M["dof_damping"])
# model_blob.cpp: 0 no joint damping, 1 on dofs >= 6 only (the finger joints), 2 anywhere among the first six
has_damping = 0 if not (damp > 0).any() else (2 if (damp[:6] > 0).any() else 1)
print("model jaco2_curtain_torque: dof_damping > 0 on dofs %s -> has_damping == %d" % (np.nonzero(damp > 0)[0].tolist(), has_damping))

B, fs = args.batch, args.frame_skip
genv = JacoBatchedEnv(num_envs=B, seed=1000, task="picking", frame_skip=fs, auto_reset=True)
env = genv.sim
dev = env.device
genv.reset()
gen = torch.Generator(device=dev); gen.manual_seed(2000)
ts = genv.task_state()
ts[:, 1] = torch.randint(0, genv.task_max_steps, (B,), device=dev, generator=gen).float()
genv.set_task_state(ts)
abuf = torch.empty(B, genv.action_space.shape[0], device=dev)
prof = np.zeros((B, 16), np.uint64)
ptr = prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
for _ in range(args.preroll):
    genv.step(abuf.uniform_(-args.action_scale, args.action_scale, generator=gen))
torch.cuda.synchronize()
env._chk(env.L.jaco_stage_profile(env.h, ptr, 1))   # (allocates and zeroes the rows)
env.clear_flags()
for _ in range(args.steps):
    genv.step(abuf.uniform_(-args.action_scale, args.action_scale, generator=gen))
torch.cuda.synchronize()
env._chk(env.L.jaco_stage_profile(env.h, ptr, 0))
c = prof[:, :4].astype(np.float64)
nsubsteps = float(B) * args.steps * fs
solves, free, dual, rows = c[:, 0].sum(), c[:, 1].sum(), c[:, 2].sum(), c[:, 3].sum()
st = env.stats().cpu().numpy()
print("B %d, frame_skip %d, %d counted env steps after %d; flags 0x%x; stats mean (contacts, rows, iterations) %s"
      % (B, fs, args.steps, args.preroll, int(np.bitwise_or.reduce(env.flags().cpu().numpy())), np.round(st[:, :3].mean(0), 2)))
print("substeps (upper bound: frozen or resetting envs run fewer)     %12.0f" % nsubsteps)
print("solves with constraint rows (stage_newton past ne == 0)       %12.0f  = %.2f %% of the substeps" % (solves, 100 * solves / nsubsteps))
print("  of those, no row on the arm/finger block (rowblocks & 1 == 0) %10.0f  = %.2f %% of the solves" % (free, 100 * free / max(solves, 1)))
print("    of those, have_qdamped (J^T f has no reader)                %10.0f  = %.2f %%" % (dual, 100 * dual / max(free, 1)))
print("    mean rows of such a solve                                   %10.2f" % (rows / max(free, 1)))
per_env = c[:, 1] / np.maximum(c[:, 0], 1)
print("per env: share of its solves in the regime: p10 %.3f  p50 %.3f  p90 %.3f; envs never in it %d, always in it %d"
      % (np.percentile(per_env, 10), np.median(per_env), np.percentile(per_env, 90), int((c[:, 1] == 0).sum()), int((c[:, 1] == c[:, 0]).sum())))
