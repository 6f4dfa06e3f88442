"""GPU tier: the dense solver blocks' lean forms (solver_blocks.h: one lane predicate per pivot, the back-substitution
sum without a lane mask) on the device.

If the build with the earlier forms (solver_blocks_masks.h; tools/build_variant.sh solvermasks -DJACO_SOLVER_MASKS=1) lies next to the product library: 256 envs
x 4 env steps x frame_skip 2 of the picking reset distribution (the case of tests/test_gpu_newton_regime.py: one env in eight gets
small actions -- side rows, bigger tiers -- and seed 41 holds a hand-in-pedestal reset) on both libraries, each in a fresh child process
with its own time limit, must agree bit for bit on qpos, qvel, qacc, obs, reward and done after every env step.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NSTEP, FS = 256, 4, 2


def _inputs(qpos0):
    from mujoco_jaco_amd import workload
    q = workload.reset_states(qpos0, B, seed=41, f32_draws=True).astype(np.float32)   # (seed 41: env 200 spawns the hand inside the pedestal)
    rng = np.random.default_rng(17)
    scale = np.where(np.arange(B) % 8 != 1, 1.0, 0.05)[:, None]
    nz0 = rng.uniform(size=(B, 12)).astype(np.float32)
    steps = [((rng.uniform(-1, 1, (B, 7)) * scale).astype(np.float32), rng.uniform(size=(B, 12)).astype(np.float32)) for _ in range(NSTEP)]
    return q, nz0, steps


def _gpu_rollout(qpos0):
    """The 256-env case on the library JACO_ENV_LIB names (default: the product library): per step obs, reward, done, qpos, qvel, qacc; the flags."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    q, nz0, steps = _inputs(qpos0)
    env = JacoBatchedEnv(num_envs=B, task="picking", frame_skip=FS)
    dev = env.device
    env.sim.set_state(torch.tensor(q, device=dev), torch.zeros(B, 21, device=dev), torch.zeros(B, 21, device=dev))
    t = env.task_state(); t[:] = 0; t[:, 0] = 0.6; t[:, 16] = 0.6
    t[:, 4:7] = torch.tensor(q[:, 9:12]); t[:, 7:9] = torch.tensor(q[:, 16:18]); t[:, 9] = 0.3468
    env.set_task_state(t)
    env.set_noise(torch.tensor(nz0))
    out = {"obs0": env.make_observation().cpu().numpy()}
    for s, (a, nz) in enumerate(steps):
        env.set_noise(torch.tensor(nz))
        obs, rew, done, _ = env.step(torch.tensor(a))
        st = env.sim.get_state()
        out.update({"obs%d" % (s + 1): obs.cpu().numpy(), "rew%d" % (s + 1): rew.cpu().numpy(), "done%d" % (s + 1): done.cpu().numpy(),
                    "qpos%d" % (s + 1): st[0].cpu().numpy(), "qvel%d" % (s + 1): st[1].cpu().numpy(), "qacc%d" % (s + 1): st[2].cpu().numpy()})
    out["flags"] = env.sim.flags().cpu().numpy()
    env.close()
    return out


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from mujoco_jaco_amd.modelc import blob
import test_gpu_solver_blocks as T
M = blob.load(%r)
np.savez(sys.argv[1], **T._gpu_rollout(M["qpos0"]))
"""


def test_masked_forms_build_gives_the_same_bits(tmp_path):
    variant = "libjaco_env_solvermasks.so"
    if not os.path.exists(os.path.join(ROOT, "mujoco_jaco_amd", variant)):
        pytest.skip("%s not built (tools/build_variant.sh solvermasks -DJACO_SOLVER_MASKS=1)" % variant)
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
    res = {}
    for lib in ("libjaco_env.so", variant):
        out = str(tmp_path / (lib + ".npz"))
        subprocess.run([sys.executable, "-c", code, out], env={**os.environ, "JACO_ENV_LIB": lib}, check=True, timeout=120)   # (a failure ends the test)
        res[lib] = np.load(out)
    a, b = res["libjaco_env.so"], res[variant]
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 2 + 6 * NSTEP
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["flags"] & 15).max() == 0
    assert all(np.isfinite(a["qacc%d" % (s + 1)]).all() for s in range(NSTEP))
