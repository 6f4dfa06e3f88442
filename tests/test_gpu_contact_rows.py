"""GPU tier: the row builder's free-column Jacobian pass (collision.h stage_contact_rows, JACO_ROWS_FREE: lane = (contact slot, dof of the
contact's free body) when every contact of the env moves one free body and nothing else, the other columns written as +0) on the device.

1. Env level, the pattern and the bounds of tests/test_gpu_newton_regime.py: 256 envs x 4 env steps x frame_skip 2 of the picking reset
   distribution against the wavefront emulator (same headers, compiled for the host).  Most of these substeps take the free-column pass
   (object on its holder, pedestal on the floor); one env in eight gets small actions (side rows, bigger tiers) and seed 41 holds a
   hand-in-pedestal reset (full-width passes, and the huge tier's second chunk over the free columns).
2. Ctrl level: 64 envs x 20 substeps against the fp64 oracle at the bounds of smoke() (__graft_entry__.py), error flags 0.
3. If the all-columns build (tools/build_variant.sh rowsall -DJACO_ROWS_FREE=0) lies next to the product library: the 256-env case on
   both libraries, each in a fresh child process with its own time limit, must agree bit for bit on qpos, qvel, obs, reward and done.
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
    """The 256-env case on the library JACO_ENV_LIB names (default: the product library): per step obs, reward, done, qpos, qvel; the flags."""
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
                    "qpos%d" % (s + 1): st[0].cpu().numpy(), "qvel%d" % (s + 1): st[1].cpu().numpy()})
    out["flags"] = env.sim.flags().cpu().numpy()
    env.close()
    return out


def test_env_steps_match_the_emulator_256_envs_4_steps(model_arrays):
    from emu_binding import EmuJacoEnv
    g = _gpu_rollout(model_arrays["qpos0"])
    q, nz0, steps = _inputs(model_arrays["qpos0"])
    e = EmuJacoEnv(nenv=B, frame_skip=FS)
    e.qpos[:] = q; e.task[:, 4:7] = q[:, 9:12]; e.task[:, 7:9] = q[:, 16:18]; e.task[:, 9] = 0.3468
    for i in (14, 15):
        e.L.emu_get_counter(i, 1)
    assert np.abs(g["obs0"] - e.forward(nz0)).max() < 2e-6
    errs, rerrs, qerrs = [], [], []
    for s, (a, nz) in enumerate(steps):
        eo, er, ed = e.env_step(a, nz)
        obs, rew, done, gq = (g["%s%d" % (k, s + 1)] for k in ("obs", "rew", "done", "qpos"))
        assert np.array_equal(done.astype(bool), ed.astype(bool))             # termination flag: exact
        assert np.array_equal(obs[:, 0], eo[:, 0])                            # touch class: exact
        errs.append(np.abs(obs - eo).max(1)); rerrs.append(np.abs(rew - er)); qerrs.append(np.abs(gq - e.qpos).max(1))
    errs, rerrs, qerrs = np.array(errs), np.array(rerrs), np.array(qerrs)
    compact, full = e.L.emu_get_counter(14, 1), e.L.emu_get_counter(15, 1)
    print("GPU vs emulator, %d envs x %d steps x %d substeps: obs err median %.2e max %.2e; reward err max %.2e; qpos err median %.2e max %.2e; "
          "Jacobian passes over the free columns %d, over all columns %d; envs that used a bigger tier %d"
          % (B, NSTEP, FS, np.median(errs), errs.max(), rerrs.max(), np.median(qerrs), qerrs.max(), compact, full, int(((g["flags"] & 32) != 0).sum())))
    assert (g["flags"] & 15).max() == 0 and (e.flags & 15).max() == 0
    assert compact > B * NSTEP * FS // 2 and full > 0                         # most env-substeps took the free-column pass (one per substep); the other path ran, too
    assert np.median(errs) < 2e-7 and errs.max() < 1.7e-4 and rerrs.max() < 1e-6      # (the bounds of tests/test_gpu_newton_regime.py)
    assert np.median(qerrs) <= 4e-7 and qerrs.max() <= 3e-4


def test_ctrl_level_matches_the_fp64_oracle_64_envs_20_substeps(model_arrays):
    """smoke()'s run and smoke()'s bounds (__graft_entry__.py)."""
    from mujoco_jaco_amd import workload
    from mujoco_jaco_amd.physics import BatchedMujoco
    from oracle_binding import Oracle
    n, nsub = 64, 20
    q = workload.reset_states(model_arrays["qpos0"], n, seed=7, f32_draws=True)
    c = workload.random_ctrl(n, seed=8, scale=0.2).astype(np.float32).astype(np.float64)
    env = BatchedMujoco(n, device=0)
    dev = env.device
    env.set_state(torch.tensor(q, dtype=torch.float32, device=dev), None, None)
    env.send_forces(torch.tensor(c, dtype=torch.float32, device=dev), nsub=nsub)
    gq = env.get_state()[0].cpu().numpy().astype(np.float64)
    fl = env.flags().cpu().numpy()
    env.close()
    o = Oracle()
    qo, vo, wo = q.copy(), np.zeros((n, 21)), np.zeros((n, 21))
    o.step_batch(qo, vo, wo, np.ascontiguousarray(c), nsub=nsub, nthreads=4)
    err = np.abs(gq - qo).max(axis=1)
    deepest = np.zeros(n)   # (smoke(): envs whose start state overlaps deeper than the 1 cm of the picking reset get the loose bound)
    for k in range(n):
        o.set("qpos", q[k]); o.set("qvel", np.zeros(21)); o.forward()
        C = o.get("contact").reshape(-1, 11)
        deepest[k] = -C[:, 0].min() if len(C) else 0.0
    clean = deepest <= 0.0105
    print("ctrl level, %d envs x %d substeps, qpos error vs fp64 oracle: median %.2e, p90 %.2e, max over %d clean envs %.2e, max %.2e; flags 0x%x"
          % (n, nsub, np.median(err), np.percentile(err, 90), int(clean.sum()), err[clean].max(), err.max(), int(np.bitwise_or.reduce(fl))))
    assert (fl & 15).max() == 0
    assert np.median(err) < 3e-7 and np.percentile(err, 90) < 4e-7
    assert err[clean].max() < 6e-7 and err.max() < 2.5e-3


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from mujoco_jaco_amd.modelc import blob
import test_gpu_contact_rows as T
M = blob.load(%r)
np.savez(sys.argv[1], **T._gpu_rollout(M["qpos0"]))
"""


def test_all_columns_build_gives_the_same_bits(tmp_path):
    variant = "libjaco_env_rowsall.so"
    if not os.path.exists(os.path.join(ROOT, "mujoco_jaco_amd", variant)):
        pytest.skip("%s not built (tools/build_variant.sh rowsall -DJACO_ROWS_FREE=0)" % variant)
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
    res = {}
    for lib in ("libjaco_env.so", variant):
        out = str(tmp_path / (lib + ".npz"))
        subprocess.run([sys.executable, "-c", code, out], env={**os.environ, "JACO_ENV_LIB": lib}, check=True, timeout=120)   # (a failure ends the test)
        res[lib] = np.load(out)
    a, b = res["libjaco_env.so"], res[variant]
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 2 + 5 * NSTEP
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["flags"] & 15).max() == 0
