"""GPU tier: the light tier's packed LDS layout (physics_kernel.h JacoLDS: sub-word per-contact and model-table index arrays) on the
device against the wavefront emulator, which compiles the same headers for the host: 256 envs x 4 env steps of the picking reset
distribution, most of them with headline-sized actions, one in eight with small ones (the EE's axis sticks on the "hand" marker's sticks:
side rows, bigger tiers), a reset or two with the hand inside the pedestal among them (contact list full, env handed up).

frame_skip is 2: the emulator walks 256 x 4 x frame_skip substeps on one core at ~3 ms each, and what the packing can break -- an index
read back wrong from a sub-word array -- shows in the first substep that has contacts; the second covers the substep loop's carry-over
(warm start, pair list, contact list reuse).
Bounds: those of tests/test_gpu_env.py::test_env_step_parity_vs_oracle_env for observation, reward, done flag and touch class (there
after 3 x 50 substeps against the fp64 oracle; here after fewer substeps against the fp32 emulator, so nothing is loosened), and for the
state the qpos bounds of tests/test_gpu_env.py::test_env_level_closed_loop_parity_256_envs_10_steps.
Measured on MI355X: obs error median 6.0e-8, max 7.6e-5; reward error max 4.3e-8; qpos error median 1.2e-7, max 2.5e-4 (the env ejected from
inside the pedestal); 52 envs beyond 64 rows, 48 through a bigger tier; 2.4 s."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_env_steps_match_the_emulator_256_envs_4_steps(model_arrays):
    from emu_binding import EmuJacoEnv
    from mujoco_jaco_amd import workload
    from mujoco_jaco_amd.env import JacoBatchedEnv
    B, nstep, fs = 256, 4, 2
    q = workload.reset_states(model_arrays["qpos0"], B, seed=41, f32_draws=True).astype(np.float32)   # (seed 41: env 200 spawns the hand inside the pedestal)
    rng = np.random.default_rng(17)
    scale = np.where(np.arange(B) % 8 != 1, 1.0, 0.05)[:, None]
    env = JacoBatchedEnv(num_envs=B, task="picking", frame_skip=fs)
    dev = env.device
    env.sim.set_state(torch.tensor(q, device=dev), torch.zeros(B, 21, device=dev), torch.zeros(B, 21, device=dev))
    t = env.task_state(); t[:] = 0; t[:, 0] = 0.6; t[:, 16] = 0.6
    t[:, 4:7] = torch.tensor(q[:, 9:12]); t[:, 7:9] = torch.tensor(q[:, 16:18]); t[:, 9] = 0.3468
    env.set_task_state(t)
    e = EmuJacoEnv(nenv=B, frame_skip=fs)
    e.qpos[:] = q; e.task[:, 4:7] = q[:, 9:12]; e.task[:, 7:9] = q[:, 16:18]; e.task[:, 9] = 0.3468
    nz = rng.uniform(size=(B, 12)).astype(np.float32)
    env.set_noise(torch.tensor(nz))
    obs = env.make_observation().cpu().numpy()
    assert np.abs(obs - e.forward(nz)).max() < 2e-6
    errs, rerrs, qerrs, rows = [], [], [], []
    for s in range(nstep):
        a = (rng.uniform(-1, 1, (B, 7)) * scale).astype(np.float32); nz = rng.uniform(size=(B, 12)).astype(np.float32)
        env.set_noise(torch.tensor(nz))
        obs, rew, done, _ = env.step(torch.tensor(a))
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        eo, er, ed = e.env_step(a, nz)
        gq = env.sim.get_state()[0].cpu().numpy()
        assert np.array_equal(done.astype(bool), ed.astype(bool))             # termination flag: exact
        assert np.array_equal(obs[:, 0], eo[:, 0])                            # touch class: exact
        errs.append(np.abs(obs - eo).max(1)); rerrs.append(np.abs(rew - er)); qerrs.append(np.abs(gq - e.qpos).max(1))
        rows.append(e.stats[:, 1].copy())
    errs, rerrs, qerrs, rows = np.array(errs), np.array(rerrs), np.array(qerrs), np.array(rows)
    gflags = env.sim.flags().cpu().numpy()
    print("GPU vs emulator, %d envs x %d steps x %d substeps: obs err median %.2e max %.2e; reward err max %.2e; qpos err median %.2e max %.2e; "
          "rows up to %d, envs beyond 64 rows %d, envs that used a bigger tier %d" % (B, nstep, fs, np.median(errs), errs.max(), rerrs.max(), np.median(qerrs),
                                                                                      qerrs.max(), rows.max(), int((rows > 64).any(0).sum()), int(((gflags & 32) != 0).sum())))
    assert (gflags & 15).max() == 0 and (e.flags & 15).max() == 0
    assert (rows > 64).any() and ((gflags & 32) != 0).any()                   # side rows / bigger tiers were reached
    assert np.median(errs) < 2e-7 and errs.max() < 1.7e-4 and rerrs.max() < 1e-6
    assert np.median(qerrs) <= 4e-7 and qerrs.max() <= 3e-4
    env.close()
