"""CPU tier: the sub-word per-contact / model-table arrays of JacoLDS (physics_kernel.h: 16-bit pair index and first row, 8-bit condim,
8-bit body / dof / coordinate indices; the pair's dof chain masks read from the pair record by the row builder) under the wavefront
emulator, which compiles the same headers.  Three scenarios that reach every packed field's range, each against the fp64 oracle in state,
contact list and constraint rows, at the bounds the existing emulator tests hold for the same scenarios
(tests/test_kernel_emu.py, tests/test_env_emu.py, tests/test_contacts_emu.py)."""
import numpy as np

import contacts_binding as cb
from emu_binding import EmuEnv, EmuJacoEnv
from mujoco_jaco_amd import workload
from oracle_binding import Oracle
from oracle_env import OracleEnv


def _record_against_oracle(M, q, ctrl):
    """One substep with the contact record on: contact list (dist, pos, normal per kind) and row forces at cb.BOUNDS / cb.FORCE_BOUND."""
    e = EmuEnv()
    e.qpos[:] = q[None]; e.qvel[:] = 0; e.qacc_ws[:] = 0
    rec, n = e.step_rec(ctrl, nsub=1, cap=128)
    R = cb.unpack(rec, n)
    oc = cb.oracle_contacts(cb.oracle_forward("jaco2_curtain_torque", q, ctrl), M)
    w = cb.compare({k: v[0] for k, v in R.items()}, int(n[0]), oc, M)
    for kind, (bd, bp, bn) in cb.BOUNDS.items():
        d, p, nn, _ = w[kind]
        assert d < bd and p < bp and nn < bn, (kind, w[kind])
    assert max(v[3] for v in w.values()) < cb.FORCE_BOUND, w
    return e, R


def test_in_hand_grasp_keeps_state_contacts_and_rows(model_arrays, names):
    """Fingers closing on the object in the hand: condim-6 hull contacts between two moving bodies (finger pads on the object: chain masks
    on both sides of the row), box contacts on the holder.  State and sensors substep by substep as
    test_kernel_emu.py::test_in_hand_grasp_with_hull_contacts, then the contact list and the row forces of the closed grasp."""
    from mujoco_jaco_amd.modelc import rot
    o = Oracle(); e = EmuEnv()
    q = model_arrays["qpos0"].copy()
    q[:6] = [1.3, 3.85, 1.05, 2.05, 1.5, -1.15]; q[6:9] = 0.6; q[16:18] = [.4, .3]
    o.set("qpos", q); o.forward()
    b = names["body"].index("EE_obj")
    xp = o.get("xpos").reshape(-1, 3)[b]; xq = o.get("xquat").reshape(-1, 4)[b]
    q[9:12] = xp + rot.quat_to_mat(xq) @ np.array([-0.04, 0, 0]); q[12:16] = xq
    o.set("qpos", q)
    errs, sens, same = [], [], 0
    for i in range(12):
        g = min(1.0, 0.6 + 0.004 * i)
        e.qpos[0], e.qvel[0], e.qacc_ws[0] = [o.get(n) for n in ("qpos", "qvel", "qacc_warmstart")]
        ctrl = np.array([0, 0, 0, 0, 0, 0, g, g, g])
        e.step(ctrl); o.step(ctrl)
        errs.append(np.abs(o.get("qpos") - e.qpos[0]).max())
        if (e.stats[0, 0], e.stats[0, 1]) == (o.ncon, o.nefc):
            same += 1
            sens.append(np.abs(o.get("sensordata") - e.sensordata[0]).max() / max(1.0, o.get("sensordata").max()))
    assert (e.flags[0] & 31) == 0
    assert np.median(errs) < 1e-6 and max(errs) < 2e-4      # (a grazing contact may flip for one step)
    assert same >= 10 and np.median(sens) < 1e-3
    M = model_arrays
    e, R = _record_against_oracle(M, cb.grasp_state(M, names, 40), cb.GRASP_CTRL)
    n = int(R["ncon"][0])
    world = names["body"].index("world")
    assert n >= 8 and (R["dim"][0, :n] == 6).any() and (R["dim"][0, :n] == 3).any()
    assert ((R["body"][0, :n] != world).all(axis=1) & (R["dim"][0, :n] == 6)).any()   # a condim-6 contact between two moving bodies


def test_marker_stick_pose_with_side_rows(names, model_arrays):
    """Small actions: the EE's axis sticks rest on the "hand" marker's sticks and the step needs 68-72 rows, so the pedestal's contacts go to
    the side buffer -- their first row is JSIDE_BASE or beyond.  As test_env_emu.py::test_side_rows_keep_a_68_row_env_in_the_light_tier;
    then the contact list and row forces of a grasp pose that splits the same way (forces of the side rows read from the side buffer)."""
    seen = 0
    for seed in (4, 6):
        fs = 10
        e = EmuJacoEnv(frame_skip=fs); oe = OracleEnv(names, frame_skip=fs)
        q = workload.reset_states(model_arrays["qpos0"], 1, seed=seed, f32_draws=True)[0]
        oe.obj_goal = q[9:12].copy(); oe.dest_goal = np.array([q[16], q[17], 0.3468]).astype(np.float32).astype(np.float64)
        oe.set_state(q)
        e.qpos[0] = q; e.task[0, 4:7] = oe.obj_goal; e.task[0, 7:10] = oe.dest_goal
        rng = np.random.default_rng(seed)
        nz = rng.uniform(size=(1, 12)).astype(np.float32)
        e.forward(nz); oe.observe(nz[0, 6:].astype(np.float64))
        for step in range(4):
            a = (rng.uniform(-1, 1, 7) * 0.05).astype(np.float32); nz = rng.uniform(size=(1, 12)).astype(np.float32)
            e.flags[:] = 0
            obs, rew, done = e.env_step(a, nz)
            oo, orew, odone, _ = oe.step(a.astype(np.float64), nz[0].astype(np.float64))
            assert (e.stats[0, 0], e.stats[0, 1]) == (oe.o.ncon, oe.o.nefc)
            assert np.abs(obs[0] - oo).max() < 2e-6 and np.abs(e.qpos[0] - oe.o.get("qpos")).max() < 2e-6 and abs(rew[0] - orew) < 1e-5
            if 64 < e.stats[0, 1] <= 80 and not (e.flags[0] & 32):
                seen += 1
    assert seen >= 2
    M = model_arrays
    e, R = _record_against_oracle(M, cb.grasp_state(M, names, 30), cb.GRASP_CTRL)
    assert e.stats[0, 1] > 64 and not e.flags[0] & 32   # split mode on the light tier


def test_deep_overlap_reset_fills_the_contact_list_and_moves_up(model_arrays):
    """A reset with the hand inside the pedestal: more contacts than the light tier's list holds (the list fills to MAXCON, the env goes to
    the bigger tiers, which compile the same packed arrays with their own capacities).  Counts and the free-running state as
    test_kernel_emu.py::test_huge_tier_keeps_every_row_of_a_hand_in_pedestal_reset, contact list and row forces as
    test_contacts_emu.py::test_deep_overlap_reset_on_the_huge_tier_matches_oracle."""
    q = workload.reset_states(model_arrays["qpos0"], 256, seed=41, f32_draws=True)[200]
    c = workload.random_ctrl(256, seed=42, scale=0.2)[200].astype(np.float32).astype(np.float64)
    o = Oracle(); e = EmuEnv()
    o.reset(); o.set("qpos", q); o.set("ctrl", c); e.qpos[0] = q
    seen, worst = 0, 0.0
    for t in range(6):
        e.step(c); o.step()
        assert (e.stats[0, 0], e.stats[0, 1]) == (o.ncon, o.nefc), t
        seen = max(seen, o.nefc)
        worst = max(worst, np.abs(e.qpos[0] - o.get("qpos")).max())
    assert worst < 3.4e-5, worst
    assert seen > 256 and (e.flags[0] & 32) and (e.flags[0] & 7) == 0
    M = model_arrays
    e, R = _record_against_oracle(M, cb.deep_state(M), np.zeros(9))
    assert int(R["ncon"][0]) > 64 and (e.flags[0] & 32) and (e.flags[0] & 7) == 0
