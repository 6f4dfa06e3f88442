"""CPU tier: the Newton stage's regime shortcuts (physics_kernel.h JACO_NEWTON_REGIME: J^T f only when somebody reads it, the products
M v and J v without the arm/finger columns when no constraint row touches that dof block) change no bit.

Two emulator builds of the same sources -- the default one and -DJACO_NEWTON_REGIME=0 (all columns, J^T f always: what the kernel did
before) -- run the same inputs, and everything the kernel hands back must be equal bit for bit: qpos, qvel, qacc_warmstart,
sensordata, flags, the contact record (contact list + contact forces, i.e. the row forces e_f decoded) and the debug dump of the last
substep (mass matrix, bias, qacc, qfrc_constraint, contact list, row forces, touch forces).  (The emulator keeps state in one fp32
word per coordinate: the compensated low words never leave the kernel here, they are zero on entry to every call in both builds.)

Each case asserts, from the emulator's event counters (8: constrained solves, 11: those without a row on the arm/finger block,
12: solves that formed J^T f, 13: damped solves of the Euler stage), that it really was in the regime it is about.
Case (a) is also held to the fp64 oracle at the bounds of tests/test_kernel_emu.py (ctrl level, states re-synchronised every substep:
test_contact_pipeline_matches_oracle_on_reset_distribution) and tests/test_env_emu.py (env level: test_env_step_matches_oracle_env).
"""
import os
import subprocess

import numpy as np
import pytest

import emu_binding
from emu_binding import EmuEnv, EmuJacoEnv
from mujoco_jaco_amd import workload
from mujoco_jaco_amd.modelc import blob

DBG_QFRC_CON = lambda nb, nv: 3 * nb + 9 * nb + nv * nv + 4 * 24   # physics_kernel.h JDBG_QFRC_CON
SOLVES, FREE_ONLY, JTF, DAMPED = 8, 11, 12, 13


def _variant(layout=""):
    """The all-columns build of a layout, driven through the emulator Makefile's own pattern rule (its flags given on the command line)."""
    name = "libjaco_emu%s_noregime.so" % layout
    flags = ("$(FLAGS%s) " % layout if layout else "") + "-DJACO_NEWTON_REGIME=0"
    subprocess.check_call(["make", "-s", "-C", emu_binding.EMU_DIR, name, "LIBS=" + name, "FLAGS%s_noregime=%s" % (layout, flags)])
    return layout + "_noregime"


def _counters(L):
    return {i: L.emu_get_counter(i, 1) for i in (SOLVES, FREE_ONLY, JTF, DAMPED)}


def _run(layout, model, q, v, ctrl, calls, nsub, dump_every, disable_contact=False, blob_bytes=None):
    """`calls` ctrl-level calls of `nsub` substeps; env 0 is dumped in every `dump_every`-th call (its last substep), the contact record is
    on throughout.  Returns everything the kernel handed back, call by call, and the counters call by call."""
    e = EmuEnv(model, nenv=len(q), layout=layout)
    if blob_bytes is not None:
        e.blob = blob_bytes
    e.qpos[:] = q
    e.qvel[:] = v
    out, ctr = [], []
    _counters(e.L)
    for k in range(calls):
        cap = 16
        rec = np.full((len(q) * cap, 24), np.nan, np.float32)
        ncon = np.full(len(q), -7, np.int32)
        dump = dump_every and k % dump_every == dump_every - 1
        e.dbg[:] = 0
        e._physics_step(ctrl, nsub, disable_contact, rec, ncon, cap, 0 if dump else -1)
        ctr.append(_counters(e.L))
        out.append(dict(qpos=e.qpos.copy(), qvel=e.qvel.copy(), qacc_ws=e.qacc_ws.copy(), sens=e.sensordata.copy(), flags=e.flags.copy(),
                        stats=e.stats.copy(), rec=rec.copy(), ncon=ncon.copy(), dbg=e.dbg.copy(), dumped=bool(dump)))
    return out, ctr, e


def _same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        for name in ("qpos", "qvel", "qacc_ws", "sens", "flags", "stats", "rec", "ncon", "dbg"):
            assert x[name].tobytes() == y[name].tobytes(), "%s: %s differs in call %d" % (what, name, k)


def _total(ctr, i):
    return sum(c[i] for c in ctr)


def _picking(M, n, seed=11):
    return workload.reset_states(M["qpos0"], n, seed=seed, f32_draws=True).astype(np.float32), np.zeros((n, 21), np.float32)


def _both(model, q, v, ctrl, calls, nsub, dump_every, **kw):
    from mujoco_jaco_amd import _lib as product_lib
    layout = product_lib.variant_for(open(os.path.join(emu_binding.ASSETS, model + ".jacomdl"), "rb").read())   # (the loader's own choice)
    new = _run(layout, model, q, v, ctrl, calls, nsub, dump_every, **kw)
    old = _run(_variant(layout), model, q, v, ctrl, calls, nsub, dump_every, **kw)
    _same_bits(new[0], old[0], model)
    # what the counters count does not depend on the build, except 12: the all-columns build forms J^T f in every constrained solve
    for cn, co in zip(new[1], old[1]):
        assert (cn[SOLVES], cn[FREE_ONLY], cn[DAMPED]) == (co[SOLVES], co[FREE_ONLY], co[DAMPED]) and co[JTF] == co[SOLVES]
    return new


def test_a_object_at_rest_arm_moving_regime_on_throughout(model_arrays):
    q, v = _picking(model_arrays, 3)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    out, ctr, e = _both("jaco2_curtain_torque", q, v, ctrl, calls=10, nsub=2, dump_every=2)
    n = _total(ctr, SOLVES)
    assert n == 3 * 20 and _total(ctr, FREE_ONLY) == n                 # every substep: rows, none of them on the arm/finger block
    assert _total(ctr, DAMPED) == 0                                    # the damped solve came out of the stage: J^T f has no reader ...
    assert _total(ctr, JTF) == 5                                       # ... except the five dumps of env 0
    assert (out[-1]["stats"][:, 0] == 8).all() and (out[-1]["stats"][:, 1] == 32).all()   # the headline's mean env: 8 contacts, 32 rows
    assert (out[-1]["flags"] == 0).all()
    # the dump still carries qfrc_constraint: zero on the arm/finger dofs, the contact forces on the free bodies
    for o in out:
        qf = o["dbg"][DBG_QFRC_CON(11, 21):DBG_QFRC_CON(11, 21) + 21]
        assert (np.abs(qf[9:]).max() > 1.0 and not qf[:9].any()) if o["dumped"] else not o["dbg"].any()


def test_a_matches_the_fp64_oracle_at_ctrl_level(model_arrays):
    """tests/test_kernel_emu.py::test_contact_pipeline_matches_oracle_on_reset_distribution, on case (a)'s envs: its bounds, restated."""
    from oracle_binding import Oracle
    o = Oracle(); e = EmuEnv()
    q = workload.reset_states(model_arrays["qpos0"], 3, seed=11, f32_draws=True)
    c = workload.random_ctrl(3, seed=12, scale=0.2)
    worst = 0.0
    _counters(e.L)
    for k in range(3):
        o.reset(); o.set("qpos", q[k])
        for i in range(12):
            e.qpos[0], e.qvel[0], e.qacc_ws[0] = [o.get(n) for n in ("qpos", "qvel", "qacc_warmstart")]
            e.step(c[k]); o.step(c[k])
            assert (e.stats[0, 0], e.stats[0, 1]) == (o.ncon, o.nefc), (k, i)
            worst = max(worst, np.abs(o.get("qpos") - e.qpos[0]).max())
    ctr = _counters(e.L)
    assert ctr[SOLVES] == 36 and ctr[FREE_ONLY] == 36 and ctr[JTF] == 0
    assert worst < 2e-6 and e.flags[0] == 0


def test_a_matches_the_fp64_oracle_at_env_level(names, model_arrays):
    """tests/test_env_emu.py::test_env_step_matches_oracle_env (its set-up and bounds, restated) with the regime counted."""
    from oracle_env import OracleEnv
    e = EmuJacoEnv(frame_skip=10); oe = OracleEnv(names, frame_skip=10)
    q = workload.reset_states(model_arrays["qpos0"], 1, seed=3)[0]
    oe.obj_goal = q[9:12].copy(); oe.dest_goal = np.array([q[16], q[17], 0.3468])
    oe.set_state(q.astype(np.float32).astype(np.float64))
    e.qpos[0] = q; e.task[0, 4:7] = oe.obj_goal; e.task[0, 7:10] = oe.dest_goal
    rng = np.random.default_rng(3)
    nz = rng.uniform(size=(1, 12)).astype(np.float32)
    _counters(e.L)
    obs0 = e.forward(nz)
    assert np.abs(obs0[0] - oe.observe(nz[0, 6:].astype(np.float64))[0]).max() < 2e-6
    for step in range(3):
        a = rng.uniform(-1, 1, 7).astype(np.float32); nz = rng.uniform(size=(1, 12)).astype(np.float32)
        obs, rew, done = e.env_step(a, nz)
        oo, orew, odone, _ = oe.step(a.astype(np.float64), nz[0].astype(np.float64))
        assert obs[0, 0] == oo[0] and bool(done[0]) == odone
        assert np.abs(obs[0] - oo).max() < 5e-5 and abs(rew[0] - orew) < 1e-4
    ctr = _counters(e.L)
    assert ctr[SOLVES] == 31 and ctr[FREE_ONLY] == 31 and ctr[JTF] == 0 and ctr[DAMPED] == 0   # forward pass + 3 x 10 substeps, nobody read J^T f


def test_b_arm_joint_at_its_limit_regime_off(model_arrays):
    q, v = _picking(model_arrays, 3)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    q[:, 2] = 0.335; v[:, 2] = -1.0; ctrl[:, 2] = -30.0                # joint 2 (range 0.332 .. 5.952) driven into its lower limit
    out, ctr, e = _both("jaco2_curtain_torque", q, v, ctrl, calls=10, nsub=2, dump_every=2)
    n = _total(ctr, SOLVES)
    assert n == 3 * 20 and _total(ctr, FREE_ONLY) == 0                  # rows on the arm block in every substep
    assert _total(ctr, JTF) == n and _total(ctr, DAMPED) == n           # so J^T f is read by the damped solve every time
    lim = np.array([o["stats"][:, 1] - 4 * o["stats"][:, 0] for o in out])   # rows that are no contact's (contacts are 4 rows each)
    assert (lim.max(0) == 1).all() and lim.min() == 0                   # every env: the limit row appears (and goes again: the joint bounces back)
    qf = out[-1]["dbg"][DBG_QFRC_CON(11, 21):DBG_QFRC_CON(11, 21) + 21]
    assert qf[2] > 1.0                                                  # qfrc_constraint on the arm block is in the dump


def test_c_object_hits_the_hand_regime_switches_off_and_on_again(model_arrays):
    """The object thrown upwards into the thumb (env 0: leaves it again within the run; env 1: slower, stays in contact): no hand contact,
    hand contact in both envs, none again in env 0.  Only the pedestal's floor contacts remain then: 16 rows on block 2."""
    q, v = _picking(model_arrays, 2)
    q[1] = q[0]
    q[0, 9:12] = np.array([-0.2757, 0.5472, 0.3539 - 0.12], np.float32); v[0, 11] = 6.0
    q[1, 9:12] = np.array([-0.2757, 0.5472, 0.3539 - 0.10], np.float32); v[1, 11] = 3.0
    out, ctr, e = _both("jaco2_curtain_torque", q, v, np.zeros((2, 9)), calls=20, nsub=1, dump_every=2)
    assert all(c[SOLVES] == 2 for c in ctr)
    on = [c[FREE_ONLY] for c in ctr]
    first_off = on.index(0)
    assert on[0] == 2 and first_off >= 3 and on[-1] >= 1 and 0 in on[first_off:] and on[-1] > on[first_off]   # on, off, on again
    assert _total(ctr, DAMPED) == 2 * 20 - sum(on)                      # the damped solve runs exactly when the arm block carries rows
    assert (out[-1]["flags"] & 31 == 0).all()


def test_d_contacts_disabled_no_rows(model_arrays):
    q, v = _picking(model_arrays, 3)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    out, ctr, e = _both("jaco2_curtain_torque", q, v, ctrl, calls=5, nsub=2, dump_every=2, disable_contact=True)
    assert _total(ctr, SOLVES) == 0 and _total(ctr, JTF) == 0 and _total(ctr, DAMPED) == 0
    assert (out[-1]["stats"][:, 1] == 0).all() and np.abs(out[-1]["qpos"][:, :6] - q[:, :6]).max() > 1e-5   # ne == 0, and the arm moved


def test_e_arm_only_model_without_free_bodies():
    M = blob.load(os.path.join(emu_binding.ASSETS, "jaco2_reaching_torque.jacomdl"))
    q = workload.reset_states(M["qpos0"], 3, seed=11, f32_draws=True).astype(np.float32)
    v = np.zeros((3, 9), np.float32)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    q[:, 6:9] = 1.52                                                    # fingers beyond their limit (1.51): three limit rows, all on block 0
    out, ctr, e = _both("jaco2_reaching_torque", q, v, ctrl, calls=5, nsub=2, dump_every=2)
    n = _total(ctr, SOLVES)
    assert n > 0 and _total(ctr, FREE_ONLY) == 0 and _total(ctr, JTF) == n and _total(ctr, DAMPED) == n
    assert (out[-1]["flags"] & 31 == 0).all()


@pytest.mark.parametrize("how", ["finger_limits", "arm_joint_damping"])
def test_f_damped_solve_of_the_euler_stage_runs(model_arrays, how):
    """The branch that needs J^T f.  finger_limits: limit rows on the damped dofs themselves (regime off).  arm_joint_damping: the model with
    damping on arm joint 2 as well (has_damping == 2: the stage never delivers the damped solve), object at rest -- regime ON and J^T f
    read in every substep, the one combination in which the narrowed products and jt_vec meet."""
    q, v = _picking(model_arrays, 3)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    bb = None
    if how == "finger_limits":
        q[:, 6:9] = 1.52; ctrl[:, 6:9] = 1.51
    else:
        M2 = dict(model_arrays); d = np.array(M2["dof_damping"]).copy(); d[2] = 0.1; M2["dof_damping"] = d
        bb = blob.dumps(M2)
    out, ctr, e = _both("jaco2_curtain_torque", q, v, ctrl, calls=5, nsub=2, dump_every=2, blob_bytes=bb)
    n = _total(ctr, SOLVES)
    assert n == 3 * 10 and _total(ctr, DAMPED) == n and _total(ctr, JTF) == n
    assert _total(ctr, FREE_ONLY) == (0 if how == "finger_limits" else n)
    st = out[-1]["stats"]
    assert (st[:, 1] - 4 * st[:, 0] == (3 if how == "finger_limits" else 0)).all() and (out[-1]["flags"] == 0).all()
