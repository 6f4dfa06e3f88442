"""CPU tier: the row builder's free-column Jacobian pass (collision.h stage_contact_rows, JACO_ROWS_FREE) changes no bit.

When every contact of an env moves exactly one free body and nothing else -- no chain-mask bit on the arm/finger dof block [0, JB0) --
the Jacobian pass maps lane = (contact slot, dof of that body): ten contacts per pass in every layout instead of three (two in d30), every
other column of those rows written as +0 by the row lanes.  Two emulator builds of the same sources -- the default one and -DJACO_ROWS_FREE=0 (every pass over all columns: what the
kernel did before) -- run the same inputs, and everything the kernel hands back must be equal byte for byte: qpos, qvel,
qacc_warmstart, sensordata, flags, stats, the contact record and the debug dump of the last substep (its qfrc_constraint goes through
jt_vec, which reads every column of every row, the zero-filled ones included).

Each case asserts from the emulator's event counters (14: Jacobian passes over the free columns, 15: over all columns; 8 / 11: the
Newton stage's constrained solves / those without a row on the arm/finger block) and the recorded contact counts that it ran what it
is about.  The all-columns build must never count a free-column pass.
"""
import os
import subprocess

import numpy as np
import pytest

import emu_binding
from emu_binding import EmuEnv
from mujoco_jaco_amd import workload
from mujoco_jaco_amd.modelc import blob

SOLVES, FREE_ONLY, COMPACT, FULL = 8, 11, 14, 15
DBG_QFRC_CON = lambda nb, nv: 3 * nb + 9 * nb + nv * nv + 4 * 24   # physics_kernel.h JDBG_QFRC_CON


def _variant(layout="", tag="rowsall", flag="-DJACO_ROWS_FREE=0"):
    """The all-columns build of a layout (or another A/B build: tag, flag), through the emulator Makefile's own pattern rule (its flags
    given on the command line)."""
    name = "libjaco_emu%s_%s.so" % (layout, tag)
    flags = ("$(FLAGS%s) " % layout if layout else "") + flag
    subprocess.check_call(["make", "-s", "-C", emu_binding.EMU_DIR, name, "LIBS=" + name, "FLAGS%s_%s=%s" % (layout, tag, flags)])
    return "%s_%s" % (layout, tag)


def _counters(L):
    return {i: L.emu_get_counter(i, 1) for i in (SOLVES, FREE_ONLY, COMPACT, FULL)}


def _run(layout, model, q, v, ctrl, calls, nsub, dump_every):
    """`calls` ctrl-level calls of `nsub` substeps, contact record on, env 0 dumped in every `dump_every`-th call: what the kernel handed
    back call by call, and the counters call by call."""
    e = EmuEnv(model, nenv=len(q), layout=layout)
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
        e._physics_step(ctrl, nsub, False, rec, ncon, cap, 0 if dump else -1)
        ctr.append(_counters(e.L))
        out.append(dict(qpos=e.qpos.copy(), qvel=e.qvel.copy(), qacc_ws=e.qacc_ws.copy(), sens=e.sensordata.copy(), flags=e.flags.copy(),
                        stats=e.stats.copy(), rec=rec.copy(), ncon=ncon.copy(), dbg=e.dbg.copy(), dumped=bool(dump)))
    return out, ctr


def _both(model, q, v, ctrl, calls, nsub, dump_every=2, tag="rowsall", flag="-DJACO_ROWS_FREE=0"):
    from mujoco_jaco_amd import _lib as product_lib
    layout = product_lib.variant_for(open(os.path.join(emu_binding.ASSETS, model + ".jacomdl"), "rb").read())   # (the loader's own choice)
    new = _run(layout, model, q, v, ctrl, calls, nsub, dump_every)
    old = _run(_variant(layout, tag, flag), model, q, v, ctrl, calls, nsub, dump_every)
    for k, (x, y) in enumerate(zip(new[0], old[0])):
        for name in ("qpos", "qvel", "qacc_ws", "sens", "flags", "stats", "rec", "ncon", "dbg"):
            assert x[name].tobytes() == y[name].tobytes(), "%s: %s differs in call %d" % (model, name, k)
    for cn, co in zip(new[1], old[1]):
        assert (cn[SOLVES], cn[FREE_ONLY]) == (co[SOLVES], co[FREE_ONLY]) and (co[COMPACT] == 0 if tag == "rowsall" else cn == co)
    return new[0], new[1], old[1]


def _total(ctr, i):
    return sum(c[i] for c in ctr)


def _picking(M, n, seed=11):
    return workload.reset_states(M["qpos0"], n, seed=seed, f32_draws=True).astype(np.float32), np.zeros((n, 21), np.float32)


def _passes(ncon, per):
    return int(sum(-(-int(n) // per) for n in ncon))


def test_a_picking_reset_distribution_mostly_free_columns(model_arrays):
    q, v = _picking(model_arrays, 64)
    ctrl = workload.random_ctrl(64, seed=12, scale=0.2)
    out, ctr, ctr_all = _both("jaco2_curtain_torque", q, v, ctrl, calls=4, nsub=2)
    light = out[-1]["stats"][:, 0] <= 32
    assert (out[-1]["flags"][light] & 15 == 0).all() and _total(ctr, SOLVES) == 64 * 8
    # the object on its holder and the pedestal on the floor: 8 contacts, one free-column pass where the all-columns build takes three
    # (the full-width passes belong to the few envs whose hand starts in contact: tens of contacts each, three to a pass)
    assert (out[-1]["ncon"] == 8).sum() >= 48
    assert _total(ctr, COMPACT) >= 48 * 8 and _total(ctr, COMPACT) >= _total(ctr, FREE_ONLY)
    assert _total(ctr, COMPACT) + _total(ctr, FULL) < _total(ctr_all, FULL)
    assert 2 * _total(ctr, FREE_ONLY) > _total(ctr, SOLVES)
    # the dump's qfrc_constraint reads the zero-filled columns: nothing on the arm/finger dofs of env 0, the contact forces on the free bodies
    for o in out:
        qf = o["dbg"][DBG_QFRC_CON(11, 21):DBG_QFRC_CON(11, 21) + 21]
        assert (np.abs(qf[9:]).max() > 1.0 and not qf[:9].any()) if o["dumped"] else not o["dbg"].any()


def test_b_limit_rows_on_the_arm_block_with_all_free_contacts(model_arrays):
    """Limit rows on the arm/finger block next to contacts on the free bodies only: the free-column pass feeds the full-width solver, which
    reads the zero-filled columns of the contact rows in M v, J v, the Hessian and J^T f.  The joints at their limit are the three finger
    joints (dofs 6..8 of block [0, 9)), beyond their upper limit of 1.51: in this model an arm joint at its limit folds the arm onto itself
    (joint 3 at 0.335: links 2 and 4 touch, 10 contacts), which is case (c)'s path, not this one."""
    q, v = _picking(model_arrays, 3)
    ctrl = workload.random_ctrl(3, seed=12, scale=0.2)
    q[:, 6:9] = 1.52; ctrl[:, 6:9] = 1.51
    out, ctr, ctr_all = _both("jaco2_curtain_torque", q, v, ctrl, calls=6, nsub=1)
    for o, c, ca in zip(out, ctr, ctr_all):
        assert (o["ncon"] == 8).all() and (o["stats"][:, 1] == 32 + 3).all() and (o["flags"] == 0).all()
        assert (c[COMPACT], c[FULL]) == (3, 0) and ca[FULL] == 3 * 3
        assert c[SOLVES] == 3 and c[FREE_ONLY] == 0                     # limit rows on block 0: the solver runs over all columns
    qf = out[-1]["dbg"][DBG_QFRC_CON(11, 21):DBG_QFRC_CON(11, 21) + 21]
    assert out[-1]["dumped"] and (qf[6:9] < -1e-3).all() and not qf[:6].any() and np.abs(qf[9:]).max() > 1.0


def test_c_contacts_on_the_arm_block_take_the_full_width_pass(model_arrays):
    """Env 0: seed 41's env 200 of the picking reset distribution, the hand inside the pedestal (68 contacts: the huge tier's row builder,
    two chunks -- 64 contacts over all columns, then the pedestal's four floor contacts over the free columns: the mapping changes between
    chunks of one call).  Env 1: the object thrown upwards into the thumb (tests/test_newton_regime_emu.py case c): free columns while it
    flies, all columns while it touches the hand, free columns again."""
    q, v = _picking(model_arrays, 2)
    q[1] = q[0]
    q[0] = workload.reset_states(model_arrays["qpos0"], 256, seed=41, f32_draws=True).astype(np.float32)[200]
    q[1, 9:12] = np.array([-0.2757, 0.5472, 0.3539 - 0.12], np.float32); v[1, 11] = 6.0
    out, ctr, ctr_all = _both("jaco2_curtain_torque", q, v, np.zeros((2, 9)), calls=20, nsub=1)
    assert (out[0]["stats"][0, 0], out[0]["stats"][0, 1]) == (68, 308) and out[0]["flags"][0] & 32
    # call 0: env 0's last chunk and env 1 (the pedestal's four floor contacts) take one free-column pass each; the all-columns build two
    # full-width passes each in their place
    assert out[0]["ncon"][1] == 4 and ctr[0][COMPACT] == 2 and ctr[0][FULL] == ctr_all[0][FULL] - 4 and ctr[0][FULL] >= 22
    hand = [k for k, o in enumerate(out) if o["ncon"][1] > 4]           # env 1: the calls with a contact on the hand
    assert hand and hand[0] >= 3 and hand[-1] < 19 and out[-1]["ncon"][1] == 4
    for k, (o, c, ca) in enumerate(zip(out, ctr, ctr_all)):
        if o["ncon"][0] > 64:                                           # (env 0 keeps its free-column chunk while it has one)
            assert c[COMPACT] == (1 if k in hand else 2) and c[FREE_ONLY] == (0 if k in hand else 1)
    assert ctr[-1][COMPACT] == 1 and ctr[-1][FREE_ONLY] == 1            # env 1 at the end: free again


def test_c_contacts_between_the_two_free_bodies_take_the_full_width_pass(model_arrays):
    """The object standing on (in) the pedestal instead of the holder: four contacts that move both free bodies, no row on the arm/finger
    block.  The Newton stage is in its narrow regime, the row builder is not: a contact with two blocks of columns has no six-column slot."""
    q, v = _picking(model_arrays, 2)
    q[:, 9:11] = q[:, 16:18]; q[:, 11] = [0.19, 0.24]
    out, ctr, ctr_all = _both("jaco2_curtain_torque", q, v, np.zeros((2, 9)), calls=4, nsub=1)
    for o, c, ca in zip(out, ctr, ctr_all):
        assert (o["ncon"] == 8).all() and (o["flags"] == 0).all()
        assert (c[COMPACT], c[FULL]) == (0, 6) and ca[FULL] == 6 and c[FREE_ONLY] == c[SOLVES] == 2
    bodies = out[0]["rec"].reshape(2, 16, 24)[0, :8, 21:23].view(np.int32)   # the contacts' original bodies
    assert sorted(map(tuple, bodies.tolist())) == [(0, 53)] * 4 + [(51, 53)] * 4


@pytest.mark.parametrize("pose, ncon", [("air", 4), ("corner", 5), ("edge", 6), ("flat", 8)])
def test_d_contact_counts_on_both_sides_of_a_pass_boundary(model_arrays, pose, ncon):
    """Contact counts of the free-column pass (default layout), reached by the object's pose over its holder: in the air 4 (the pedestal's
    floor contacts alone), on a corner 5, on an edge 6, flat 8 -- all four confirmed on the emulator; 7 was not looked for.  They sit on
    both sides of the all-columns pass's boundaries (3 and 6 contacts); the free-column pass holds ten contacts, and more than ten
    single-body contacts were not reached with this model's one object (case (e) has the d12 counts).  One substep per call: the
    recorded count is the count the row builder saw."""
    def quat(axis, ang):
        a = np.asarray(axis, float) / np.linalg.norm(axis)
        return np.r_[np.cos(ang / 2), np.sin(ang / 2) * a].astype(np.float32)
    dz, qu = {"air": (0.10, quat([1, 0, 0], 0.0)), "corner": (0.02, quat([1, 1, 0], np.arccos(1 / np.sqrt(3)))),
              "edge": (0.012, quat([1, 0, 0], np.pi / 4)), "flat": (0.0, quat([1, 0, 0], 0.0))}[pose]
    q, v = _picking(model_arrays, 1)
    q[0, 11] += dz; q[0, 12:16] = qu
    out, ctr, ctr_all = _both("jaco2_curtain_torque", q, v, np.zeros((1, 9)), calls=2, nsub=1, dump_every=1)
    for o, c, ca in zip(out, ctr, ctr_all):
        assert o["ncon"][0] == ncon and o["stats"][0, 1] == 4 * ncon and o["flags"][0] == 0
        assert (c[COMPACT], c[FULL]) == (1, 0) and ca[FULL] == _passes([ncon], 3)
        assert c[FREE_ONLY] == c[SOLVES] == 1


def test_e_d12_layout_one_object_ten_contacts_per_pass():
    """The 12-hinge layout (six free columns, ten contacts per free-column pass) with its one-object models.  jaco2_curtain_torque_sensor:
    the object on the floor between the static cylinders, 5 contacts or 1.  jaco2_curtain_torque_old: 4 contacts next to three finger
    limit rows (free-column pass, full-width solver)."""
    for model, z, want in (("jaco2_curtain_torque_sensor", [0.0, 0.03, 0.05], [5, 5, 1]), ("jaco2_curtain_torque_old", [0.0, 0.02], [4, 4])):
        M = blob.load(os.path.join(emu_binding.ASSETS, model + ".jacomdl"))
        q = np.tile(M["qpos0"].astype(np.float32), (len(z), 1))
        q[:, 14] = z
        out, ctr, ctr_all = _both(model, q, np.zeros((len(z), 18), np.float32), np.zeros((len(z), int(M["nu"][0]))), calls=3, nsub=1, dump_every=1)
        for o, c, ca in zip(out, ctr, ctr_all):
            assert o["ncon"].tolist() == want and (o["flags"] == 0).all()
            assert (c[COMPACT], c[FULL]) == (len(z), 0) and ca[FULL] == _passes(want, 3)
            assert c[FREE_ONLY] == (c[SOLVES] if model.endswith("sensor") else 0) and c[SOLVES] == len(z)


def test_e_d30_layout_two_objects_twelve_contacts_cross_the_pass_boundary():
    """The two-arm layout (30 dofs, two free objects, two contacts per all-columns pass): both objects on the floor.  Env 0: 12 contacts, each
    on one object -- more than the ten of one free-column pass, so two; env 1: 4 contacts, one pass."""
    M = blob.load(os.path.join(emu_binding.ASSETS, "jaco2_dual_torque.jacomdl"))
    q = np.tile(M["qpos0"].astype(np.float32), (2, 1))
    q[:, 20] = [0.0, 0.03]; q[:, 27] = [0.03, 0.05]
    out, ctr, ctr_all = _both("jaco2_dual_torque", q, np.zeros((2, 30), np.float32), np.zeros((2, int(M["nu"][0]))), calls=3, nsub=1, dump_every=1)
    for o, c, ca in zip(out, ctr, ctr_all):
        assert o["ncon"].tolist() == [12, 4] and o["stats"][:, 1].tolist() == [48, 16] and (o["flags"] == 0).all()
        assert (c[COMPACT], c[FULL]) == (2 + 1, 0) and ca[FULL] == 6 + 2 and c[FREE_ONLY] == c[SOLVES] == 2


@pytest.mark.parametrize("case", ["picking", "finger_limits", "hand_in_pedestal"])
def test_f_fused_products_of_the_newton_stage_change_no_bit(model_arrays, case):
    """physics_kernel.h mat_vec_rows_dot (JACO_NEWTON_FUSE): M v and J v of the Newton stage's start point and search directions behind one
    set of broadcasts, against the build with the two separate products (-DJACO_NEWTON_FUSE=0), byte for byte -- in the narrow regime
    (picking: free bodies only) and over all columns (finger limit rows; the bigger tiers' two and more rows per lane)."""
    kw = dict(tag="nofuse", flag="-DJACO_NEWTON_FUSE=0")
    q, v = _picking(model_arrays, 4)
    ctrl = workload.random_ctrl(4, seed=12, scale=0.2)
    if case == "finger_limits":
        q[:, 6:9] = 1.52; ctrl[:, 6:9] = 1.51
    if case == "hand_in_pedestal":
        q[0] = workload.reset_states(model_arrays["qpos0"], 256, seed=41, f32_draws=True).astype(np.float32)[200]
    out, ctr, _ = _both("jaco2_curtain_torque", q, v, ctrl, calls=4, nsub=2, **kw)
    n = _total(ctr, SOLVES)
    assert n == 32 and _total(ctr, FREE_ONLY) == {"picking": n, "finger_limits": 0, "hand_in_pedestal": n - 8}[case]
    if case == "hand_in_pedestal":
        assert out[-1]["flags"][0] & 32 and out[-1]["stats"][0, 1] > 256     # the huge tier: eight rows per lane
