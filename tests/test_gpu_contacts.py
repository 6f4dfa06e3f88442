"""GPU tier: the contact record (jaco_set_contact_record; BatchedMujoco.record_contacts / contacts / net_contact_force) on the MI355X --
oracle parity through every capacity tier, static equilibrium of the resting object, the auto_reset rule, and that recording changes no
result (default build at the env tier, _d30 build at the sim tier); and, beyond the reset draws, the placed-object sweep, the device's
record against the emulated kernel's, and the golden poses of the two-arm and the sensor model contact by contact."""
import os

import numpy as np
import pytest
import torch

import contacts_binding as cb
from mujoco_jaco_amd.modelc import blob
from mujoco_jaco_amd.physics import BatchedMujoco

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name="jaco2_curtain_torque"):
    return blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", name + ".jacomdl"))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def _np_record(c):
    """BatchedMujoco.contacts() -> numpy fields in the layout contacts_binding.compare reads (geom ids mapped back to kernel ids are not
    needed: compare maps through f_geom_orig, so pass the identity map's inputs)."""
    return {"ncon": c.ncon.cpu().numpy(), "dist": c.dist.cpu().numpy(), "pos": c.pos.cpu().numpy(), "frame": c.frame.cpu().numpy(),
            "force": c.force.cpu().numpy(), "geom": c.geom.cpu().numpy(), "body": c.body.cpu().numpy(), "dim": c.dim.cpu().numpy()}


def _compare_mjcf(R, i, oc, M):
    """contacts_binding.compare for a record whose geom ids are MJCF ids already (BatchedMujoco.contacts maps them)."""
    ident = dict(M)
    ident["f_geom_orig"] = np.arange(len(M["geom_type"]), dtype=np.int32)
    return cb.compare({k: v[i] for k, v in R.items()}, int(R["ncon"][i]), oc, ident)


def test_oracle_parity_through_every_tier(names):
    """1 024 envs, one substep from seeded states: resting objects (picking resets), fingers closed on the object (hull contacts, condim 6;
    after more closing, more rows than the light tier's 64 with the pedestal's contacts in the side buffer), and the hand-in-pedestal reset
    (68 contacts, huge tier).  In the emulator grasp(30) holds 72 rows on the light tier, grasp(20) 110 rows on the medium tier.  Every env's record against the oracle's forward(): exact counts, the emulator tests' bounds."""
    M = _model()
    B = 1024
    q = cb.rest_states(M, B)
    ctrl = np.zeros((B, 9))
    q[1] = cb.grasp_state(M, names, 40); ctrl[1] = cb.GRASP_CTRL
    q[2] = cb.grasp_state(M, names, 30); ctrl[2] = cb.GRASP_CTRL    # 72 rows, 16 of them the pedestal's: light tier + side rows
    q[3] = cb.deep_state(M)
    q[4] = cb.grasp_state(M, names, 20); ctrl[4] = cb.GRASP_CTRL    # 110 rows: medium tier
    sim = BatchedMujoco(B)
    sim.set_state(_dev(q), torch.zeros(B, 21, device="cuda:0"), torch.zeros(B, 21, device="cuda:0"))
    sim.record_contacts(128)
    sim.clear_flags()
    sim.send_forces(_dev(ctrl), nsub=1)
    R = _np_record(sim.contacts())
    fl, st = sim.flags().cpu().numpy(), sim.stats().cpu().numpy()
    sim.close()
    res = []
    for i in range(B):
        oc = cb.oracle_contacts(cb.oracle_forward("jaco2_curtain_torque", q[i], ctrl[i]), M)
        res.append((cb.deepest(oc), _compare_mjcf(R, i, oc, M)))
    worst, fclean, fdeep = cb.check_sweep(res)
    print("1 024 envs: worst [dist, pos, normal, force rel]", worst, "force rel clean %.2e deep %.2e" % (fclean, fdeep),
          "| grasp / deep envs: ncon", R["ncon"][1:5], "rows", st[1:5, 1], "flags", fl[1:5])
    for i in (1, 2, 3):   # the seeded grasp / deep states: the emulator tests' sharper bounds
        w = res[i][1]
        for kind, (bd, bp, bn) in cb.BOUNDS.items():
            assert w[kind][0] < bd and w[kind][1] < bp and w[kind][2] < bn, (i, kind, w[kind])
    assert (fl & 15).max() == 0
    assert fl[3] & 32 and R["ncon"][3] > 64                                      # recorded by a bigger tier (the huge one: 68 contacts)
    assert fl[4] & 32                                                            # ... and by the medium one
    side = [i for i in (1, 2) if st[i, 1] > 64 and not fl[i] & 32]               # light tier, more than its 64 rows: pedestal rows on the side
    assert side, (st[1:3], fl[1:3])


def test_resting_object_net_force_balances_its_weight():
    """Independent of the oracle: once the object has settled on its holder, the holder's net contact force on it plus its weight is zero
    (within 1 % of the weight).  The arm is held in its reset pose (state re-set every 50 substeps) so that it cannot reach the object."""
    M = _model()
    B = 256
    q0 = cb.rest_states(M, B)
    sim = BatchedMujoco(B)
    q = _dev(q0)
    sim.set_state(q, torch.zeros(B, 21, device="cuda:0"), torch.zeros(B, 21, device="cuda:0"))
    ctrl = torch.zeros(B, 9, device="cuda:0"); ctrl[:, 6:] = 0.6
    for _ in range(8):
        qp, qv, qa = sim.get_state()
        qp[:, :6] = q[:, :6]; qv[:, :6] = 0
        sim.set_state(qp.contiguous(), qv.contiguous(), qa)
        sim.send_forces(ctrl, nsub=50)
    sim.record_contacts(64)   # (an arm resting in the pedestal brings up to ~90 contacts: the object's must not be cut off)
    sim.send_forces(ctrl, nsub=1)
    c = sim.contacts()
    F = sim.net_contact_force("object_holder", "object_body", contacts=c).cpu().numpy()
    back = sim.net_contact_force("object_body", "object_holder", contacts=c).cpu().numpy()
    names = sim.contact_names
    ob = names.body_id("object_body")
    touching = ((c.body == ob).any(-1) & c.valid).cpu().numpy()
    others = (touching & ~((c.body[..., 0] == names.body_id("object_holder")) | (c.body[..., 1] == names.body_id("object_holder"))).cpu().numpy()).any(1)
    others |= (c.ncon > 64).cpu().numpy()   # (records past the capacity are not in the sum)
    vel = sim.get_state()[1][:, 9:12].abs().max(1).values.cpu().numpy()
    sim.close()
    weight = M["body_mass"][ob] * M["opt_gravity"]                              # [0, 0, -m g]
    err = np.abs(F + weight).max(1) / np.abs(weight).max()
    print("resting object: |F + m g| / m g max %.2e median %.2e over %d envs (%d with other contacts), object speed max %.1e"
          % (err[~others].max(), np.median(err[~others]), B, int(others.sum()), vel.max()))
    assert (~others).sum() >= B // 2 and vel[~others].max() < 1e-3
    assert err[~others].max() < 0.01
    assert np.array_equal(back, -F)                                              # Newton's third law, as the reduction forms it


def test_auto_reset_records_the_terminal_step():
    """With auto_reset the record after a step that ended an episode is that TERMINAL step's (the reset's forward pass writes nothing):
    bit-identical to an explicit step() followed by a masked reset(done) -- 8 192 envs with episode counters just below the time-out."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    B = 8192
    outs = []
    for auto in (True, False):
        env = JacoBatchedEnv(num_envs=B, task="picking", seed=31, auto_reset=auto, frame_skip=10)
        env.record_contacts(32)
        env.reset()
        gen = torch.Generator(device=env.device); gen.manual_seed(3)
        t = env.task_state(); t[:, 1] = torch.randint(695, 699, (B,), device=env.device, generator=gen).float(); env.set_task_state(t)
        rec = []
        for s in range(4):
            a = torch.rand(B, 7, device=env.device, generator=gen) * 2 - 1
            _, _, d, _ = env.step(a)
            d = d.clone()
            if not auto:
                env.reset(d)
            rec.append((d, env.sim._crec.clone(), env.sim._cn.clone()))
        outs.append(rec)
        env.close()
    ndone = 0
    for (d1, r1, n1), (d2, r2, n2) in zip(*outs):
        assert torch.equal(d1, d2)
        ndone += int(d1.sum())
        assert torch.equal(n1, n2) and torch.equal(r1.view(torch.int32), r2.view(torch.int32))
    assert ndone >= B // 2
    d1, r1, n1 = outs[0][-1]
    term = d1.bool()
    assert (n1[term] > 0).all()


def test_recording_changes_no_result():
    """20 env steps at 8 192 envs, record on (capacity 4: most envs overflow it) and off: obs, reward, done, state bit-identical."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    B = 8192
    outs = []
    for cap in (4, 0):
        env = JacoBatchedEnv(num_envs=B, task="picking", seed=5, auto_reset=True)
        if cap:
            env.record_contacts(cap)
        env.reset()
        gen = torch.Generator(device=env.device); gen.manual_seed(7)
        t = env.task_state(); t[:, 1] = torch.randint(0, 700, (B,), device=env.device, generator=gen).float(); env.set_task_state(t)
        res = []
        for s in range(20):
            a = torch.rand(B, 7, device=env.device, generator=gen) * 2 - 1
            o, r, d, _ = env.step(a)
            res.append((o.clone(), r.clone(), d.clone()))
        res.append(tuple(x.clone() for x in env.sim.get_state()))
        if cap:
            n = env.contacts().ncon
            live = ~d.bool()   # (an env reset inside the step has the reset's forward-pass statistics; its record is the terminal step's)
            assert (n > cap).any() and torch.equal(n[live], env.sim.stats()[:, 0][live])
        outs.append(res)
        env.close()
    for x, y in zip(*outs):
        for a, b in zip(x, y):
            assert torch.equal(a, b)


def test_two_arm_model_at_the_sim_tier():
    """_d30 build (jaco2_dual_torque, n_robots=2, sim tier): record on / off gives bit-identical states, and the arm-on-arm poses of
    tests/golden/dual_cross_poses.npz record the oracle's contact counts."""
    from mujoco_jaco_amd.env import JacoBatchedEnv
    from mujoco_jaco_amd import workload
    M = _model("jaco2_dual_torque")
    P = np.load(os.path.join(ROOT, "tests", "golden", "dual_cross_poses.npz"))
    B = 1024
    q = workload.reset_states_dual(M["qpos0"], B, seed=8)
    n = len(P["qpos"])
    q[:n] = P["qpos"]
    ctrl = np.zeros((B, 18)); ctrl[:, 6:9] = 0.6; ctrl[:, 15:18] = 0.6
    states, recs = [], None
    for cap in (64, 0):
        env = JacoBatchedEnv(num_envs=B, n_robots=2)
        sim = env.sim
        if cap:
            env.record_contacts(cap)
        sim.set_state(_dev(q), torch.zeros(B, 30, device="cuda:0"), torch.zeros(B, 30, device="cuda:0"))
        sim.send_forces(_dev(ctrl), nsub=1)
        if cap:
            c = env.contacts()
            recs = (c.ncon.cpu().numpy(), sim.stats()[:, 0].cpu().numpy())
        sim.send_forces(_dev(ctrl), nsub=5)
        states.append([t.clone() for t in sim.get_state()])
        env.close()
    for a, b in zip(*states):
        assert torch.equal(a, b)
    ncon, stat = recs
    assert np.array_equal(ncon[:n], P["ncon"]) and np.array_equal(ncon, stat)


# ---------------------------------------------------------------- contact by contact beyond the reset draws (contacts_binding.placed_states)
@pytest.fixture(scope="module")
def placed_sweep():
    """1 024 placed-object states (the emulator tier's 210 are the first of them), one substep in one launch, and the oracle's forward() of each
    with its knife-edge verdict: computed once, read by the tests below."""
    M = _model()
    B = 1024
    qs, regime = cb.placed_states(M, B, 7)
    sim = BatchedMujoco(B)
    sim.set_state(_dev(qs), torch.zeros(B, 21, device="cuda:0"), torch.zeros(B, 21, device="cuda:0"))
    sim.record_contacts(128)
    sim.clear_flags()
    sim.send_forces(torch.zeros(B, 9, device="cuda:0"), nsub=1)
    R = _np_record(sim.contacts())
    fl = sim.flags().cpu().numpy()
    sim.close()
    ocs = cb.oracle_states("jaco2_curtain_torque", M, qs, np.zeros(9), knife=True)
    return M, qs, regime, ocs, R, fl


def _ident(M):
    return np.arange(len(M["geom_type"]), dtype=np.int32)


def test_placed_object_sweep_matches_oracle_contact_by_contact(placed_sweep, names):
    """The emulator tier's sweep (tests/test_contacts_emu.py) at 1 024 envs on the device: same criteria, caps and bounds, census minima x 4.
    Measured on the emulator at these states: box-box pairs 1: 427, 2: 235, 3: 95, 4: 329, 5: 36, 6: 7, plane-box 1: 33, 2: 44, 3: 20, 342
    box-hull contacts, 260 states with three pairs, 0 left out; analytic dist 8.8e-8, pos 3.2e-7, normal 3.5e-7; MPR dist 3.7e-7, pos 2.3e-7, normal
    1.5e-4, none beyond BOUNDS_SWEEP, consistency 1.2e-7, optimality 4.9e-7; force 3.3e-6 / 1.8e-5."""
    M, qs, regime, ocs, R, fl = placed_sweep
    cb.check_census(*cb.census(ocs, M, bodies=(names["body"].index("object_body"), names["body"].index("object_dest"))), scale=4)
    skip = {i for i, oc in enumerate(ocs) if oc["knife"]}
    print("knife-edge states left out: %d of %d" % (len(skip), len(qs)))
    assert len(skip) <= cb.KNIFE_CAP * len(qs)
    assert (fl & 31).max() == 0
    s = cb.summarise(cb.tabulate(R, ocs, M, gmap=_ident(M), skip=skip))
    cb.print_summary("placed sweep (MI355X)", s)
    cb.check_contacts(s, cb.PLACED)


def test_device_record_against_the_emulated_kernel(placed_sweep):
    """The first 210 placed states under the wavefront emulator: the device's record has the same counts and the same geom pairs in the same
    order; dist, pos, normal and force (relative to the env's largest normal force) within cb.DEVICE_VS_EMU -- a wave primitive or a
    compiler choice the emulator does not model would show here.  Not expected to be bit for bit."""
    from emu_binding import EmuEnv
    M, qs, regime, ocs, R, fl = placed_sweep
    n = 210
    e = EmuEnv(nenv=n)
    e.qpos[:] = qs[:n]; e.qvel[:] = 0; e.qacc_ws[:] = 0
    rec, ncon = e.step_rec(np.zeros(9), nsub=1, cap=128)
    E = cb.unpack(rec, ncon)
    assert np.array_equal(ncon, R["ncon"][:n])
    worst = np.zeros(4)
    for i in range(n):
        k = int(ncon[i])
        assert np.array_equal(M["f_geom_orig"][E["geom"][i, :k]], R["geom"][i, :k]), i
        assert np.array_equal(E["dim"][i, :k], R["dim"][i, :k]), i
        if k:
            fmax = max(np.abs(E["force"][i, :k, 0]).max(), 1e-9)
            worst = np.maximum(worst, [np.abs(E["dist"][i, :k] - R["dist"][i, :k]).max(), np.abs(E["pos"][i, :k] - R["pos"][i, :k]).max(),
                                       np.abs(E["frame"][i, :k, 0] - R["frame"][i, :k, 0]).max(), np.abs(E["force"][i, :k] - R["force"][i, :k]).max() / fmax])
    print("device against emulator, %d states, %d contacts: worst [dist, pos, normal, force rel]" % (n, int(ncon.sum())), worst)
    assert (worst <= cb.DEVICE_VS_EMU).all(), worst


@pytest.mark.parametrize("model,poses,bounds,want", [
    ("jaco2_dual_torque", "dual_cross_poses.npz", cb.DUAL_POSES, {(7, 7): 79, (6, 7): 178, (6, 6): 72}),
    ("jaco2_curtain_torque_sensor", "sensor_post_poses.npz", cb.SENSOR_POSES, {(5, 7): 29, (5, 6): 8})])
def test_golden_poses_match_oracle_contact_by_contact(model, poses, bounds, want):
    """The arm-on-arm poses on the _d30 build (through JacoBatchedEnv(n_robots=2)) and the arm-on-cylinder poses of the sensor model on the
    _d12 build, fp32-rounded, zero ctrl, one substep: hull-hull, box-hull, box-box, cylinder-hull and cylinder-box contacts one by one
    against the oracle's, with the emulator tier's checks and bounds (tests/test_contacts_emu.py, same test name)."""
    from collections import Counter
    M = _model(model)
    P = np.load(os.path.join(ROOT, "tests", "golden", poses))
    qs = cb._f32(P["qpos"])
    B, nv, nu = len(qs), int(M["nv"][0]), int(M["nu"][0])
    if model == "jaco2_dual_torque":
        from mujoco_jaco_amd.env import JacoBatchedEnv
        owner = JacoBatchedEnv(num_envs=B, n_robots=2)
        sim = owner.sim
    else:
        owner = sim = BatchedMujoco(B, robot_file=model)
    sim.record_contacts(64)
    sim.set_state(_dev(qs), torch.zeros(B, nv, device="cuda:0"), torch.zeros(B, nv, device="cuda:0"))
    sim.clear_flags()
    sim.send_forces(torch.zeros(B, nu, device="cuda:0"), nsub=1)
    R = _np_record(sim.contacts())
    fl = sim.flags().cpu().numpy()
    owner.close()
    assert (fl & 31).max() == 0 and np.array_equal(R["ncon"], P["ncon"])
    ocs = cb.oracle_states(model, M, qs, np.zeros(nu))
    rows = cb.tabulate(R, ocs, M, gmap=_ident(M))
    assert Counter(tuple(sorted(int(M["geom_type"][g]) for g in r["geoms"])) for r in rows) == want
    s = cb.summarise(rows)
    cb.print_summary(model + " golden poses (MI355X)", s)
    cb.check_contacts(s, bounds)
