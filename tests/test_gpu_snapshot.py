"""GPU tier: env snapshots (jaco_save_envs / jaco_load_envs; BatchedMujoco.save_envs / load_envs, JacoBatchedEnv.save_envs / load_envs /
clone_envs) on the MI355X.  A restored env continues BIT FOR BIT -- on a mixed batch (envs in bigger tiers, non-zero compensation words,
frozen finished envs), into the same handle and into new ones, with the separating-direction cache and the merged queue preparation on
and off -- which today's accessors (set_state + set_task_state + set_markers) cannot do; fan-out, the sim-tier builds, launch counts and
the error paths.  Every bound here is exact equality of 32-bit words: a row holds every word a step reads, nothing is measured.

One field is compared differently: `cost` is the shader-clock time the env's last step took (launch order only, bit-neutral).  It is a
time measurement, so two runs of the same steps do not reproduce it; the end-of-run snapshots are compared in every word but that one."""
import ctypes

import numpy as np
import pytest
import torch

import snapshot_binding as sb
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.env import EnvSnapshot, JacoBatchedEnv
from mujoco_jaco_amd.physics import BatchedMujoco

pytestmark = pytest.mark.gpu
B, PRE, M = 4096, 40, 6


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.to(torch.int32)


def _make(auto_reset, seed=1000, num_envs=B, task="picking", **options):
    env = JacoBatchedEnv(num_envs=num_envs, task=task, seed=seed, auto_reset=auto_reset)
    for k, v in options.items():
        env.sim.set_option(k, v)
    env.reset()
    return env


def _spread_counters(env, seed=2000):
    """Episode counters spread over the 700-step episode (bench.py's workload): some envs time out inside the pre-roll."""
    gen = torch.Generator(device=env.device); gen.manual_seed(seed)
    ts = env.task_state(); ts[:, 1] = torch.randint(0, env.task_max_steps, (env.num_envs,), device=env.device, generator=gen).float(); env.set_task_state(ts)


def _actions(n, num_envs, seed, nact=7):
    g = torch.Generator(); g.manual_seed(seed)
    return (torch.rand(n, num_envs, nact, generator=g) * 2 - 1).to("cuda:0")


def _everything(env):
    qpos, qvel, qacc = env.sim.get_state()
    return {"qpos": qpos, "qvel": qvel, "qacc_ws": qacc, "task": env.task_state(), "marker": env.markers().reshape(env.num_envs, 24), "flags": env.sim.flags(),
            "sensordata": env.sim.sensordata()}


def _run(env, acts):
    """Step through acts; every step's (obs, reward, done) and the final state, as 32-bit words."""
    out = []
    for a in acts:
        obs, rew, done, _ = env.step(a)
        out += [_bits(obs).clone(), _bits(rew).clone(), _bits(done.view(torch.uint8)).clone()]
    return out + [_bits(v) for v in _everything(env).values()]


def _same(ta, tb):
    return all(torch.equal(x, y) for x, y in zip(ta, tb))


def _table(env):
    return sb.table(env.sim.nq, env.sim.nv, env.sim.nsensor, {"picking": 0, "reaching": 2}[env.task])


def _rows_but_cost(env, rows):
    w, off = _table(env)[1]["cost"]
    keep = torch.ones(rows.shape[1], dtype=torch.bool, device=rows.device); keep[off:off + w] = False
    return rows[:, keep], rows[:, off:off + w]


def _prerolled(auto_reset, acts, **options):
    env = _make(auto_reset, **options)
    _spread_counters(env)
    for a in acts[:PRE - 1]:
        env.step(a)
    # a quarter of the running envs start a new episode one step before the snapshot: ~1 % of the picking resets put the hand inside the
    # pedestal (tens of contacts: a bigger tier's work), which is where envs with a tier hint come from under random actions
    fresh = (torch.arange(B, device=env.device) % 4 == 0) & (env.task_state()[:, 3] == 0)
    env.reset(fresh)
    env.step(acts[PRE - 1])
    return env


def _assert_mix(env, snap, auto_reset):
    """The batch at snapshot time is mixed, read from the rows themselves through the table of csrc/snapshot.h."""
    W, tab, fp = _table(env)
    assert W == env.sim.snapshot_words and snap.rows.shape == (B, W) and bool((snap.rows[:, 0] == np.int32(np.uint32(fp))).all())
    col = lambda f: snap.rows[:, tab[f][1]:tab[f][1] + tab[f][0]]
    hint = col("hint")[:, 0]
    lo = (col("qpos_lo") != 0).any(1)
    done = col("task").view(torch.float32)[:, 3] != 0
    counts = {"hint > 0": int((hint > 0).sum()), "hint == 0": int((hint == 0).sum()), "non-zero qpos_lo": int(lo.sum()), "frozen done": int(done.sum())}
    print("mix at snapshot time (%d envs, auto_reset %d, %d pre-roll steps):" % (B, auto_reset, PRE), counts)
    assert counts["hint > 0"] > 0 and counts["hint == 0"] > 0 and counts["non-zero qpos_lo"] > 0
    if not auto_reset:
        assert counts["frozen done"] > 0
    return counts


@pytest.mark.parametrize("auto_reset", [False, True])
def test_restore_continues_bit_for_bit_and_the_old_accessors_do_not(auto_reset):
    """Run A: pre-roll, save, M steps.  Run B: load the rows back into the same handle, the same M steps.  Every output of every step, the
    final state and a second snapshot are equal word for word (the second snapshot: but for `cost`, see the module docstring).  Then the
    same restore through set_state + set_task_state + set_markers: NOT bit-identical (asserted only as > 0 differing envs)."""
    acts = _actions(PRE + M, B, 7)
    env = _prerolled(auto_reset, acts)
    snap = env.save_envs()
    old = _everything(env)
    obs0 = snap.obs.clone()
    _assert_mix(env, snap, auto_reset)
    ta = _run(env, acts[PRE:])
    end_a = env.save_envs().rows.clone()
    obs = env.load_envs(snap)
    assert torch.equal(_bits(obs), _bits(obs0)) and torch.equal(env.save_envs().rows, snap.rows)
    tb = _run(env, acts[PRE:])
    end_b = env.save_envs().rows
    assert _same(ta, tb)
    (ra, ca), (rb, cb) = _rows_but_cost(env, end_a), _rows_but_cost(env, end_b)
    print("end-of-run snapshots: %d of %d cost words differ (time stamps); every other word compared" % (int((ca != cb).sum()), ca.numel()))
    assert torch.equal(ra, rb)
    # today's accessors
    env.sim.set_state(old["qpos"], old["qvel"], old["qacc_ws"]); env.set_task_state(old["task"]); env.set_markers(old["marker"])
    tc = _run(env, acts[PRE:])
    qa, qc = ta[-7], tc[-7]           # final qpos words of run A and of the accessor restore
    differ = int((qa != qc).any(1).sum())
    print("restore with set_state + set_task_state + set_markers: %d of %d envs end with different qpos words" % (differ, B))
    assert differ > 0
    env.close()


def test_load_is_independent_of_what_the_destination_held():
    """The rows go (a) into the same handle after 20 further steps, (b) into NEW handles with the same seed, with the separating-direction
    cache and the merged queue preparation on and off.  All continue exactly as run A did: nothing outside the row matters."""
    acts = _actions(PRE + M + 20, B, 7)
    env = _prerolled(False, acts)
    snap = env.save_envs()
    _assert_mix(env, snap, False)
    ta = _run(env, acts[PRE:PRE + M])
    for a in acts[PRE + M:]:
        env.step(a)
    env.load_envs(snap)
    assert _same(ta, _run(env, acts[PRE:PRE + M])), "same handle, 20 steps later"
    env.close()
    host = snap.to("cpu")
    for sep, mp in ((1, 1), (0, 0), (1, 0)):
        new = _make(False, sep_cache=sep, merge_prepare=mp)
        new.step(acts[0])                                  # (a launch of its own first: the queues of the new handle have been in use)
        new.load_envs(host)
        assert _same(ta, _run(new, acts[PRE:PRE + M])), "new handle, sep_cache %d merge_prepare %d" % (sep, mp)
        new.close()


def test_fan_out_with_clone_envs():
    """clone_envs(0): every env becomes env 0.  With injected noise (identical rows) and identical actions all envs stay identical to env 0;
    with different actions they part.  Without injected noise only the physical state right after the clone is asserted (the clones draw
    their sub-goal noise from their own index's stream: the documented RNG rule)."""
    n, m = 1024, 4
    env = _make(False, num_envs=n)
    acts = _actions(6 + m, n, 11)
    for a in acts[:6]:
        env.step(a)
    obs = env.clone_envs(0)
    st = _everything(env)
    for k, v in st.items():
        assert bool((_bits(v) == _bits(v)[0]).all()), k
    assert bool((_bits(obs) == _bits(obs)[0]).all())
    scratch = env.save_envs()
    noise = torch.rand(1, 12, device=env.device).expand(n, 12).contiguous()
    env.set_noise(noise)
    for a in acts[6:]:
        obs, rew, done, _ = env.step(a[:1].expand(n, 7).contiguous())
        assert bool((_bits(obs) == _bits(obs)[0]).all()) and bool((_bits(rew) == _bits(rew)[0]).all()) and bool((done == done[0]).all())
    for k, v in _everything(env).items():
        assert bool((_bits(v) == _bits(v)[0]).all()), k
    env.load_envs(scratch)
    for a in acts[6:]:
        obs, _, _, _ = env.step(a)
    q = _bits(env.sim.get_state()[0])
    assert int((q != q[0]).any(1).sum()) > n // 2
    # masked clone: only the masked envs change
    before = _bits(env.sim.get_state()[0]).clone()
    mask = torch.zeros(n, dtype=torch.bool, device=env.device); mask[5] = mask[9] = True
    env.clone_envs(torch.full((n,), 3), mask)
    after = _bits(env.sim.get_state()[0])
    want = before.clone(); want[5] = before[3]; want[9] = before[3]
    assert torch.equal(after, want)
    env.close()


@pytest.mark.parametrize("robot_file", ["jaco2_curtain_torque_sensor", "jaco2_torque", "jaco2_dual_torque", "jaco2_reaching_torque"])
def test_sim_tier_builds(robot_file):
    """The d12 and d30 builds (and the contact-free model of the default build) at the sim tier: save, send_forces m times, load, repeat."""
    n = 512
    sim = BatchedMujoco(n, robot_file=robot_file)
    g = torch.Generator(); g.manual_seed(3)
    ctrl = ((torch.rand(8, n, sim.nu, generator=g) * 2 - 1) * 0.3).to(sim.device)
    for c in ctrl[:4]:
        sim.send_forces(c, nsub=25)
    rows = sim.save_envs()
    assert rows.shape == (n, sim.snapshot_words) and sim.snapshot_words % 4 == 0

    def run():
        for c in ctrl[4:]:
            sim.send_forces(c, nsub=25)
        return [_bits(t) for t in (*sim.get_state(), sim.flags())] + ([_bits(sim.sensordata())] if sim.nsensor else [])   # (jaco2_torque has no sensor)

    ta = run()
    sim.load_envs(rows)
    assert _same(ta, run())
    # ... and through an index list: the second half := rows of the first half, reversed
    half = n // 2
    sim.load_envs(rows)
    sim.load_envs(rows, envs=torch.arange(half, n), row_index=torch.arange(half - 1, -1, -1))
    q = _bits(sim.get_state()[0])
    assert torch.equal(q[half:], q[:half].flip(0))
    print("%s: W = %d words" % (robot_file, sim.snapshot_words))
    sim.close()


def test_one_launch_each_and_error_paths():
    """launch_count() rises by exactly 1 per save / load (no hidden launches); JACO_EINVAL cases; a foreign row (a `reaching` handle's)
    leaves state untouched and sets JACO_FLAG_BAD_SNAPSHOT in exactly the addressed envs; out-of-range indices are skipped."""
    n = 256
    env = _make(False, num_envs=n)
    sim = env.sim
    for a in _actions(3, n, 5):
        env.step(a)
    sim.launch_count()
    rows = sim.save_envs()
    assert sim.launch_count() == 1
    sim.load_envs(rows)
    assert sim.launch_count() == 1
    idx = torch.tensor([4, 9], dtype=torch.int32, device=sim.device)
    sim.save_envs(idx); sim.load_envs(rows, envs=idx, row_index=idx)
    assert sim.launch_count() == 2
    L, h, st = sim.L, sim.h, sim._stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.jaco_snapshot_words(h) == rows.shape[1]
    assert L.jaco_save_envs(h, None, -1, p(rows), st) == -1
    assert L.jaco_save_envs(h, p(idx), n + 1, p(rows), st) == -1
    assert L.jaco_save_envs(h, None, n, None, st) == -1
    assert L.jaco_save_envs(h, None, 2, p(rows), st) == -1            # no index list: n must be num_envs
    assert L.jaco_save_envs(h, p(idx), 2, ctypes.c_void_p(rows.data_ptr() + 4), st) == -1   # rows are 16-byte aligned
    assert L.jaco_load_envs(h, None, n - 1, p(rows), n, None, st) == -1
    assert L.jaco_load_envs(h, p(idx), 2, None, n, None, st) == -1
    assert L.jaco_load_envs(h, p(idx), 2, p(rows), 1, None, st) == -1  # row i of a 1-row buffer for i = 1
    assert L.jaco_load_envs(h, p(idx), n + 1, p(rows), n, p(idx), st) == -1
    assert sim.launch_count() == 0
    # out of range on the device: skipped, the neighbours served
    before = _everything(env)
    sim.load_envs(rows, envs=[-1, n, 7, 8], row_index=[0, 0, n, 2])
    after = _everything(env)
    for k in before:
        want = before[k].clone(); want[8] = before[k][2]
        assert torch.equal(_bits(after[k]), _bits(want)), k
    # foreign rows
    other = _make(False, num_envs=8, task="reaching")
    foreign = other.save_envs()
    other.close()
    assert foreign.rows.shape[1] == rows.shape[1] and int(foreign.rows[0, 0]) != int(rows[0, 0])
    sim.clear_flags()
    before = _everything(env)
    obs_before = env._obs.clone()
    env.load_envs(foreign, envs=[3, 200], row_index=[0, 5])
    after = _everything(env)
    fl = after.pop("flags"); before.pop("flags")
    for k in before:
        assert torch.equal(_bits(after[k]), _bits(before[k])), k
    assert torch.equal(env._obs, obs_before)
    bad = (fl & _lib.JACO_FLAG_BAD_SNAPSHOT) != 0
    assert bad.nonzero().flatten().tolist() == [3, 200]
    env.close()


def test_snapshot_object_round_trips_through_the_host(tmp_path):
    """EnvSnapshot: indexing, .to("cpu"), torch.save of its tensors; num_envs = 1 returns the reference's unbatched observation."""
    env = _make(False, num_envs=64)
    for a in _actions(2, 64, 2):
        env.step(a)
    snap = env.save_envs()
    torch.save(snap.to("cpu").tensors(), tmp_path / "snap.pt")
    back = EnvSnapshot.from_tensors(torch.load(tmp_path / "snap.pt"))
    assert torch.equal(back.rows, snap.rows.cpu()) and torch.equal(back.obs, snap.obs.cpu()) and back.current_steps == env.current_steps == 2
    one = back[5]
    assert len(one) == 1 and torch.equal(one.rows[0], back.rows[5])
    env.step(_actions(1, 64, 3)[0])
    env.load_envs(back[[5, 6]], envs=[0, 1])
    q = _bits(env.sim.get_state()[0]); s = _bits(snap.rows)
    off = _table(env)[1]["qpos"][1]
    assert torch.equal(q[:2], s[5:7, off:off + env.sim.nq]) and env.current_steps == 2
    env.close()
    e1 = JacoBatchedEnv(num_envs=1, task="picking", seed=3)
    o0 = e1.reset()
    s1 = e1.save_envs()
    e1.step(np.zeros(7, np.float32))
    o1 = e1.load_envs(s1)
    assert isinstance(o1, np.ndarray) and o1.shape == (26,) and np.array_equal(o1, o0)
    e1.close()
