"""CPU tier: env snapshots (jaco_save_envs / jaco_load_envs) -- the row table and the save / load routines of csrc/snapshot.h in their
host build (tests/snapshot_binding.py), alone and around the emulated step kernels: a restored env continues bit for bit."""
import os
import re

import numpy as np
import pytest

import snapshot_binding as sb
from emu_binding import EmuJacoEnv
from mujoco_jaco_amd.modelc import blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"": ("jaco2_curtain_torque", "jaco2_reaching_torque"), "_d12": ("jaco2_torque", "jaco2_curtain_torque_sensor"), "_d30": ("jaco2_dual_torque",)}


def _dims(model):
    M = blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", model + ".jacomdl"))
    return int(M["nq"][0]), int(M["nv"][0]), int(M["nsensor"][0])


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype.itemsize == 4 else np.ascontiguousarray(a).astype(np.uint32)


def test_table_is_dense_aligned_and_covers_the_env_call_state():
    """W is a multiple of 4 and the sum of the table (+ header, + padding < 4); fields follow one another without gap or overlap; the table
    names every per-env state array the emulated env-level call takes (emu_env_call's mutable pointers, outputs aside)."""
    sig = re.search(r"int emu_env_call\((.*?)\)\s*\{", open(os.path.join(ROOT, "tests", "emu", "emu_driver.cpp")).read(), re.S).group(1)
    state = [name for const, name in re.findall(r"(const )?(?:float|unsigned|int|unsigned char)\* (\w+)", sig) if not const]
    state = [s for s in state if s not in ("obs", "reward", "done", "heavy_envs")]   # what the call returns, not what it carries
    assert state == ["qpos", "qvel", "qacc_ws", "sensordata", "flags", "stats", "task", "cache", "marker"], state
    for layout, models in MODELS.items():
        L = sb.lib(layout)
        names = sb.fields(layout)
        assert set(state) <= set(names), set(state) - set(names)
        for model in models:
            nq, nv, ns = _dims(model)
            W, tab, fp = sb.table(nq, nv, ns, 0, layout)
            end = L.snap_header_words()
            for f in names:            # table order = row order
                words, off = tab[f]
                assert off == end and words >= 0, (f, off, end)
                end += words
            assert W % 4 == 0 and 0 <= W - end < 4 and W == (L.snap_header_words() + sum(w for w, _ in tab.values()) + 3) // 4 * 4
            assert tab["qpos"][0] == tab["qpos_lo"][0] == nq and tab["qvel"][0] == tab["qvel_lo"][0] == tab["qacc_ws"][0] == nv
            assert tab["sensordata"][0] == ns and tab["task"][0] == L.snap_task_floats() and tab["cache"][0] == L.snap_cache_floats()
            assert fp != 0 and fp != sb.table(nq, nv, ns, 1, layout)[2] and fp != sb.table(nq + 1, nv, ns, 0, layout)[2]
            print("%s (%s build): W = %d words = %d bytes per env" % (model, layout or "default", W, 4 * W))


def _start(nenv=4, fs=10, seed=5):
    e = EmuJacoEnv(nenv=nenv, frame_skip=fs, seed=seed)
    for k in range(nenv):
        e.reset_env(k)
    e.forward()
    return e


def _actions(nenv, n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, nenv, 7)).astype(np.float32)


def _trace(e, actions):
    """Every state array and every output after each step, as uint32 words."""
    out = []
    for a in actions:
        obs, rew, done = e.env_step(a)     # (no injected noise: the sub-goal noise comes from the counter-based RNG, i.e. from the task row)
        out.append([_u32(x).copy() for x in (e.qpos, e.qvel, e.qacc_ws, e.sensordata, e.flags, e.stats, e.task, e.cache, e.marker, obs, rew, done)])
    return out


def _equal(ta, tb):
    return all(np.array_equal(x, y) for sa, sb_ in zip(ta, tb) for x, y in zip(sa, sb_))


K, M_STEPS = 3, 3


def _run_a():
    e = _start()
    acts = _actions(e.nenv, K + M_STEPS, 9)
    _trace(e, acts[:K])
    rows = sb.emu_host(e).save()
    return rows, acts, _trace(e, acts[K:])


def test_restored_env_continues_bit_for_bit_through_the_emulator():
    """Run A: k steps, save, m steps.  Run B: a freshly constructed env loaded from the rows, the same m steps.  Equal word for word: the row
    holds every word the step reads, so the bound is exact equality."""
    rows, acts, ta = _run_a()
    assert ta[0][6].reshape(4, -1)[:, 18].min() > 0 and np.any(ta[-1][5].reshape(4, 4)[:, 0] > 0)   # draws were consumed, contacts present
    b = EmuJacoEnv(nenv=4, frame_skip=10, seed=5)
    b.forward()                                     # (sizes the emulator's own latches; state comes from the rows)
    hb = sb.emu_host(b)
    hb.load(rows)
    assert np.array_equal(hb.save(), rows)          # what was loaded is what a save gives back
    tb = _trace(b, acts[K:])
    assert _equal(ta, tb)


def test_a_field_left_out_of_the_load_is_noticed():
    """The same with one field at a time withheld from the load: run B must differ for the controller cache and the task row; the others
    are reported (a field whose omission changes nothing ON THIS WORKLOAD is printed, not asserted)."""
    rows, acts, ta = _run_a()
    differs = {}
    for f in ("cache", "task", "sensordata", "qacc_ws", "marker", "stats", "flags"):
        b = EmuJacoEnv(nenv=4, frame_skip=10, seed=5)
        b.forward()
        sb.emu_host(b).load(rows, leave_out=(f,))
        differs[f] = not _equal(ta, _trace(b, acts[K:]))
    print("run B differs from run A when the load leaves out:", {f: d for f, d in differs.items()})
    assert differs["cache"] and differs["task"], differs


def _synthetic(nenv, layout="", model="jaco2_curtain_torque", task_id=0, seed=1, guard=1):
    """Random words in every field's array, `guard` extra env rows in front of and behind each (the arrays handed out are the middle)."""
    nq, nv, ns = _dims(model)
    _, tab, _ = sb.table(nq, nv, ns, task_id, layout)
    rng = np.random.default_rng(seed)
    full = {f: rng.integers(1, 2 ** 32, (nenv + 2 * guard, w), dtype=np.uint32) for f, (w, _) in tab.items()}
    return sb.SnapHost({f: a[guard:guard + nenv] for f, a in full.items()}, nq, nv, ns, task_id, nenv, layout), full


def _state(h):
    return {f: a.copy() for f, a in h.arrays.items()}


@pytest.mark.parametrize("layout,model", [("", "jaco2_curtain_torque"), ("", "jaco2_reaching_torque"), ("_d12", "jaco2_torque"), ("_d30", "jaco2_dual_torque")])
def test_index_semantics(layout, model):
    """Permutation, fan-out, partial index lists; out-of-range env / row indices are no-ops and nothing outside the buffers is written;
    a row with a foreign fingerprint leaves the env untouched and sets the flag bit in it."""
    n = 6
    h, full = _synthetic(n, layout, model)
    full0 = {f: a.copy() for f, a in full.items()}
    s0 = _state(h)
    W = h.W
    buf = np.full((n + 2, W), 0xDEADBEEF, np.uint32)
    rows = buf[1:n + 1]
    h.save(rows=rows)
    assert np.all(buf[0] == 0xDEADBEEF) and np.all(buf[-1] == 0xDEADBEEF)
    assert np.all(rows[:, 0] == h.fingerprint) and np.all(rows[:, 1:4] == 0)
    for f, (w, off) in h.tab.items():                       # every field sits where the table says
        assert np.array_equal(rows[:, off:off + w], s0[f].reshape(n, w)), f
    end = max(off + w for w, off in h.tab.values())
    assert np.all(rows[:, end:] == 0)
    # partial save with an index list
    part = h.save(envs=[4, 1])
    assert np.array_equal(part, rows[[4, 1]])
    # permutation: env i := row perm[i]
    perm = np.array([3, 0, 5, 1, 2, 4])
    h.load(rows, row_index=perm)
    for f in s0:
        assert np.array_equal(h.arrays[f], s0[f][perm]), f
    # fan-out of one row to all envs
    h.load(rows, row_index=np.full(n, 2))
    for f in s0:
        assert np.all(h.arrays[f] == s0[f][2]), f
    # partial load: envs 5 and 0 from rows 1 and 4; the others keep what they hold
    h.load(rows)
    h.load(rows, envs=[5, 0], row_index=[1, 4])
    for f in s0:
        want = s0[f].copy(); want[5] = s0[f][1]; want[0] = s0[f][4]
        assert np.array_equal(h.arrays[f], want), f
    # out of range: env index and row index, both signs -- no-ops; the valid entry next to them is served
    h.load(rows)
    before = _state(h)
    h.load(rows, envs=[-1, n, 2, 3, 1], row_index=[0, 0, -1, n, 5])
    for f in s0:
        want = before[f].copy(); want[1] = s0[f][5]
        assert np.array_equal(h.arrays[f], want), f
    out = np.full((3, W), 0xDEADBEEF, np.uint32)
    h.save(envs=[n, 1, -3], rows=out)
    assert np.all(out[0] == 0xDEADBEEF) and np.all(out[2] == 0xDEADBEEF) and out[1, 0] == h.fingerprint
    g = 1
    for f, a in full.items():                                # the guard rows around every array
        assert np.array_equal(a[:g], full0[f][:g]) and np.array_equal(a[-g:], full0[f][-g:]), f
    assert np.all(buf[0] == 0xDEADBEEF) and np.all(buf[-1] == 0xDEADBEEF)
    # foreign fingerprint (another task's row): env untouched, flag bit set in exactly the addressed envs
    h.load(rows)
    before = _state(h)
    foreign = rows.copy(); foreign[:, 0] = sb.table(*h.dims[:3], h.dims[3] + 1, layout)[2]
    h.load(foreign, envs=[2, 4], row_index=[0, 0])
    bad = h.L.snap_bad_flag()
    for f in s0:
        want = before[f].copy()
        if f == "flags":
            want[[2, 4]] |= bad
        assert np.array_equal(h.arrays[f], want), f
    assert bad == 0x40000


def test_absent_fields_are_saved_as_zeros_and_skipped_by_a_load():
    """A build without some array (the emulator keeps no compensation words, hints, costs, terminal observation) keeps the row layout."""
    h, _ = _synthetic(3)
    lean = sb.SnapHost({f: a for f, a in h.arrays.items() if f not in ("qpos_lo", "hint", "terminal_obs")}, *h.dims, 3)
    rows = lean.save()
    assert lean.W == h.W
    for f in ("qpos_lo", "hint", "terminal_obs"):
        w, off = h.tab[f]
        assert np.all(rows[:, off:off + w] == 0)
    s0 = _state(h)
    h.load(rows, leave_out=("cache",))
    assert np.array_equal(h.arrays["cache"], s0["cache"]) and np.all(h.arrays["qpos_lo"] == 0)
