"""CPU tier: stage T (csrc/collision.h stage_touch / ray_hits_site) of the *unmodified* kernel source under the wavefront emulator, held to an
fp64 restatement of the stage fed the kernel's own contact record (tests/touch_binding.py), on every sensor model and the three layouts.
One substep from a set state (zero velocity and warm start): the record and the readings belong to a forward pass whose body poses the
oracle gives.  The states (tests/golden/touch_states.npz, make_touch_states.py) are chosen on the oracle by what they exercise; the census
of what the stage really saw is asserted, so that a change of states cannot quietly lose a branch.

Measured, emulator (worst |kernel - recomputation| / bound, the bound being (10 + n_k) 2^-23 sum fn; knife readings / non-zero readings;
pipeline figure |kernel - oracle sensordata| / largest reading, printed only):
  default  43 states   0.054   3 / 210   8.3e-7
  old       4 states   0.038   0 / 19    1.1e-5
  sensor   19 states   0.000   0 / 8     1.8e-4 (the 14 golden poses alone: 5.5e-4; every reading there is one contact's force, read back exactly)
  dual     20 states   0.050   0 / 140   2.7e-6
Each of these breaks, applied alone to collision.h, fails test_stage_against_its_own_record: the ray sign for a second body ([default],
[sensor], [dual]); the cylinder site's half height taken from its radius ([default], [dual]); c_fn filled for the first 64 contacts only
([default]); the sphere branch's far root tested <= 0 ([sensor]); word 2 of the body mask read as word 1 ([dual])."""
import numpy as np
import pytest

import touch_binding as tb
from emu_binding import EmuEnv


def _run(name, q, ctrl, cap=128):
    e = EmuEnv(name, nenv=len(q), layout=tb.LAYOUT[name])
    e.qpos[:] = q; e.qvel[:] = 0; e.qacc_ws[:] = 0
    e.sensordata[:] = 7.0   # (every reading is written, zeros included)
    rec, n = e.step_rec(ctrl, nsub=1, cap=cap)
    return rec, n, e.sensordata.copy(), e.flags.copy(), e.stats.copy()


@pytest.mark.parametrize("key", list(tb.SETS))
def test_restatement_is_the_oracles_touch(key):
    """touch_reference() on the oracle's own contacts and forces is the oracle's sensordata (1e-11; measured 7.3e-12 on readings of up to
    1.5e4 N, 5e-13 and below on the other sets), and the chosen states hold what they were chosen for -- knife readings included, which
    only the oracle's contacts decide."""
    name, M, q, ctrl, S, refs = tb.states(key)
    print("%s: restatement against the oracle's sensordata %.2e" % (key, tb.check_restatement(M, S, refs)))
    tb.check_census(key, M, S, refs, knife=True)
    nonzero = sum(int((r["sens"] > 0).sum()) for r in refs)
    assert sum(int(r["knife"].sum()) for r in refs) <= tb.KNIFE_SHARE * nonzero


@pytest.mark.parametrize("key", list(tb.SETS))
def test_stage_against_its_own_record(key):
    """Every reading that is not knife within (10 + n_k) 2^-23 sum(fn) of the fp64 recomputation from the record, exactly 0 where nothing
    counts (envs without a sensor-body contact: the early-out; envs whose sensor-body contacts carry no force or miss every site: the ballot
    passes and the sums stay 0); nothing overflowed; knife readings below 2 % of the non-zero ones; the census, on the record.
    default: light, light with side rows, medium, heavy and huge tier, contacts past the 64th on sensor bodies, the cylinder site.
    old / sensor: the _d12 build (cylinder site; sphere site from inside and from outside; 61 sensors).  dual: the _d30 build, sensor
    bodies above id 64 (word 2 of the body mask)."""
    tb.check_set(key, _run, "emulator")


def test_arm_only_model_reads_zero():
    """jaco2_reaching_torque under disable_contact (the contact-free kernel: no touch stage at all): every reading is written as 0."""
    e = EmuEnv("jaco2_reaching_torque", nenv=3)
    e.sensordata[:] = 7.0
    e.step(np.full(9, 0.1), nsub=2, disable_contact=True)
    assert e.ns == 20 and (e.sensordata == 0).all()
