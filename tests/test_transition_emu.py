"""CPU tier: the transition-Jacobian kernel (mujoco_jaco_amd/csrc/transition.h, jaco_transition_fd) under the wavefront emulator, against
jaco_rollout bit for bit, against the formula recomputed from jaco_rollout, against the fp64 oracle and against robot_config.linearize
(tests/transition_binding.py holds the emulated call, the inputs, the cases and the references; tests/test_gpu_transition.py is the
GPU-tier twin).  Nine pairs per model from rollout_binding.inputs: three with a limit row from the start, three at least 0.15 rad
inside every limit, three as drawn.  The small sets (dofs 0, 3, 5 and two motor words) everywhere, the arm's full set on the default model.
Every hinge dof with every ctrl word (18 + 9 columns; 36 + 18 on the two-arm model, all 36 lanes) runs the bit-for-bit cases and the
formula, which need no fp64 reference; largest formula ratio there 0.99 / 0.986.

Bit for bit: the nominal against jaco_rollout(nknots = 1, hold, final_only) on all four models; groups 1 / 2 / ncol / the library's
choice; each output alone; a pair alone; two identical calls; the small set inside the full set; a clamped ctrl word's B column 0.0f.
The formula: |kernel - fp64 columns from jaco_rollout's high words at the explicitly perturbed fp32 rows| <= (ulp32(x'(+)) + ulp32(x'(-)))
/ 2 / |c(+) - c(-)| + 4 * 2^-23 |entry| per entry (derived in transition_binding.case_formula; not measured; the largest ratio on the emulator is 0.997: the low words do reach half a spacing).
Against fp64 (central differences of the oracle's contact-free rollout, the kernel's eps, the same rounded inputs, the increment form),
fd_binding.merr over A and over B on the kept pairs (all nine on every model); bounds = 3 x the largest value measured on the emulator:
  A / B, hold 3, small sets, four models ....... 6.70e-5 / 2.03e-5 -> 2.0e-4 / 6.1e-5
  A / B, hold 1, small sets, four models ....... 6.09e-5 / 1.24e-6 -> 1.8e-4 / 3.7e-6
  A / B, hold 3, full set, default model ....... 6.19e-5 / 2.00e-5 -> 1.9e-4 / 6.0e-5
  position rows of A, pairs without a limit row: the increment form against the end states' high words, at most a quarter
    (measured: 3.2e-8 .. 2.0e-7 against 2.7e-6 .. 1.5e-5)
Against robot_config.linearize (jaco_fd + the torch assembly), hold 1, jaco2_reaching_torque, fd_binding.stepper_inputs(), pairs with
nefc == 0: A / B 4.88e-7 / 1.36e-6 -> 1.5e-6 / 4.1e-6.
"""
import numpy as np
import pytest

import fd_binding as fb
import rollout_binding as rb
import transition_binding as tb

FP64_BOUNDS = {3: (2.0e-4, 6.1e-5), 1: (1.8e-4, 3.7e-6)}
FP64_FULL_BOUNDS = (1.9e-4, 6.0e-5)
LINEARIZE_BOUNDS = (1.5e-6, 4.1e-6)


def run(model, q, v, c, dofs, acts, **k):
    return tb.transition(model, q, v, c, dofs, acts, **k)


roll = tb.emu_roll


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_the_nominal_is_jaco_rollout_bit_for_bit(model, hold):
    tb.case_nominal(run, roll, model, hold)


@pytest.mark.parametrize("model", tb.MODELS)
def test_groups_outputs_and_batch_do_not_change_a_bit(model):
    tb.case_invariance(run, model)


@pytest.mark.parametrize("model", tb.EVERY_MODELS)
def test_every_hinge_dof_and_every_ctrl_word(model):
    """nx = 18 with 9 ctrl words, and the two-arm model's 36 lanes x 54 columns (where the kept low word waits in the flags word): groups,
    output subsets, a pair alone, a repeat bit for bit, forward differences against groups too, and the formula recomputed from jaco_rollout."""
    tb.case_invariance(run, model, sets=tb.every_set)
    q, v, c = tb.inputs(model)
    dofs, acts = tb.every_set(model)
    f1 = run(model, q[:3], v[:3], c[:3], dofs, acts, want=("A", "B"), hold=1, centered=0, groups=1)
    tb.same(f1, run(model, q[:3], v[:3], c[:3], dofs, acts, want=("A", "B"), hold=1, centered=0, groups=7))
    tb.case_formula(run, roll, "emu", model, dofs, acts, 3)


def test_forward_differences_do_not_depend_on_groups_either():
    full = tb.case_invariance(run, rb.MODEL, hold=1, centered=0)
    q, v, c = tb.inputs(rb.MODEL)
    dofs, acts = tb.small_set(rb.MODEL)
    central = run(rb.MODEL, q, v, c, dofs, acts, hold=1)
    tb.same(full, central, ("next_qpos", "next_qvel", "status"))
    assert (tb.bits(full["A"]) != tb.bits(central["A"])).any()
    inside = [1, 4, 7]   # (no limit row: one-sided and central differences agree to the truncation error)
    assert tb.merr(full["A"][inside], central["A"][inside]) < 1e-3


def test_the_small_set_sits_inside_the_full_set():
    tb.case_subset_of_full(run, rb.MODEL)


def test_a_clamped_ctrl_word_has_a_zero_column():
    tb.case_clamped_ctrl(run)


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_the_formula_recomputed_from_jaco_rollout(model, hold):
    tb.case_formula(run, roll, "emu", model, *tb.small_set(model), hold)


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_against_fp64_central_differences(model, hold):
    ea, eb, mine, theirs = tb.case_fp64(run, roll, "emu", model, *tb.small_set(model), hold)
    assert ea <= FP64_BOUNDS[hold][0] and eb <= FP64_BOUNDS[hold][1], (ea, eb)
    assert mine <= theirs / 4, (mine, theirs)


def test_the_full_set_on_the_default_model():
    dofs, acts = tb.full_set(rb.MODEL)
    tb.case_formula(run, roll, "emu", rb.MODEL, dofs, acts, 3)
    ea, eb, mine, theirs = tb.case_fp64(run, roll, "emu", rb.MODEL, dofs, acts, 3)
    assert ea <= FP64_FULL_BOUNDS[0] and eb <= FP64_FULL_BOUNDS[1], (ea, eb)
    assert mine <= theirs / 4, (mine, theirs)


def test_against_robot_config_linearize():
    ea, eb = tb.case_linearize(lambda model, q, v: tb.EmuTransitionSim(model, q, v))
    print("MEASURE linearize: transition_fd against robot_config.linearize: A %.3g B %.3g" % (ea, eb))
    assert ea <= LINEARIZE_BOUNDS[0] and eb <= LINEARIZE_BOUNDS[1], (ea, eb)


def test_transition_fd_shapes_and_messages():
    import torch
    q, v, c = tb.inputs(rb.MODEL)
    dofs, acts = tb.small_set(rb.MODEL)
    sim = tb.EmuTransitionSim(rb.MODEL, q, v)
    r = sim.transition_fd(torch.tensor(c), dofs=dofs, acts=acts, hold=3, want=("A", "B", "next_qpos", "status"))   # the sim's state
    assert sim.launches["jaco_transition_fd"] == 1 and set(r) == {"A", "B", "next_qpos", "status"}
    direct = run(rb.MODEL, q, v, c, dofs, acts, hold=3)
    assert (tb.bits(r["A"].numpy()) == tb.bits(direct["A"])).all() and (tb.bits(r["next_qpos"].numpy()) == tb.bits(direct["next_qpos"])).all()
    lead = sim.transition_fd(torch.tensor(c[:8]).reshape(2, 4, -1), torch.tensor(q[:8]).reshape(2, 4, -1), torch.tensor(v[:8]).reshape(2, 4, -1), dofs=dofs,
                             acts=acts, hold=3, want=("A", "B", "next_qvel", "status"))
    assert lead["A"].shape == (2, 4, 6, 6) and lead["B"].shape == (2, 4, 6, 2) and lead["next_qvel"].shape == (2, 4, 21) and lead["status"].shape == (2, 4)
    assert (tb.bits(lead["A"].numpy().reshape(8, 6, 6)) == tb.bits(direct["A"][:8])).all()
    with pytest.raises(ValueError, match="leading shape"):
        sim.transition_fd(torch.tensor(c[:8]), torch.tensor(q[:7]), torch.tensor(v[:7]), dofs=dofs, acts=acts)
    with pytest.raises(ValueError, match="together or not at all"):
        sim.transition_fd(torch.tensor(c), torch.tensor(q), None, dofs=dofs, acts=acts)
    with pytest.raises(ValueError, match="names none or not only outputs"):
        sim.transition_fd(torch.tensor(c), dofs=dofs, acts=acts, want=("A", "C"))
    with pytest.raises(TypeError, match="unknown transition option"):
        sim._transition(None, None, None, 9, ("A",), dofs=dofs, acts=acts, eps=1.0)


@pytest.mark.parametrize("model,ee", ((rb.MODEL, "EE"), ("jaco2_dual_torque", "EE_1")))
def test_linearize_rollout_is_two_launches(model, ee):
    """robot_config.linearize_rollout (n_robots = 2 too): the documented shapes; pair (b, t) is the state at the start of knot t and
    that knot's applied ctrl row, bit for bit against the two entries called directly; one launch each."""
    import torch
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    q, v, c = tb.inputs(model)
    B, T, hold = 4, 2, 2
    sim = tb.EmuTransitionSim(model, q[:B], v[:B])
    cfg = BatchedMujocoConfig(sim, ee=ee)
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    n, m = len(dofs), len(acts)
    u = torch.tensor(np.stack([c[:B, acts], c[B:2 * B, acts]], 1))
    A, Bm, X, ua, status = cfg.linearize_rollout(u, ctrl=torch.tensor(c[:B]), hold=hold)
    assert sim.launches["jaco_rollout_fb"] == 1 and sim.launches["jaco_transition_fd"] == 1 and sum(sim.launches.values()) == 2
    assert A.shape == (B, T, 2 * n, 2 * n) and Bm.shape == (B, T, 2 * n, m) and X.shape == (B, T + 1, 2 * n) and ua.shape == (B, T, m) and status.shape == (B,)
    full = np.repeat(c[:B, None], T, 1)
    full[:, :, acts] = u.numpy()
    r = rb.rollout(model, full, q[:B], v[:B], want=("qpos", "qvel", "status"), hold=hold)
    Q, V = np.concatenate([q[:B, None], r["qpos"]], 1), np.concatenate([v[:B, None], r["qvel"]], 1)
    assert (tb.bits(X.numpy()) == tb.bits(tb.x_of(model, dofs, Q, V))).all() and (tb.bits(ua.numpy()) == tb.bits(u.numpy())).all()
    d = run(model, Q[:, :T].reshape(B * T, -1), V[:, :T].reshape(B * T, -1), full.reshape(B * T, -1), dofs, acts, want=("A", "B"), hold=hold)
    assert (tb.bits(A.numpy().reshape(B * T, 2 * n, 2 * n)) == tb.bits(d["A"])).all() and (tb.bits(Bm.numpy().reshape(B * T, 2 * n, m)) == tb.bits(d["B"])).all()


@pytest.mark.parametrize("case", sorted(tb.REFUSALS))
def test_refusals(case):
    with pytest.raises(ValueError) as e:
        tb.transition(tb.REFUSAL_MODEL, **tb.refusal_args(case))
    assert str(e.value) == "emu_transition_fd returned -1: jaco_transition_fd: " + tb.REFUSALS[case]
    for k, a in e.value.outputs.items():   # a refusal writes nothing
        assert (a == (rb.STATUS_SENTINEL if k == "status" else rb.SENTINEL)).all(), k


def test_no_pairs_launch_nothing():
    q, v, c = tb.inputs(rb.MODEL)
    r = run(rb.MODEL, q[:0], v[:0], c[:0], *tb.small_set(rb.MODEL))
    assert r["A"].shape == (0, 6, 6)
