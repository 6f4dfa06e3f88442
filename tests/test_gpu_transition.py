"""GPU tier: jaco_transition_fd (mujoco_jaco_amd/csrc/transition.h) on the MI355X against jaco_rollout bit for bit, against the formula
recomputed from jaco_rollout, against the fp64 oracle, against robot_config.linearize and through one iLQR iteration on one handle
(tests/transition_binding.py holds the inputs, the cases and the references; tests/test_transition_emu.py is the CPU-tier twin, whose
docstring states the shapes, the references and the error measures).  The arm's full set runs on every model here.

The formula: transition_binding.case_formula's derived bound, also on a handle with compensated = 0, where its low-word term drops.
Against fp64, fd_binding.merr over A / B on the kept pairs (all nine on every model); bounds = 3 x the largest value measured on the MI355X:
  A / B, hold 3, small sets, four models ....... 1.18e-4 / 3.39e-5 -> 3.6e-4 / 1.1e-4
  A / B, hold 1, small sets, four models ....... 9.41e-5 / 1.39e-6 -> 2.9e-4 / 4.2e-6
  A / B, hold 3, full sets, four models ........ 1.18e-4 / 3.04e-5 -> 3.6e-4 / 9.2e-5
  position rows of A, pairs without a limit row: the increment form against the end states' high words, at most a quarter
    (measured: 2.9e-8 .. 3.2e-7 against 2.7e-6 .. 1.5e-5)
Against robot_config.linearize, hold 1, jaco2_reaching_torque, pairs with nefc == 0: A / B 1.24e-6 / 1.34e-6 -> 3.8e-6 / 4.1e-6.
One iLQR iteration (8 envs x 20 knots x hold 3): the nominal's cost 104.6 .. 112.8, the best step's 81.2 .. 82.1.
"""
import ctypes

import numpy as np
import pytest
import torch

import fd_binding as fb
import lqr_binding as lb
import rollout_binding as rb
import transition_binding as tb
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError

pytestmark = pytest.mark.gpu
FP64_BOUNDS = {3: (3.6e-4, 1.1e-4), 1: (2.9e-4, 4.2e-6)}
FP64_FULL_BOUNDS = (3.6e-4, 9.2e-5)
LINEARIZE_BOUNDS = (3.8e-6, 4.1e-6)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


_TORCH = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
GPU = rb.Tier(lambda a, dtype: _dev(a, _TORCH[dtype]), lambda shape, value, dtype: torch.full(shape, value, dtype=_TORCH[dtype], device="cuda:0"),
              lambda t: ctypes.c_void_p(t.data_ptr()), 1)


@pytest.fixture(scope="module")
def sims():
    """One BatchedMujoco per (model, num_envs, compensated), opened on first use and closed at the end of the module."""
    open_ = {}

    def get(model, n, compensated=True):
        key = (model, n, compensated)
        if key not in open_:
            open_[key] = BatchedMujoco(n, robot_file=model)
            if not compensated:
                open_[key].set_option("compensated", 0)
        return open_[key]
    yield get
    for s in open_.values():
        s.close()


def abi_call(sim, qpos, qvel, ctrl, dofs, acts, want=tb.OUTS, hold=1, centered=1, groups=0, n=None, no_opt=False, no_out=False, patch=None, **eps):
    """jaco_transition_fd straight through the C ABI on device tensors, the arguments of transition_binding.transition: (return code,
    {output: device tensor handed in filled with the sentinels}); for n <= 0 the outputs have one pair's rows, so that no pointer is NULL."""
    p = GPU.ptr
    q, v, c = GPU.f32(qpos), GPU.f32(qvel), GPU.f32(ctrl)
    rows = next((a.shape[0] for a in (q, v, c) if a is not None), sim.num_envs)   # (the outputs' rows: what the arrays say, whatever n a refusal case hands)
    n = rows if n is None else n
    sh = tb.shapes(max(rows, GPU.min_rows), sim.nq, sim.nv, max(len(dofs), 1), max(len(acts), 1))   # (an empty list: one column, so that no pointer is NULL)
    outs = {k: GPU.blank(sh[k], k == "status") for k in want}
    rec = _lib.JacoTransitionOut(*[p(outs.get(k)) for k in tb.OUTS])
    opt = tb.options(dofs, acts, patch, hold=hold, centered=centered, groups=groups, **eps)
    rc = sim.L.jaco_transition_fd(sim.h, rb.ref(opt, no_opt), n, p(q), p(v), p(c), rb.ref(rec, no_out), sim._stream())
    return rc, outs


def _host(outs):
    return {k: (t.cpu().numpy().view(np.uint32) if k == "status" else t.cpu().numpy()) for k, t in outs.items()}


def runner(sims, compensated=True):
    def call(model, q, v, c, dofs, acts, handle=None, **k):
        if handle is None:
            sim = sims(model, 2, compensated)   # (n is not tied to num_envs: any handle of the model serves)
        else:
            sim = sims(model, len(handle[0]), compensated)
            sim.set_state(_dev(handle[0]), _dev(handle[1]), None)
        rc, outs = abi_call(sim, q, v, c, dofs, acts, **k)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return _host(outs)
    return call


def roller(sims, compensated=True):
    def call(model, q, v, c, hold):
        r = sims(model, 2, compensated).rollout(_dev(c)[:, None], _dev(q), _dev(v), hold=hold, final_only=True)
        return {"qpos": r["qpos"][:, 0].cpu().numpy(), "qvel": r["qvel"][:, 0].cpu().numpy(), "status": r["status"].cpu().numpy().view(np.uint32)}
    return call


@pytest.fixture(scope="module")
def run(sims):
    return runner(sims)


@pytest.fixture(scope="module")
def roll(sims):
    return roller(sims)


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_the_nominal_is_jaco_rollout_bit_for_bit(run, roll, model, hold):
    tb.case_nominal(run, roll, model, hold)


@pytest.mark.parametrize("model", tb.MODELS)
def test_groups_outputs_and_batch_do_not_change_a_bit(run, model):
    tb.case_invariance(run, model)


@pytest.mark.parametrize("model", tb.EVERY_MODELS)
def test_every_hinge_dof_and_every_ctrl_word(run, roll, model):
    """nx = 18 with 9 ctrl words, and the two-arm model's 36 lanes x 54 columns (where the kept low word waits in the flags word): groups,
    output subsets, a pair alone, a repeat bit for bit, forward differences against groups too, and the formula recomputed from jaco_rollout."""
    tb.case_invariance(run, model, sets=tb.every_set)
    q, v, c = tb.inputs(model)
    dofs, acts = tb.every_set(model)
    f1 = run(model, q[:3], v[:3], c[:3], dofs, acts, want=("A", "B"), hold=1, centered=0, groups=1)
    tb.same(f1, run(model, q[:3], v[:3], c[:3], dofs, acts, want=("A", "B"), hold=1, centered=0, groups=7))
    tb.case_formula(run, roll, "gpu", model, dofs, acts, 3)


def test_forward_differences_do_not_depend_on_groups_either(run):
    full = tb.case_invariance(run, rb.MODEL, hold=1, centered=0)
    q, v, c = tb.inputs(rb.MODEL)
    dofs, acts = tb.small_set(rb.MODEL)
    central = run(rb.MODEL, q, v, c, dofs, acts, hold=1)
    tb.same(full, central, ("next_qpos", "next_qvel", "status"))
    assert (tb.bits(full["A"]) != tb.bits(central["A"])).any()
    inside = [1, 4, 7]   # (no limit row: one-sided and central differences agree to the truncation error)
    assert tb.merr(full["A"][inside], central["A"][inside]) < 1e-3


@pytest.mark.parametrize("model", tb.MODELS)
def test_the_small_set_sits_inside_the_full_set(run, model):
    tb.case_subset_of_full(run, model)


def test_a_clamped_ctrl_word_has_a_zero_column(run):
    tb.case_clamped_ctrl(run)


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_the_formula_recomputed_from_jaco_rollout(run, roll, model, hold):
    tb.case_formula(run, roll, "gpu", model, *tb.small_set(model), hold)


def test_the_formula_without_the_low_words(sims):
    """Option "compensated" = 0 on the handle: jaco_rollout and the kernel both run without low words, and the low-word term of the
    bound drops: what is left is the reciprocal, the difference and the product."""
    tb.case_formula(runner(sims, False), roller(sims, False), "gpu-uncompensated", rb.MODEL, *tb.small_set(rb.MODEL), 3, compensated=False)


@pytest.mark.parametrize("hold", tb.HOLDS)
@pytest.mark.parametrize("model", tb.MODELS)
def test_against_fp64_central_differences(run, roll, model, hold):
    ea, eb, mine, theirs = tb.case_fp64(run, roll, "gpu", model, *tb.small_set(model), hold)
    assert ea <= FP64_BOUNDS[hold][0] and eb <= FP64_BOUNDS[hold][1], (ea, eb)
    assert mine <= theirs / 4, (mine, theirs)


@pytest.mark.parametrize("model", tb.MODELS)
def test_the_full_set_against_fp64(run, roll, model):
    dofs, acts = tb.full_set(model)
    tb.case_formula(run, roll, "gpu", model, dofs, acts, 3)
    ea, eb, mine, theirs = tb.case_fp64(run, roll, "gpu", model, dofs, acts, 3)
    assert ea <= FP64_FULL_BOUNDS[0] and eb <= FP64_FULL_BOUNDS[1], (ea, eb)
    assert mine <= theirs / 4, (mine, theirs)


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


def test_against_robot_config_linearize(make_sim):
    ea, eb = tb.case_linearize(make_sim)
    print("MEASURE linearize: transition_fd against robot_config.linearize: A %.3g B %.3g" % (ea, eb))
    assert ea <= LINEARIZE_BOUNDS[0] and eb <= LINEARIZE_BOUNDS[1], (ea, eb)


def test_the_handles_state_is_read_and_nothing_is_written(sims):
    """NULL qpos / qvel = get_state()'s rows bit for bit; one launch; state, flags and sensordata bitwise unchanged."""
    q, v, c = tb.inputs(rb.MODEL)
    dofs, acts = tb.small_set(rb.MODEL)
    sim = sims(rb.MODEL, tb.N)
    sim.set_state(_dev(q), _dev(v), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (tb.N, 9))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    ctrl = _dev(c)
    sim.launch_count()   # (reading the counter resets it)
    a = sim.transition_fd(ctrl, dofs=dofs, acts=acts, hold=3, want=tb.OUTS)
    assert sim.launch_count() == 1
    b = sim.transition_fd(ctrl, qh, vh, dofs=dofs, acts=acts, hold=3, want=tb.OUTS)
    for k in tb.OUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    lead = sim.transition_fd(ctrl[:8].reshape(2, 4, -1), qh[:8].reshape(2, 4, -1), vh[:8].reshape(2, 4, -1), dofs=dofs, acts=acts, hold=3)
    assert lead["A"].shape == (2, 4, 6, 6) and lead["B"].shape == (2, 4, 6, 2) and torch.equal(lead["A"].reshape(8, 6, 6), a["A"][:8])
    assert sim.transition_fd(ctrl[:0], qh[:0], vh[:0], dofs=dofs, acts=acts)["A"].shape == (0, 6, 6)


ILQR_T, ILQR_HOLD = 20, 3


def test_one_ilqr_iteration_on_one_handle(make_sim):
    """linearize_rollout -> ilqr_backward(full=True) -> rollout_feedback at eight step sizes on jaco2_reaching_torque, 8 envs x 20 knots x
    hold 3, the cost of lqr_binding.case_ilqr, around gravity compensation: no status flag, dV1 < 0, and for every env the best true cost
    of the nonlinear rollouts below the nominal's.  Four launches, no second handle."""
    from mujoco_jaco_amd.robot_config import BatchedMujocoConfig
    import osc_binding as ob
    model, B, T = lb.ARM_MODEL, lb.ILQR_B, ILQR_T
    q, _ = ob.states(model, B)
    sim = make_sim(model, q.astype(np.float32), np.zeros((B, int(tb.ib.load_model(model)["nv"][0])), np.float32))
    cfg = BatchedMujocoConfig(sim, ee="EE")
    dofs, qadr, acts = cfg._joint_subset(None, "test")
    n, m, dev = len(dofs), len(acts), sim.device
    ubar = cfg.joint(joints=None).gravity_compensation()                     # [B, nu]
    u = ubar[:, None, acts].expand(-1, T, -1).contiguous()                    # [B, T, m]
    qpos0, _, _ = sim.get_state()
    goal = qpos0[:, qadr] + lb.GOAL_OFF

    def cost(X, U, g):
        """[..] true cost of states X [.., T + 1, 2 n] under the motor words U [.., T, m], in fp64 (lqr_binding.case_ilqr's)."""
        X, U, g = X.double(), U.double(), g.double()
        e = X[..., :n] - g[..., None, :]
        run_ = 0.5 * lb.WQ * (e[..., :-1, :] ** 2).sum(-1) + 0.5 * lb.WV * (X[..., :-1, n:] ** 2).sum(-1) + 0.5 * lb.WU * (U ** 2).sum(-1)
        return run_.sum(-1) + 0.5 * lb.WF * (e[..., -1, :] ** 2).sum(-1) + 0.5 * lb.WV * (X[..., -1, n:] ** 2).sum(-1)
    sim.launch_count()
    A, Bm, X, ua, status = cfg.linearize_rollout(u, ctrl=ubar, hold=ILQR_HOLD)
    assert A.shape == (B, T, 2 * n, 2 * n) and Bm.shape == (B, T, 2 * n, m) and X.shape == (B, T + 1, 2 * n) and ua.shape == (B, T, m)
    w = torch.tensor([lb.WQ] * n + [lb.WV] * n, device=dev)
    wf = torch.tensor([lb.WF] * n + [lb.WV] * n, device=dev)
    D = X.clone()
    D[..., :n] -= goal[:, None]
    K, k, dV, st = cfg.ilqr_backward(A, Bm, torch.diag(w), lb.WU * torch.eye(m, device=dev), lx=w * D[:, :-1], lu=lb.WU * ua, Vxx=torch.diag(wf),
                                     Vx=wf * D[:, -1], mu=1e-3 * lb.WU)
    alphas = torch.tensor([2.0 ** -i for i in range(8)], device=dev)
    r = cfg.rollout_feedback(ua, K=K, x_ref=X[:, :-1].contiguous(), k=k, alphas=alphas, ctrl=ubar, hold=ILQR_HOLD)
    assert sim.launch_count() == 4
    assert not status.cpu().numpy().any() and not st.cpu().numpy().any() and not r["status"].cpu().numpy().any()
    assert torch.equal(ua, u)                                                # (no gain, no step: the applied words are the plan's)
    J0 = cost(X, ua, goal).cpu().numpy()
    Xa = torch.cat([torch.cat([X[:, None, :1, :n].expand(-1, 8, -1, -1), r["q"]], 2), torch.cat([X[:, None, :1, n:].expand(-1, 8, -1, -1), r["dq"]], 2)], -1)
    J = cost(Xa, r["u"], goal[:, None]).cpu().numpy()
    dV = dV.cpu().numpy()
    print("MEASURE ilqr: nominal cost %s, best cost %s, dV1 %s" % (np.round(J0, 3), np.round(J.min(1), 3), np.round(dV[:, 0], 3)))
    assert (dV[:, 0] < 0).all() and (J.min(1) < J0).all(), (dV, J0, J)


@pytest.mark.parametrize("case", sorted(tb.REFUSALS))
def test_refusals_leave_the_outputs_untouched(case, sims):
    a = tb.refusal_args(case)
    handle = a.pop("handle", None)
    sim = sims(tb.REFUSAL_MODEL, tb.REFUSAL_ENVS if handle is not None else 2)
    rc, outs = abi_call(sim, a.pop("qpos"), a.pop("qvel"), a.pop("ctrl"), a.pop("dofs"), a.pop("acts"), **a)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_transition_fd: " + tb.REFUSALS[case]   # (the emulator's text: test_transition_emu.py)
    for k, t in outs.items():
        assert (t == (rb.STATUS_SENTINEL if k == "status" else rb.SENTINEL)).all(), k


def test_the_python_layer_passes_refusals_on(sims):
    sim = sims(rb.MODEL, 2)
    with pytest.raises(JacoError, match="jaco_transition_fd: dof 9 belongs to a free joint"):
        sim.transition_fd(None, dofs=[9], acts=[0])
