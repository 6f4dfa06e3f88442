"""GPU tier: jaco_fd (mujoco_jaco_amd/csrc/fd.h) on the MI355X against the fp64 oracle, against the emulator, against the step kernel
and against itself (tests/fd_binding.py holds the inputs, the cases and the references; tests/test_fd_emu.py is the CPU-tier twin, whose
docstring states the references and the error measures).

Bounds = 3 x the largest value measured on the MI355X (B = 67 on the default model, 9 on the others):
  qacc / qfrc_smooth / qacc with implicit damping, four models ................. 2.73e-3 / 8.68e-4 / 2.73e-3 -> 8.2e-3 / 2.7e-3 / 8.2e-3
  actuator model (ctrl beyond ctrlrange, forcerange held): qacc / qfrc / dctrl ... 8.20e-4 / 3.96e-4 / 2.50e-5 -> 2.5e-3 / 1.2e-3 / 7.5e-5
  free bodies at rest: gravity and zero rotational acceleration ............... 7.87e-4 -> 2.4e-3
  dqacc_dqpos (default eps 2^-8), four models ................................. 8.11e-5 -> 2.5e-4   (the issue's cap: 1e-2)
  dqacc_dqvel (default eps 2^-3) .............................................. 2.47e-5 -> 7.5e-5
  dqacc_dctrl ................................................................. 5.36e-5 -> 1.7e-4
  dqacc_dqvel at eps 0.125 against eps 0.5 (qacc is quadratic in qvel) ........ 3.77e-6 -> 1.2e-5
  qvel + h qacc against one oracle substep, jaco2_reaching_torque, B = 32 ..... 2.31e-5 -> 7.0e-5
  ... against send_forces(ctrl, 1) on the device ............................... 8.76e-8 -> 2.7e-7
  robot_config.linearize: A x + B u + c 1e-3 away against the oracle's substep  4.35e-7 -> 1.4e-6
  two-arm model, EE_1: dq + h qacc against the oracle's contact-free substep .. 3.26e-7 -> 9.8e-7
  GPU against the emulator: qacc / qfrc_smooth (case 1, default model) ........ 1.25e-3 / 4.75e-4 -> 3.8e-3 / 1.5e-3
  GPU against the emulator: dqacc_dqpos / dqacc_dqvel / dqacc_dctrl (case 4) .. 3.67e-5 / 3.50e-5 / 3.49e-5 -> 1.2e-4 / 1.1e-4 / 1.1e-4
"""
import ctypes

import numpy as np
import pytest
import torch

import fd_binding as fb
from mujoco_jaco_amd import _lib
from mujoco_jaco_amd.physics import BatchedMujoco, JacoError

pytestmark = pytest.mark.gpu
QACC_BOUND, QFRC_BOUND, QACC_DAMPED_BOUND = 8.2e-3, 2.7e-3, 8.2e-3
ACT_BOUNDS = (2.5e-3, 1.2e-3, 7.5e-5)
FREE_BOUND = 2.4e-3
DQPOS_BOUND, DQVEL_BOUND, DCTRL_BOUND, QUADRATIC_BOUND = 2.5e-4, 7.5e-5, 1.7e-4, 1.2e-5
DQPOS_CAP = 1e-2      # set by the issue
STEP_BOUND, STEP_DEVICE_BOUND = 7.0e-5, 2.7e-7
CONFIG_BOUND, TWO_ARM_BOUND = 1.4e-6, 9.8e-7
EMU_VALUE_BOUNDS = (3.8e-3, 1.5e-3)
EMU_LIN_BOUNDS = (1.2e-4, 1.1e-4, 1.1e-4)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


@pytest.fixture(scope="module")
def sims():
    """One BatchedMujoco per (model, B), opened on first use and closed at the end of the module."""
    open_ = {}

    def get(model, n):
        if (model, n) not in open_:
            open_[(model, n)] = BatchedMujoco(n, robot_file=model)
        return open_[(model, n)]
    yield get
    for s in open_.values():
        s.close()


def abi_call(sim, opt, q, v, c, outs, no_out=False):
    """jaco_fd straight through the C ABI on device tensors (None: NULL); outs: {name: tensor}.  Returns the return code."""
    vp = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    rec = _lib.JacoFdOut(*[vp(outs.get(k)) for k in fb.OUTS])
    return sim.L.jaco_fd(sim.h, None if opt is None else ctypes.cast(ctypes.pointer(opt), ctypes.c_void_p), vp(q), vp(v), vp(c),
                         None if no_out else ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), sim._stream())


def shapes(sim):
    B, nv, nu = sim.num_envs, sim.nv, sim.nu
    return {"qacc": (B, nv), "qfrc_smooth": (B, nv), "dqacc_dqpos": (B, nv, nv), "dqacc_dqvel": (B, nv, nv), "dqacc_dctrl": (B, nu, nv)}


@pytest.fixture(scope="module")
def run(sims):
    def call(model, q, v, c, want=fb.OUTS, defaults=False, **options):
        sim = sims(model, len(q))
        outs = {k: torch.full(shapes(sim)[k], float("nan"), device="cuda:0") for k in want}
        rc = abi_call(sim, None if defaults else _lib.JacoFdOptions(**options), _dev(q), _dev(v), _dev(c), outs)
        assert rc == 0, sim.L.jaco_last_error(sim.h).decode()
        return {k: t.cpu().numpy() for k, t in outs.items()}
    return call


@pytest.fixture(scope="module")
def make_sim(sims):
    def make(model, q, v):
        sim = sims(model, len(q))
        sim.set_state(_dev(q), _dev(v), None)
        return sim
    return make


@pytest.mark.parametrize("model", (fb.MODEL,) + fb.SMALL)
def test_qacc_and_qfrc_smooth_match_the_oracle(run, model):
    a, f, ad = fb.case_values(run, model)
    print("MEASURE values %s: qacc %.3g qfrc_smooth %.3g qacc(implicit damping) %.3g" % (model, a, f, ad))
    assert a <= QACC_BOUND and f <= QFRC_BOUND and ad <= QACC_DAMPED_BOUND, (a, f, ad)


def test_the_actuator_model_clamps_and_closes_its_gates(run):
    m = fb.case_actuator_model(run)
    print("MEASURE actuator model: qacc %.3g qfrc_smooth %.3g dqacc_dctrl %.3g" % m)
    assert all(x <= b for x, b in zip(m, ACT_BOUNDS)), m


def test_a_free_body_at_rest_falls_with_gravity(run):
    e = fb.case_free_body_at_rest(run)
    print("MEASURE free body at rest: %.3g" % e)
    assert e <= FREE_BOUND, e


@pytest.mark.parametrize("model", (fb.MODEL,) + fb.SMALL)
def test_the_linearisation_matches_the_oracles_differences(run, model):
    dq, dv, du, quad = fb.case_linearisation(run, model)
    print("MEASURE linearisation %s: dqpos %.3g dqvel %.3g dctrl %.3g dqvel(0.125) - dqvel(0.5) %.3g" % (model, dq, dv, du, quad))
    assert dq < DQPOS_CAP
    assert dq <= DQPOS_BOUND and dv <= DQVEL_BOUND and du <= DCTRL_BOUND and quad <= QUADRATIC_BOUND, (dq, dv, du, quad)


def test_dof_mask_subsets(run):
    fb.case_masks(run)


def test_each_output_alone_equals_the_all_outputs_call(run):
    fb.case_output_subsets(run)


def test_against_the_stepper_in_fp64_and_on_the_device(run, make_sim):
    e, (q, v, c), ok = fb.case_stepper(run)
    print("MEASURE stepper: qvel + h qacc against one oracle substep %.3g (%d of %d envs without constraint rows)" % (e, ok.sum(), len(ok)))
    assert e <= STEP_BOUND, e
    sim = make_sim(fb.STEP_MODEL, q, v)
    ctrl = _dev(c)
    pred = sim.get_state()[1] + fb.tables(fb.STEP_MODEL)["h"] * sim.forward_dynamics(ctrl, implicit_damping=True)
    sim.send_forces(ctrl, 1)
    d = fb.verr(pred.cpu().numpy()[ok], sim.get_state()[1].cpu().numpy()[ok])
    print("MEASURE stepper: qvel + h qacc against send_forces(ctrl, 1) on the device %.3g" % d)
    assert d <= STEP_DEVICE_BOUND, d


def test_robot_config_linearize_predicts_the_next_state(make_sim):
    e = fb.case_config_linearize(make_sim)
    print("MEASURE robot_config.linearize: A x + B u + c against the oracle's substep %.3g" % e)
    assert e <= CONFIG_BOUND, e


def test_robot_config_on_the_two_arm_model(make_sim):
    e, resid = fb.case_config_two_arms(make_sim)
    print("MEASURE two arms: dq + h qacc of EE_1's joints against the oracle's substep %.3g; A x + B u + c at its own point off by %.3g" % (e, resid))
    assert e <= TWO_ARM_BOUND, e
    assert resid <= 1e-5, resid   # (fp32 assembly: x' - A x - B u cancels to 1e-7 of |x| <= 6.3)


@pytest.mark.parametrize("case", sorted(fb.REFUSALS))
def test_refusals_leave_the_output_untouched(case, sims):
    sim = sims(fb.REFUSAL_MODEL, 2)
    want, no_out, opts = fb.refusal_args(case)
    outs = {k: torch.full(shapes(sim)[k], 7.0, device="cuda:0") for k in want}
    rc = abi_call(sim, _lib.JacoFdOptions(**opts), None, None, None, outs, no_out=no_out)
    assert rc == -1 and sim.L.jaco_last_error(sim.h).decode() == "jaco_fd: " + fb.REFUSALS[case]   # (the emulator's text: test_fd_emu.py)
    assert all((t == 7.0).all() for t in outs.values())
    if opts:
        with pytest.raises(JacoError, match="jaco_fd: "):
            sim._fd(None, None, None, ("qacc",), **opts)


def test_the_handles_state_is_read_and_nothing_is_written(sims):
    """NULL qpos / qvel = get_state()'s tensors bit for bit; one launch; state, task rows, flags and sensordata bitwise unchanged."""
    g = fb.shared(fb.MODEL)
    sim = sims(fb.MODEL, fb.B)
    sim.set_state(_dev(g["q"]), _dev(g["v"]), None)
    sim.send_forces(_dev(np.random.default_rng(8).uniform(-0.2, 0.2, (fb.B, 9))), nsub=3)
    version, before, flags, sens = sim.state_version, sim.save_envs().clone(), sim.flags().clone(), sim.sensordata().clone()
    qh, vh, _ = sim.get_state()
    c = _dev(g["c"])
    sim.launch_count()   # (reading the counter resets it)
    a = sim._fd(c, None, None, fb.OUTS, dof_mask=fb.MASKS[2])
    assert sim.launch_count() == 1
    b = sim._fd(c, qh, vh, fb.OUTS, dof_mask=fb.MASKS[2])
    for k in fb.OUTS:
        assert (fb.bits(a[k].cpu().numpy()) == fb.bits(b[k].cpu().numpy())).all(), k
    assert sim.state_version == version and torch.equal(before, sim.save_envs())
    assert torch.equal(flags, sim.flags()) and torch.equal(sens, sim.sensordata())
    lin = sim.linearize(c, dofs=[0, 3, 5])   # the Python layer hands out the transposed views (fb.MASKS[2] = dofs 0, 3, 5)
    a1 = sim._fd(c, None, None, fb.OUTS, dof_mask=fb.MASKS[2], implicit_damping=1)
    assert torch.equal(lin["dq"], a1["dqacc_dqpos"].transpose(1, 2)) and torch.equal(lin["du"], a1["dqacc_dctrl"].transpose(1, 2))
    assert lin["dq"].shape == (fb.B, 21, 21) and lin["du"].shape == (fb.B, 21, 9) and (lin["dq"][:, :, [1, 2, 4]] == 0).all()


def test_gpu_agrees_with_the_emulator(run):
    g = fb.shared(fb.MODEL)
    r = run(fb.MODEL, g["q"], g["v"], g["c"], want=("qacc", "qfrc_smooth"))
    e = fb.fd(fb.MODEL, g["q"], g["v"], g["c"], want=("qacc", "qfrc_smooth"))
    m = (fb.verr(r["qacc"], e["qacc"]), fb.verr(r["qfrc_smooth"], e["qfrc_smooth"]))
    print("MEASURE gpu - emulator values: qacc %.3g qfrc_smooth %.3g" % m)
    assert all(x <= b for x, b in zip(m, EMU_VALUE_BOUNDS)), m
    n = 16
    r = run(fb.MODEL, g["q"][:n], g["v"][:n], g["c"][:n], want=fb.OUTS[2:], implicit_damping=1)
    e = fb.fd(fb.MODEL, g["q"][:n], g["v"][:n], g["c"][:n], want=fb.OUTS[2:], implicit_damping=1)
    m = tuple(fb.merr(r[k], e[k]) for k in fb.OUTS[2:])
    print("MEASURE gpu - emulator linearisation: dqpos %.3g dqvel %.3g dctrl %.3g" % m)
    assert all(x <= b for x, b in zip(m, EMU_LIN_BOUNDS)), m
    assert all((fb.bits(run(fb.MODEL, g["q"][:n], g["v"][:n], g["c"][:n], want=fb.OUTS[2:], implicit_damping=1)[k]) == fb.bits(r[k])).all() for k in fb.OUTS[2:])   # two identical calls
