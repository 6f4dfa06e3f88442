"""GPU tier: the device launches and emu_sim.EmuSim's stand-in launches sit under the same public methods -- query, ik, osc (jaco_osc and
jaco_osc_task) and joint called with the same rows on a BatchedMujoco and on an EmuSim agree.  jaco2_curtain_torque, B = 5, states
osc_binding.states.

Bounds: each entry's own device-against-emulator bound and measure (test_gpu_ik.GPU_EMU_QPOS_BOUND, test_gpu_osc.EMU_BOUND,
test_gpu_osc_task.EMU_BOUND, test_gpu_joint.EMU_BOUND).  jaco_query has no such test: its device results (test_gpu_query) and its emulated
ones (test_query_emu) are each held to the fp64 oracle on picking states with the bounds below, in the measures below, so the two differ
by at most the sum of the two bounds -- twice each number.  ik's status words and the OSC entry reached compare exactly.
"""
import numpy as np
import pytest
import torch

import ik_binding as ib
import joint_binding as jb
import osc_binding as ob
import osc_task_binding as tb
from emu_sim import EmuSim
from mujoco_jaco_amd.physics import BatchedMujoco
from test_gpu_ik import GPU_EMU_QPOS_BOUND
from test_gpu_joint import EMU_BOUND as JOINT_EMU_BOUND
from test_gpu_osc import EMU_BOUND as OSC_EMU_BOUND
from test_gpu_osc_task import EMU_BOUND as OSC_TASK_EMU_BOUND

pytestmark = pytest.mark.gpu
MODEL, B = "jaco2_curtain_torque", 5
QUERY_ORACLE_BOUNDS = dict(xpos=3.5e-7, xmat=8e-7, jac=8e-7, qM=1.6e-7, qfrc_bias=4e-7)   # test_gpu_query / test_query_emu, default model


def answers(sim, g):
    """The five calls on `sim` (a BatchedMujoco or an EmuSim at the states g["q"], g["v"]) with g's rows on its device, as numpy; "entries":
    the C entry each of the two osc calls reached."""
    T = lambda a: torch.as_tensor(a, device=sim.device)
    entries, inner = [], sim._osc
    sim._osc = lambda *a, **k: (entries.append("jaco_osc" if a[6] is None else "jaco_osc_task"), inner(*a, **k))[1]
    fr = sim.frames.jaco_frame("EE")
    r = dict(query=sim.query([fr]), ik=sim.ik(sim.frames.jaco_frame("EE", point=np.zeros(3)), T(g["P"]), T(g["Qt"])),
             osc=sim.osc(fr, T(g["tp"]), T(g["tq"])), osc_pos=sim.osc(fr, T(g["tp"]), axes=tb.POS),
             joint=dict(ctrl=sim.joint(T(g["t"]), T(g["tv"]), T(g["ff"]))))
    del sim._osc
    out = {name: {k: t.cpu().numpy() for k, t in d.items()} for name, d in r.items()}
    out["entries"] = entries
    return out


def test_device_and_emulator_launches_agree_under_the_public_methods():
    q, v = ob.states(MODEL, B)
    tp, tq = ob.kernel_targets(ob.targets6(MODEL, "EE", q)[:, None, :])
    P, Qt, _ = ib.targets(MODEL, "EE", [0, 0, 0], q, 0.3)
    g = dict(q=q, v=v, tp=tp, tq=tq, P=P, Qt=Qt, t=jb.targets(MODEL, q), tv=jb.rates(MODEL, B, 14, 0.5), ff=jb.rates(MODEL, B, 15, 2.0))
    emu = EmuSim(MODEL, q, v)
    e = answers(emu, g)
    dev = BatchedMujoco(B, robot_file=MODEL)
    dev.set_state(torch.tensor(q, device=dev.device), torch.tensor(v, device=dev.device), None)
    d = answers(dev, g)
    dev.close()
    # query: absolute for the poses and the Jacobian, relative to the env's largest entry for qM and qfrc_bias
    rel = lambda a, b: (np.abs(a - b).reshape(B, -1).max(1) / np.maximum(np.abs(b).reshape(B, -1).max(1), 1e-9)).max()
    qerr = {k: (rel if k in ("qM", "qfrc_bias") else lambda a, b: np.abs(a - b).max())(d["query"][k], e["query"][k]) for k in QUERY_ORACLE_BOUNDS}
    # ik: the configurations on the envs both converge on; the status words exactly
    both = d["ik"]["converged"] & e["ik"]["converged"]
    ik_dq = np.abs(d["ik"]["qpos"] - e["ik"]["qpos"])[both].max()
    mot = jb.motors(MODEL, jb.motor_dofs(MODEL))
    osc_err = ob.error(d["osc"]["ctrl"][:, :6], e["osc"]["ctrl"][:, :6]).max()
    pos_err = ob.error(d["osc_pos"]["ctrl"][:, :6], e["osc_pos"]["ctrl"][:, :6]).max()
    joint_err = jb.error(d["joint"]["ctrl"][:, mot], e["joint"]["ctrl"][:, mot]).max()
    print("MEASURE device - EmuSim: query %s; ik |dqpos| %.3g on %d envs, iters %s / %s; osc %.3g, osc position only %.3g, joint %.3g"
          % ({k: "%.3g" % x for k, x in qerr.items()}, ik_dq, both.sum(), d["ik"]["iters"], e["ik"]["iters"], osc_err, pos_err, joint_err))
    for k, bound in QUERY_ORACLE_BOUNDS.items():
        assert qerr[k] < 2 * bound, (k, qerr[k])
    assert both.all() and (d["ik"]["iters"] == e["ik"]["iters"]).all() and d["ik"]["iters"].dtype == e["ik"]["iters"].dtype == np.int32
    assert ik_dq < GPU_EMU_QPOS_BOUND, ik_dq
    assert d["entries"] == e["entries"] == ["jaco_osc", "jaco_osc_task"]
    assert emu.launches == dict.fromkeys(emu.launches, 0) | dict(jaco_query=1, jaco_ik=1, jaco_osc=1, jaco_osc_task=1, jaco_joint=1)
    assert osc_err <= OSC_EMU_BOUND and (d["osc"]["singular"] == e["osc"]["singular"]).all(), osc_err
    assert pos_err <= OSC_TASK_EMU_BOUND and (d["osc_pos"]["singular"] == e["osc_pos"]["singular"]).all(), pos_err
    assert joint_err <= JOINT_EMU_BOUND, joint_err
