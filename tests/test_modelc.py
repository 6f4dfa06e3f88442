"""CPU tier: the model compiler's MJCF reader (mujoco_jaco_amd/modelc/mjcf.py) on the on-disk format either side of the hot path."""
import os

import numpy as np
import pytest

from mujoco_jaco_amd.modelc import mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numeric_attributes_are_read_like_mujoco_reads_them():
    """Stream extraction: each number is the longest valid prefix; white space between numbers is optional.  The reference's own
    jaco2_torque.xml:47 has size=".01 .02.035" (three numbers for MuJoCo)."""
    assert mjcf._numbers(".01 .02.035") == [0.01, 0.02, 0.035]
    assert mjcf._numbers("1e-3 -2.5E+2 3") == [0.001, -250.0, 3.0]
    assert mjcf._numbers("0 -1.9 -1.1") == [0.0, -1.9, -1.1]
    assert mjcf._numbers("  1.  2  ") == [1.0, 2.0]
    assert mjcf._numbers("-.5-.5") == [-0.5, -0.5]
    with pytest.raises(ValueError):
        mjcf._numbers("1 x 2")
    assert np.array_equal(mjcf._floats(".3", n=3, default=(1, 2, 3)), [0.3, 2, 3])


def test_sibling_models_keep_their_sizes():
    """The compiled sibling models (mujoco_jaco_amd/assets/*.jacomdl, what modelc/compile.py made of the reference's MJCF files, which
    are not part of this repository): jaco2_torque (12 hinge joints incl. the sprung distal finger joints, xml:109-133) and the old
    curtain model are there; the default model and the arm-only model keep the sizes SURVEY.md section 8a lists."""
    from mujoco_jaco_amd.modelc import blob
    sizes = {}
    for name in ("jaco2_curtain_torque", "jaco2_reaching_torque", "jaco2_torque", "jaco2_curtain_torque_old", "jaco2_curtain_torque_sensor"):
        M = blob.load(os.path.join(ROOT, "mujoco_jaco_amd", "assets", name + ".jacomdl"))
        sizes[name] = (int(M["nq"][0]), int(M["nv"][0]), int(M["nu"][0]), int(M["njnt"][0]))
    assert sizes["jaco2_curtain_torque"] == (23, 21, 9, 11) and sizes["jaco2_reaching_torque"] == (9, 9, 9, 9)
    assert sizes["jaco2_torque"] == (12, 12, 9, 12) and sizes["jaco2_curtain_torque_old"][3] == 13


def test_compiled_model_against_the_surveys_model_table():
    """An independent pin of the MJCF reader: SURVEY.md section 8a's model table was read off jaco2_curtain_torque.xml by the surveyor
    (line numbers cited there), not produced by this compiler.  The compiled blob must hold those numbers: an MJCF-convention error in
    modelc would otherwise be common to the kernel and the oracle (both read the blob)."""
    from mujoco_jaco_amd.modelc import blob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    M = blob.load(os.path.join(root, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.jacomdl"))
    names = {}
    for line in open(os.path.join(root, "mujoco_jaco_amd", "assets", "jaco2_curtain_torque.names.txt")):
        k, v = line.strip().split(": ", 1)
        names[k] = v.split()
    B = {n: i for i, n in enumerate(names["body"])}
    J = {n: i for i, n in enumerate(names["joint"]) if n != "-"}
    pos, mass, ipos = M["body_pos"].reshape(-1, 3), M["body_mass"], M["body_ipos"].reshape(-1, 3)
    # frame positions and inertial rows (xml:109-140)
    for body, p in (("link1", (0, 0, 0.157)), ("link2", (0, 0.0016, 0.1186)), ("link3", (0, 0, 0.410)), ("link4", (0, -0.0115, 0.2072)),
                    ("link5", (0, 0.037, 0.0641)), ("link6", (0, 0.037, 0.0641)), ("EE", (0, 0, 0.12)), ("object_body", (1, 1.2, 1)), ("object_dest", (0.6, 0.3, 0.09))):
        assert np.allclose(pos[B[body]], p, atol=1e-12), body
    for body, m in (("link1", 0.754), ("link2", 1.01), ("link3", 0.559), ("link4", 0.417), ("link5", 0.417), ("link6", 0.727)):
        assert abs(mass[B[body]] - m) < 1e-12, body
    assert np.allclose(ipos[B["link1"]], (-4.2e-5, -1.285e-3, 0.112784)) and np.allclose(ipos[B["link2"]], (1.4e-5, 0.009353, 0.329006))
    # joints: axes (normalised at compile; joint4 is `0 -1.9 -1.1` in the XML), reference angles, ranges, damping (xml:113-144,172,208,244)
    ax, rng, q0 = M["jnt_axis"].reshape(-1, 3), M["jnt_range"].reshape(-1, 2), M["qpos0"]
    assert np.allclose(ax[J["joint0"]], (0, 0, -1)) and np.allclose(ax[J["joint1"]], (0, -1, 0)) and np.allclose(ax[J["joint2"]], (0, 1, 0))
    assert np.allclose(ax[J["joint4"]], np.array([0, -1.9, -1.1]) / np.linalg.norm([1.9, 1.1])) and np.allclose(ax[J["joint_thumb"]], (1, 0, 0)) and np.allclose(ax[J["joint_index"]], (-1, 0, 0))
    qa = M["jnt_qposadr"]
    assert q0[qa[J["joint1"]]] == 3.14 and q0[qa[J["joint2"]]] == 3.14 and q0[qa[J["joint_thumb"]]] == 1.1
    assert np.allclose(rng[J["joint1"]], (0.872665, 5.41052)) and np.allclose(rng[J["joint2"]], (0.331613, 5.95157)) and np.allclose(rng[J["joint_thumb"]], (0, 1.51))
    da = M["jnt_dofadr"]
    assert all(M["dof_damping"][da[J[j]]] == 0.15 for j in ("joint_thumb", "joint_index", "joint_pinky")) and M["dof_damping"][:6].max() == 0
    # free bodies from their geoms (no <inertial>): box .027 x .027 x .03 at density 100 -> 0.017496 kg; pedestal .1 x .1 x .16 at 1e5 -> 1280 kg
    assert abs(mass[B["object_body"]] - 8 * 0.027 * 0.027 * 0.03 * 100) < 1e-12 and abs(mass[B["object_dest"]] - 8 * 0.1 * 0.1 * 0.16 * 1e5) < 1e-6
    # actuators (xml:341-349): 6 motors with force ranges 30 / 15, 3 position servos kp 20, ctrlrange [0, 1.51], force +-0.3
    fr = M["actuator_forcerange"].reshape(-1, 2)
    assert np.allclose(fr[:6, 1], (30, 30, 30, 15, 15, 15)) and np.allclose(fr[6:, 1], 0.3) and np.allclose(M["actuator_kp"][6:], 20)
    assert list(M["actuator_position"]) == [0] * 6 + [1] * 3 and np.allclose(M["actuator_ctrlrange"].reshape(-1, 2)[6:], (0, 1.51))
    # contact parameters of the object and the hand mesh (xml:141,292): friction .95 .3 .1, solref .001 1; condim 6, solref .01
    G = {n: i for i, n in enumerate(names["geom"]) if n != "-"}
    gobj = int(np.where(M["geom_bodyid"] == B["object_body"])[0][0])
    assert np.allclose(M["geom_friction"].reshape(-1, 3)[gobj], (0.95, 0.3, 0.1)) and np.allclose(M["geom_solref"].reshape(-1, 2)[gobj], (0.001, 1))
    assert M["geom_condim"][G["link6"]] == 6 and np.allclose(M["geom_solref"].reshape(-1, 2)[G["link6"]], (0.01, 1))
    assert float(M["opt_timestep"][0]) == 0.001 and np.allclose(M["opt_gravity"], (0, 0, -9.81))


def test_cylinder_geoms_and_zaxis_frames_in_the_shipped_sensor_model():
    """jaco2_curtain_torque_sensor.xml:62-74,278-281: five static cylinders -- two posts (.01 x .4), the rod (.01 x .5, axis turned onto x by
    `zaxis="1 0 0"`), the object holder's stem (.01 x .2) and disc (.1 x .01).  Read from the compiled asset (no reference needed)."""
    from mujoco_jaco_amd import _lib
    from mujoco_jaco_amd.modelc import blob, rot
    M = blob.load(_lib.model_path("jaco2_curtain_torque_sensor"))
    cyl = np.nonzero(M["geom_type"] == mjcf.GEOM_CYLINDER)[0]
    size = M["geom_size"].reshape(-1, 3)[cyl]
    assert sorted(map(tuple, np.round(size[:, :2], 6).tolist())) == sorted([(.01, .4), (.01, .4), (.01, .5), (.01, .2), (.1, .01)])
    assert np.allclose(M["geom_rbound"][cyl], np.hypot(size[:, 0], size[:, 1]))
    quat = M["geom_quat"].reshape(-1, 4)[cyl]
    rod = int(np.nonzero(np.abs(size[:, 1] - 0.5) < 1e-12)[0][0])
    assert np.allclose(rot.quat_to_mat(quat[rod]) @ [0, 0, 1], [1, 0, 0], atol=1e-12)       # the rod lies along x
    for i in range(len(cyl)):
        if i != rod:
            assert np.allclose(quat[i], [1, 0, 0, 0])
    # the minimal rotation: about y by +90 degrees, nothing about the axis itself
    assert np.allclose(quat[rod], [np.sqrt(0.5), 0, np.sqrt(0.5), 0], atol=1e-12)


def test_cylinder_mass_properties():
    """A moving cylinder's mass and inertia from its density (none of the shipped assets has one; the formulae are MuJoCo's [EXT])."""
    import tempfile
    xml = """<mujoco><worldbody><body name="b" pos="0 0 1"><freejoint/><geom type="cylinder" size=".05 .2" density="1000"/></body></worldbody></mujoco>"""
    with tempfile.NamedTemporaryFile("w", suffix=".xml", delete=False) as f:
        f.write(xml)
    try:
        M, names = mjcf.parse(f.name, timestep=0.001)
    finally:
        os.remove(f.name)
    m = 1000 * np.pi * 0.05 ** 2 * 0.4
    assert np.isclose(M["body_mass"][1], m)
    assert np.allclose(M["body_inertia"].reshape(-1, 3, 3)[1], np.diag([m * (0.05 ** 2 / 4 + 0.2 ** 2 / 3)] * 2 + [m * 0.05 ** 2 / 2]))
