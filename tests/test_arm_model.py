"""The arm model table (dart_mpc/arm_model.py), its MJCF loader, the committed xArm7 fixture and the pure entries of the
arm-dynamics ABI; no GPU."""
import ctypes
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "xarm7_arm_models.npz")

DEFAULTS = """
<mujoco><default>
  <default class="arm">
    <joint axis="0 0 1" armature="0.1" range="-3 3"/>
    <default class="big"><joint damping="10"/></default>
    <default class="small"><joint damping="2" armature="0.05" axis="0 1 0"/></default>
  </default>
</default></mujoco>
"""
CHAIN = """
<mujocoinclude>
<body name="base" pos="0 0 0.1" childclass="arm">
  <inertial pos="0 0 0" mass="5" diaginertia="1 1 1"/>
  <body name="l1" pos="0 0 0.2">
    <inertial pos="0 0 0.1" mass="2" diaginertia="0.01 0.02 0.03"/>
    <joint name="j1" class="big"/>
    <body name="l2" pos="0.3 0 0" quat="1 1 0 0">
      <inertial pos="0.1 0 0" quat="1 0 0 1" mass="1.5" diaginertia="0.004 0.005 0.006"/>
      <joint name="j2" range="-1 2"/>
      <geom size="0.1"/>
      <body name="l3" pos="0 0.25 0">
        <inertial pos="0 0 0.05" mass="1" diaginertia="0.001 0.001 0.002"/>
        <joint name="j3" class="small"/>
        <body name="tool" pos="0 0 0.1" quat="0 0 0 1">
          <inertial pos="0 0.02 0" mass="0.5" diaginertia="0.0003 0.0002 0.0001"/>
          <site name="tcp" pos="0 0 0.1"/>
          <body name="finger" pos="0 0.03 0.05">
            <inertial pos="0 0 0.01" mass="0.1" diaginertia="1e-5 1e-5 1e-5"/>
            <joint name="finger_joint" axis="1 0 0"/>
          </body>
        </body>
      </body>
    </body>
  </body>
</body>
</mujocoinclude>
"""


def _load(chain=CHAIN, **over):
    from dart_mpc.arm_model import ArmModel
    kw = dict(base_pos=[1, 2, 3], base_quat=[2, 0, 0, 0], joints=["j1", "j2", "j3"], body_name="tool", offset=0.05,
              gravity=[0, 0, -9.81])
    kw.update(over)
    return ArmModel.from_mjcf(chain, DEFAULTS, **kw)


def test_from_mjcf_three_links_defaults_and_fixed_child():
    m = _load()
    assert m.n == 3 and m.row().shape == (22 * 3 + 18,)
    np.testing.assert_allclose(m.base_pos, [1, 2, 3.3])             # base o <body base> o <body l1>
    np.testing.assert_allclose(m.base_quat, [1, 0, 0, 0])
    np.testing.assert_allclose(m.pos, [[0, 0, 0], [0.3, 0, 0], [0, 0.25, 0]])
    np.testing.assert_allclose(m.quat[1], np.array([1, 1, 0, 0]) / np.sqrt(2))
    # <default> inheritance: class big / the childclass arm / class small overriding axis and armature
    np.testing.assert_allclose(m.axis, [[0, 0, 1], [0, 0, 1], [0, 1, 0]])
    np.testing.assert_allclose(m.armature, [0.1, 0.1, 0.05])
    np.testing.assert_allclose(m.damping, [10, 0, 2])
    np.testing.assert_allclose(m.limits, [[-3, 3], [-1, 2], [-3, 3]])
    # link 2's inertial frame is turned 90 degrees about z: x and y principal moments swap
    np.testing.assert_allclose(m.inertia[1], [0.005, 0.004, 0.006, 0, 0, 0], atol=1e-15)
    # the last link composes tool (turned 180 degrees about z) and the finger held at 0
    parts = [(1.0, np.array([0, 0, 0.05])), (0.5, np.array([0, -0.02, 0.1])), (0.1, np.array([0, -0.03, 0.16]))]
    mass = sum(p[0] for p in parts)
    com = sum(p[0] * p[1] for p in parts) / mass
    assert m.mass[2] == pytest.approx(mass, rel=1e-15)
    np.testing.assert_allclose(m.com[2], com, atol=1e-15)
    I = np.diag([0.001, 0.001, 0.002]) + np.diag([0.0003, 0.0002, 0.0001]) + 1e-5 * np.eye(3)
    for mk, c in parts:
        d = c - com
        I = I + mk * ((d @ d) * np.eye(3) - np.outer(d, d))
    np.testing.assert_allclose(m.inertia[2], [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]], atol=1e-15)
    np.testing.assert_allclose(m.ee_pos, [0, 0, 0.1])
    np.testing.assert_allclose(m.ee_quat, [0, 0, 0, 1])
    # row() and from_row() are inverses
    from dart_mpc.arm_model import ArmModel
    np.testing.assert_array_equal(ArmModel.from_row(m.row(), 3).row(), m.row())


def test_from_mjcf_rejects_what_it_does_not_model():
    from dart_mpc import DartMPCError
    with pytest.raises(DartMPCError, match="slide"):
        _load(CHAIN.replace('<joint name="j2" range="-1 2"/>', '<joint name="j2" type="slide"/>'))
    with pytest.raises(DartMPCError, match="'pos'.*j3"):
        _load(CHAIN.replace('<joint name="j3" class="small"/>', '<joint name="j3" class="small" pos="0 0 0.1"/>'))
    with pytest.raises(DartMPCError, match="fullinertia"):
        _load(CHAIN.replace('mass="1" diaginertia="0.001 0.001 0.002"', 'mass="1" fullinertia="1 1 1 0 0 0"'))
    with pytest.raises(DartMPCError, match="freejoint"):
        _load(CHAIN.replace('<site name="tcp" pos="0 0 0.1"/>', "<freejoint/>"))
    with pytest.raises(DartMPCError, match="euler"):
        _load(CHAIN.replace('<body name="l3" pos="0 0.25 0">', '<body name="l3" euler="0 0 1">'))
    with pytest.raises(DartMPCError, match="j9"):
        _load(joints=["j1", "j2", "j9"])
    with pytest.raises(DartMPCError, match="nothing"):
        _load(body_name="nothing")


def test_from_arrays_and_payload():
    from dart_mpc.arm_model import ArmModel
    m = _load()
    f = dict(base_pos=m.base_pos, base_quat=m.base_quat, pos=m.pos, quat=m.quat, axis=m.axis, armature=m.armature,
             damping=m.damping, mass=m.mass, com=m.com, inertia=m.inertia, ee_pos=m.ee_pos, ee_quat=m.ee_quat,
             offset=m.offset, gravity=m.gravity)
    np.testing.assert_array_equal(ArmModel.from_arrays(**f).row(), m.row())
    p = m.with_payload(1.0)
    assert p.mass[2] == pytest.approx(m.mass[2] + 1.0) and np.array_equal(p.row()[:7 + 44], m.row()[:7 + 44])
    assert np.all(np.linalg.eigvalsh(_sym(p.inertia[2])) > 0)


def _sym(v):
    return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])


def test_committed_xarm7_fixture():
    g = np.load(GOLD)
    rows = g["rows"]
    assert rows.shape == (2, 22 * 7 + 18) and g["joint_names"].shape == (2, 7) and g["limits"].shape == (2, 7, 2)
    assert list(g["joint_names"][0]) == [f"L_joint{i}" for i in range(1, 8)]
    for r in rows:
        L = r[7:7 + 154].reshape(7, 22)
        for qv in [r[3:7], r[-8:-4]] + [k[3:7] for k in L]:
            assert abs(np.linalg.norm(qv) - 1) <= 1e-15
        for k in L:
            assert abs(np.linalg.norm(k[7:10]) - 1) <= 1e-15 and k[12] > 0 and k[10] == 0.1
            assert np.all(np.linalg.eigvalsh(_sym(k[16:22])) > 0)
        assert r[-4] == 0.125 and list(r[-3:]) == [0, 0, -9.81]
    np.testing.assert_allclose(rows[:, :3], [[-0.7, 0, 0.267], [0.7, 0, 0.267]], atol=1e-15)
    # the right arm is the left one moved: everything but the base position agrees
    np.testing.assert_array_equal(rows[0, 3:], rows[1, 3:])
    np.testing.assert_allclose(g["limits"][0][:, 0], [-6.28319, -2.059, -6.28319, -0.19198, -6.28319, -1.69297, -6.28319])


def test_pure_entries_and_argument_checks():
    import dart_mpc
    from dart_mpc.arm import ArmDynConfig, arm_config, arm_dyn_config
    L = dart_mpc.lib()
    assert L.dart_arm_model_len(7) == 172 and L.dart_arm_state_len(7) == 28 and L.dart_mpc_abi_version() == 8
    assert L.dart_arm_model_len(0) == -1 and L.dart_arm_model_len(9) == -1 and L.dart_arm_state_len(9) == -1
    assert L.dart_dual_arm_work_len(18, 7) == 36 * (206 + 17) and L.dart_dual_arm_work_len(0, 7) == -1
    d, c = arm_dyn_config(), arm_config()
    assert d.jacdot_point == 0 and list(d.reserved) == [0] * 7
    x = np.zeros(4096)
    p = ctypes.c_void_p(x.ctypes.data)          # a non-null pointer: every call below returns before using it
    z = None
    dyn = lambda cfg, B, n, ptrs=(p, p, p), stride=0: L.dart_arm_dynamics_batch(  # noqa: E731
        ctypes.byref(cfg), B, n, ptrs[0], stride, ptrs[1], ptrs[2], z)
    assert dyn(d, 1, 0) == -1 and dyn(d, 1, 9) == -1 and dyn(d, 0, 7) == -1 and dyn(d, -3, 7) == -1
    assert dyn(d, 1, 7, (z, p, p)) == -1 and dyn(d, 1, 7, (p, z, p)) == -1 and dyn(d, 1, 7, (p, p, z)) == -1
    assert dyn(d, 1, 7, stride=100) == -1
    assert dyn(ArmDynConfig(jacdot_point=2), 1, 7) == -1
    assert L.dart_arm_dynamics_batch(None, 1, 7, p, 0, p, p, z) == -1
    assert L.dart_arm_dynamics_batch_dev(ctypes.byref(d), 1, 9, p, 0, p, p, z, z) == -1
    ctl = lambda B, n, snapless=False: L.dart_arm_control_batch(  # noqa: E731
        ctypes.byref(d), ctypes.byref(c), B, n, p, 0, p, p, 0, z, *([z if snapless else p] * 5))
    assert ctl(1, 9) == -1 and ctl(0, 7) == -1 and ctl(1, 7, True) == -1
    assert L.dart_arm_control_batch_dev(ctypes.byref(d), ctypes.byref(c), 1, 7, p, 0, p, p, 0, z, p, p, p, p, p, z) == -1
    dual = lambda E, n, first=p: L.dart_dual_arm_control(  # noqa: E731
        ctypes.byref(d), ctypes.byref(c), E, n, first, *([p] * 6), 0, z, z, *([p] * 5))
    assert dual(0, 7) == -1 and dual(1, 9) == -1 and dual(1, 7, z) == -1
    roll = lambda E, n, steps, rows, logs: L.dart_dual_arm_rollout(  # noqa: E731
        ctypes.byref(d), ctypes.byref(c), E, n, steps, rows, *([p] * 5), 0, *([p] * 4), *logs)
    assert roll(0, 7, 1, 1, [z] * 6) == -1 and roll(1, 9, 1, 1, [z] * 6) == -1 and roll(1, 7, -1, 1, [z] * 6) == -1
    assert roll(1, 7, 5, 3, [z] * 6) == -1                     # tray rows neither 1 nor steps
    assert roll(1, 7, 5, 1, [p, z, z, z, z, z]) == -1          # some logs set, others not
