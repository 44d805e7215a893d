"""The numpy statement of the coupling (tests/stack_refs.py) against poses built independently with scipy
(arm_dyn_refs.resolve_ee_targets): the tray two perfectly tracking arms hold is the tray that was commanded.  No GPU.

Bars: 1e-14 absolute.  The quantities are at most 1 in magnitude, a pose goes through a rotation matrix and back (a few
fp64 roundings of 1.1e-16 each), and on |u_i| <= 0.5 the condition number of asin, 1 / cos(pitch), is at most 1.14.
"""
import numpy as np
from scipy.spatial.transform import Rotation as Rot

import arm_dyn_refs as R
import stack_refs as S
from dart_mpc.pmpc import tilt_to_quat

TOL = 1e-14
N_POSES = 200


def _poses(seed=0):
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.5, 0.5, (N_POSES, 2))
    pos = rng.uniform(-0.5, 0.5, (N_POSES, 3))
    ee_pos, ee_quat = np.zeros((N_POSES, 2, 3)), np.zeros((N_POSES, 2, 4))
    for e in range(N_POSES):
        for a, (p, q) in enumerate(R.resolve_ee_targets(pos[e], tilt_to_quat(u[e]))):
            ee_pos[e, a], ee_quat[e, a] = p, q
    return u, pos, ee_pos, ee_quat


def test_asin_condition_number_on_the_set():
    u, _, _, _ = _poses()
    assert np.max(1.0 / np.cos(u[:, 0])) <= 1.14


def test_coupling_returns_the_commanded_tray():
    u, pos, ee_pos, ee_quat = _poses()
    m = S.tray_from_arms_batch(ee_pos, ee_quat)
    assert np.max(np.abs(m["tilt"] - u)) <= TOL
    assert np.max(np.abs(m["tray"][:, :3] - pos)) <= TOL
    quat = np.stack([tilt_to_quat(v) for v in u])
    assert np.max(np.abs(m["tray"][:, 3:] - quat)) <= TOL       # (w > 0 on this set: no sign to fix)
    for k in ("yaw", "gap", "angle"):
        assert np.max(np.abs(m[k])) <= TOL, k


def test_sign_of_either_ee_quat_is_free():
    _, _, ee_pos, ee_quat = _poses(1)
    ref = S.tray_from_arms_batch(ee_pos, ee_quat)
    for flip in ((-1, 1), (1, -1), (-1, -1)):
        q = ee_quat * np.array(flip, dtype=float)[None, :, None]
        m = S.tray_from_arms_batch(ee_pos, q)
        for k in ref:
            np.testing.assert_array_equal(m[k], ref[k], err_msg=f"{flip} {k}")


def test_rotation_about_world_z_is_yaw_only():
    u, pos, ee_pos, ee_quat = _poses(2)
    ref = S.tray_from_arms_batch(ee_pos, ee_quat)
    delta = 1e-3
    Rz = Rot.from_euler("z", delta)
    qz = np.array([np.cos(delta / 2), 0.0, 0.0, np.sin(delta / 2)])
    # both arms turned about the vertical through the tray's position
    p2 = pos[:, None, :] + np.einsum("ij,eaj->eai", Rz.as_matrix(), ee_pos - pos[:, None, :])
    q2 = np.array([[R.qmul(qz, q) for q in pair] for pair in ee_quat])
    m = S.tray_from_arms_batch(p2, q2)
    assert np.max(np.abs(m["yaw"] - delta)) <= TOL
    assert np.max(np.abs(m["tilt"] - ref["tilt"])) <= TOL
    assert np.max(np.abs(m["tray"][:, :3] - pos)) <= TOL
    assert np.max(np.abs(m["gap"])) <= TOL and np.max(np.abs(m["angle"])) <= TOL


def test_outward_displacement_is_the_gap():
    _, _, ee_pos, ee_quat = _poses(3)
    ref = S.tray_from_arms_batch(ee_pos, ee_quat)
    d = 2e-3
    axis = ee_pos[:, 1] - ee_pos[:, 0]
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    p2 = ee_pos.copy()
    p2[:, 1] += d * axis
    m = S.tray_from_arms_batch(p2, ee_quat)
    assert np.max(np.abs(m["gap"] - d)) <= TOL
    np.testing.assert_array_equal(m["tilt"], ref["tilt"])
    np.testing.assert_array_equal(m["angle"], ref["angle"])
    assert np.max(np.abs(m["tray"][:, :3] - (ref["tray"][:, :3] + 0.5 * d * axis))) <= TOL


def test_non_finite_pose_gives_non_finite_tilt_and_is_held():
    _, pos, ee_pos, ee_quat = _poses(4)
    q = ee_quat[:3].copy()
    q[1, 0, 2] = np.nan
    m = S.tray_from_arms_batch(ee_pos[:3], q)
    assert not np.isfinite(m["tilt"][1]).any() and np.isfinite(m["tilt"][[0, 2]]).all()
    sm = np.zeros((3, 8))
    held = S.stack_metrics_step(sm, m, np.zeros((3, 2)), pos[:3])
    assert held.tolist() == [False, True, False]
    assert sm[:, 6].tolist() == [0.0, 1.0, 0.0] and sm[:, 7].tolist() == [1.0, 1.0, 1.0]
    assert np.isfinite(sm).all() and sm[1, 0] == 0.0


def test_one_step_in_achieved_mode_puts_the_measured_tilt_on_the_plant():
    u, pos, ee_pos, ee_quat = _poses(5)
    E = 4
    x = np.zeros((E, 6)); x[:, 0] = 0.02
    target = np.zeros((E, 6)); target[:, 0] = 0.1
    prm = np.tile([0.1, 600, 5, 0.1, -0.6, 0.6], (E, 1))
    common = dict(k=0, do_post=1, do_pre=1, Ts=0.002, target=target, prm=prm, tray_pos=pos[:E], ee_pos=ee_pos[:E],
                  ee_quat=ee_quat[:E], x=x, tilt=np.zeros((E, 2)), metrics=np.tile([0, -1, 0, 0, 0, 0, 0, 0.0], (E, 1)),
                  stack_metrics=np.zeros((E, 8)), u0=np.full((E, 2), 0.3), f=np.zeros(E), status=np.zeros(E, np.int32),
                  iters=np.full(E, 7, np.int32))
    a = S.stack_step(False, S.ACHIEVED, **common)
    r = S.stack_step(False, S.RIDE, **common)
    assert np.max(np.abs(a["tilt"] - u[:E])) <= TOL                  # no lag: the arms are the lag
    lag = 1.0 - np.exp(-0.002 / 0.03)
    np.testing.assert_allclose(r["tilt"], lag * 0.3, rtol=1e-15)
    np.testing.assert_array_equal(a["stack_metrics"], r["stack_metrics"])     # measured alike in both modes
    np.testing.assert_allclose(a["stack_metrics"][:, 0], np.max(np.abs(u[:E] - 0.3), axis=1), atol=TOL)
    assert a["metrics"][:, 7].tolist() == [1.0] * E and a["metrics"][:, 5].tolist() == [7.0] * E
    np.testing.assert_array_equal(a["x0"][:, :4], a["x"][:, :4])
