"""The arm dynamics kernel (csrc/arm_dyn.hip), the entries built on it and the device-resident loop of the arm layer,
against the CPU references of tests/arm_dyn_refs.py.

Bars.  Every snapshot field is compared with the reference's Jacobian formulation; the bar per field is 16 x the largest
difference between the two CPU formulations on the same inputs (computed here, never from the kernel; 16 allows for a
third summation order) with the floor 1e-13, both relative to 1 + |reference|.

Measured on an MI355X (largest kernel-vs-reference difference over n in {1, 2, 3, 7, 8}, 65 arms each): ee_pos 1.3e-15,
rotvec 1.4e-15, jac 1.9e-15, jacDot 4.9e-15, M 5.9e-15, h 2.7e-14 (bar 3.7e-13 there), Mx_inv 9.0e-15; the two CPU
formulations differ by up to 2.3e-14 (h) and 2.7e-14 (Mx_inv) on the same inputs.  Rollout, E = 2, K = 20: device vs numpy
q 1.2e-14, qd 1.3e-12, tau 1.9e-11, ee_pos 4.2e-15, loss 2.2e-14 against margins 5.8e-13, 3.9e-11, 6.4e-9, 5.2e-13, 1.8e-11.
"""
import functools
import os

import numpy as np
import pytest

import arm_dyn_refs as R
import arm_qp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "xarm7_arm_models.npz")
FLOOR = 1e-13
HOME = np.array([0.0, -0.247, 0.0, 0.909, 0.0, 1.15644, 0.0])        # the scene's "home" keyframe
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def _xarm():
    g = np.load(GOLD)
    return g["rows"], g["limits"]


def _rand_states(rng, n, count, lo=None, hi=None):
    lo = -np.pi * np.ones(n) if lo is None else lo
    hi = np.pi * np.ones(n) if hi is None else hi
    S = np.zeros((count, 3 * n + 7))
    for s in S:
        v = rng.standard_normal(4)
        s[:] = np.concatenate([rng.uniform(lo, hi), rng.uniform(-2, 2, n), rng.uniform(-5, 5, n), rng.uniform(-1, 1, 3),
                               v / np.linalg.norm(v)])
    return S


@functools.lru_cache(maxsize=None)
def _case(n):
    """Per joint count: 65 per-instance models and states with both CPU formulations (jacDot REFERENCE), and the first
    two states on model 0 (jacDot BODY).  Computed once, shared by the tests, never written to."""
    rng = np.random.default_rng(100 + n)
    rows = np.stack([R.random_model(rng, n) for _ in range(65)])
    S = _rand_states(rng, n, 65)
    if n == 7:
        xr, lim = _xarm()
        rows[:2] = xr
        S[:2, :7] = rng.uniform(lim[0][:, 0], lim[0][:, 1], (2, 7))
    per = [R.snapshot_batch(rows, n, S, R.JACDOT_REFERENCE, f) for f in ("jac", "rec")]
    shared = [R.snapshot_batch(rows[0], n, S[:2], R.JACDOT_BODY, f) for f in ("jac", "rec")]
    return rows, S, per, shared


def _bars(a, b):
    return {k: max(16.0 * v, FLOOR) for k, v in R.form_difference(a, b).items()}


def _check_fields(snap_rows, n, ref, bars, what):
    from dart_mpc.arm import unpack_snapshot
    got = unpack_snapshot(snap_rows, n)
    worst = {}
    for k in R.SNAP_KEYS:
        worst[k] = float(np.max(np.abs(got[k] - ref[k]) / (1.0 + np.abs(ref[k]))))
    print(what, "kernel vs reference:", {k: f"{v:.1e}" for k, v in worst.items()}, "bars:",
          {k: f"{v:.1e}" for k, v in bars.items()})
    for k in R.SNAP_KEYS:
        assert worst[k] <= bars[k], (what, k, worst[k], bars[k])
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_snapshot_fields_host(n):
    """B = 65 per-instance model rows (jacDot REFERENCE), B = 2 and B = 1 on a shared row (jacDot BODY); M bit-symmetric.
    (Measured differences: the module docstring and DESIGN.md section 6b.)"""
    from dart_mpc.arm import ArmDynamics, JACDOT_BODY
    rows, S, per, shared = _case(n)
    snap, eq = ArmDynamics(rows, n).dynamics_batch(S, want_ee_quat=True)
    got = _check_fields(snap, n, per[0], _bars(*per), f"n={n} B=65 per-instance")
    assert np.array_equal(got["M"], np.swapaxes(got["M"], 1, 2))
    sign = np.sign(np.sum(eq * per[1]["ee_quat"], axis=1))[:, None]
    assert np.max(np.abs(eq - sign * per[1]["ee_quat"])) <= 1e-14
    dyn = ArmDynamics(rows[0], n, jacdot_point=JACDOT_BODY)
    s2 = dyn.dynamics_batch(S[:2])
    _check_fields(s2, n, shared[0], _bars(*shared), f"n={n} B=2 shared")
    s1 = dyn.dynamics_batch(S[:1])
    assert np.array_equal(s1, s2[:1])


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_snapshot_device_path(n):
    """dart_arm_dynamics_batch_dev on device pointers, B in {1, 2, 65}, shared and per-instance rows: the bits of the
    host path."""
    import torch
    from dart_mpc.arm import ArmDynamics
    rows, S, _, _ = _case(n)
    dev = torch.device("cuda", 0)
    dyn = ArmDynamics(rows, n)
    host = dyn.dynamics_batch(S)
    host_shared = ArmDynamics(rows[0], n).dynamics_batch(S)
    d_rows, d_S = torch.tensor(rows, device=dev), torch.tensor(S, device=dev)
    for B in (1, 2, 65):
        for shared, want in ((False, host), (True, host_shared)):
            out = torch.full((B, dyn.snap_len), float("nan"), dtype=torch.float64, device=dev)
            eq = torch.zeros((B, 4), dtype=torch.float64, device=dev)
            dyn.dynamics_batch_dev(B, d_rows.data_ptr(), shared, d_S.data_ptr(), out.data_ptr(), eq.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want[:B]), (n, B, shared)


def test_rest_state_and_closed_forms():
    """q = qd = 0: jacDot is exactly 0 and h is the gravity torque; the pendulum and the planar 2R arm to
    1e-12 (1 + |.|) (a few hundred fp64 operations on O(1) data)."""
    from test_arm_dyn_refs import pendulum_exact, pendulum_row, planar_2r_exact, planar_2r_row
    from dart_mpc.arm import ArmDynamics, unpack_snapshot
    xr, _ = _xarm()
    dyn = ArmDynamics(xr[0], 7)
    s0 = np.concatenate([np.zeros(21), [0.1, 0.2, 0.3], IDENT])[None]
    got = unpack_snapshot(dyn.dynamics_batch(s0), 7)
    assert np.all(got["jacDot"] == 0.0)
    ref = [R.snapshot_batch(xr[0], 7, s0, form=f) for f in ("jac", "rec")]
    m = R.unpack(xr[0], 7)
    Rs, ps, _, _ = R.frames_mat(m, np.zeros(7))
    z, pc, _ = R._geometry(m, Rs, ps)
    grav = -sum(m["mass"][k] * R.point_jac(z, ps, pc[k], k)[:3].T @ m["gravity"] for k in range(7))
    bar = _bars(*ref)["h"]
    assert np.max(np.abs(got["h"][0] - grav) / (1 + np.abs(grav))) <= bar
    rng = np.random.default_rng(21)
    q1, qd1 = rng.uniform(-3, 3, (9, 1)), rng.uniform(-2, 2, (9, 1))
    d1 = ArmDynamics(pendulum_row(), 1)
    g1 = unpack_snapshot(d1.dynamics_batch(d1.pack_state(q1, qd1, 0 * q1, np.zeros((9, 3)), np.tile(IDENT, (9, 1)))), 1)
    for b in range(9):
        M, h = pendulum_exact(q1[b, 0])
        assert abs(g1["M"][b, 0, 0] - M) <= 1e-12 * (1 + abs(M)) and abs(g1["h"][b, 0] - h) <= 1e-12 * (1 + abs(h))
    q2, qd2 = rng.uniform(-3, 3, (9, 2)), rng.uniform(-2, 2, (9, 2))
    d2 = ArmDynamics(planar_2r_row(), 2)
    g2 = unpack_snapshot(d2.dynamics_batch(d2.pack_state(q2, qd2, 0 * q2, np.zeros((9, 3)), np.tile(IDENT, (9, 1)))), 2)
    for b in range(9):
        M, h = planar_2r_exact(q2[b], qd2[b])
        assert np.all(np.abs(g2["M"][b] - M) <= 1e-12 * (1 + np.abs(M)))
        assert np.all(np.abs(g2["h"][b] - h) <= 1e-12 * (1 + np.abs(h)))


def test_stretched_xarm7_is_rank_deficient_and_finite():
    from dart_mpc.arm import ArmDynamics, unpack_snapshot
    xr, _ = _xarm()
    rng = np.random.default_rng(31)
    S = _rand_states(rng, 7, 4)
    S[:, [1, 3, 5]] = 0.0
    ref = [R.snapshot_batch(xr[0], 7, S, form=f) for f in ("jac", "rec")]
    bars = _bars(*ref)
    got = _check_fields(ArmDynamics(xr[0], 7).dynamics_batch(S), 7, ref[0], bars, "stretched xArm7")
    assert np.all(np.isfinite(got["Mx_inv"]))
    # the xArm7's link offsets (52.5, 77.5, 76 mm) keep the stretched arm a hair away from an exact singularity (CPU
    # reference: smallest / largest eigenvalue of Mx_inv 3e-7 .. 4e-5 on these states): rank is lost in the QP's own
    # sense, an eigenvalue below its pinv rcond 1e-3 of the largest.  The kernel's spectrum is the reference's within
    # the field's bar (eigenvalues of a symmetric matrix move by at most the perturbation's norm, <= 6 max |entry|)
    for Mx, Mr in zip(got["Mx_inv"], ref[0]["Mx_inv"]):
        w, wr = np.linalg.eigvalsh(Mx), np.linalg.eigvalsh(Mr)
        print("stretched arm: eigenvalues of Mx_inv", w)
        assert wr[0] <= 1e-3 * wr[-1]
        assert np.max(np.abs(w - wr)) <= 6 * bars["Mx_inv"] * (1 + np.max(np.abs(Mr)))


def test_orientation_error_cases():
    """Identity, theta = 1e-4 and 1e-3 -+ 1e-6 (the series switch), w = +-1e-3 (the double cover), -mocap_quat."""
    from dart_mpc.arm import ArmDynamics, unpack_snapshot
    xr, _ = _xarm()
    dyn = ArmDynamics(xr[0], 7)
    q = HOME + 0.1
    base = np.concatenate([q, np.zeros(14), np.zeros(3), IDENT])[None]
    _, eq = dyn.dynamics_batch(base, want_ee_quat=True)
    u = np.array([0.3, -0.5, 0.8]); u /= np.linalg.norm(u)
    errs = [IDENT]
    for th in (1e-4, 1e-3 - 1e-6, 1e-3 + 1e-6):
        errs.append(np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * u]))
    for w in (1e-3, -1e-3):
        errs.append(np.concatenate([[w], np.sqrt(1 - w * w) * u]))
    S = np.repeat(base, 2 * len(errs), axis=0)
    for i, e in enumerate(errs):
        S[2 * i, -4:] = R.qmul(e, eq[0])
        S[2 * i + 1, -4:] = -S[2 * i, -4:]
    got = unpack_snapshot(dyn.dynamics_batch(S), 7)
    ref = [R.snapshot_batch(xr[0], 7, S, form=f) for f in ("jac", "rec")]
    bar = _bars(*ref)["rotvec"]
    d = np.abs(got["rotvec"] - ref[0]["rotvec"]) / (1 + np.abs(ref[0]["rotvec"]))
    print("rotvec cases: kernel vs scipy", d.max(axis=1), "bar", bar)
    assert d.max() <= bar
    # exact angles: the error quaternion is a product of unit quaternions, each component good to a few eps (~5e-16),
    # and the angle is twice its vector part: 4e-15
    assert np.max(np.abs(got["rotvec"][0])) <= 4e-15                                     # identity
    assert np.array_equal(got["rotvec"][0::2], got["rotvec"][1::2])                      # the sign of mocap_quat
    th = np.linalg.norm(got["rotvec"], axis=1)
    assert abs(th[2] - 1e-4) <= 4e-15 and abs(th[8] - 2 * np.arctan2(np.sqrt(1 - 1e-6), 1e-3)) <= 4e-15


def test_nan_state_gives_nan_snapshot_and_breakdown():
    import dart_mpc
    from dart_mpc.arm import ArmDynamics, pack_params, unpack_snapshot
    xr, _ = _xarm()
    dyn = ArmDynamics(xr[0], 7)
    S = _rand_states(np.random.default_rng(41), 7, 3)
    S[:, :7] = HOME
    S[1, 2] = np.nan
    out = dyn.control_batch(S, pack_params(arm_qp.default_params()), want_snap=True)
    got = unpack_snapshot(out["snap"], 7)
    for k in ("q", "jac", "M", "h", "Mx_inv", "ee_pos"):
        assert np.any(np.isnan(got[k][1])) and np.all(np.isfinite(got[k][[0, 2]])), k
    assert np.all(np.isnan(got["Mx_inv"][1]))
    assert out["status"][1] == dart_mpc.arm.BREAKDOWN and out["iters"][1] == 0 and np.isnan(out["loss"][1])
    S[1, 2] = 0.0
    clean = dyn.control_batch(S, pack_params(arm_qp.default_params()), want_snap=True)
    for k in ("qdd", "tau", "loss", "status", "iters", "snap"):                 # the other instances are not affected
        assert np.array_equal(out[k][[0, 2]], clean[k][[0, 2]]), k


@functools.lru_cache(maxsize=None)
def _xarm_control_case():
    from dart_mpc.arm import ArmDynamics, pack_params
    xr, lim = _xarm()
    rng = np.random.default_rng(51)
    S = _rand_states(rng, 7, 36, lim[0][:, 0], lim[0][:, 1])
    S[:, 7:14] *= 0.5
    S[:, 14:21] = 0.0
    dyn = ArmDynamics(np.tile(xr, (18, 1)), 7)
    # targets near the arm: the EE pose of a nearby configuration
    near = S.copy()
    near[:, :7] += rng.uniform(-0.05, 0.05, (36, 7))
    sn, eq = dyn.dynamics_batch(near, want_ee_quat=True)
    S[:, 21:24] = sn[:, 24:27]
    S[:, 24:28] = eq
    prm = arm_qp.default_params()
    return dyn, S, prm, pack_params(prm)


def test_control_batch_is_dynamics_then_solve():
    import dart_mpc
    dyn, S, _, prow = _xarm_control_case()
    out = dyn.control_batch(S, prow, want_snap=True)
    snap = dyn.dynamics_batch(S)
    assert np.array_equal(out["snap"], snap)
    two = dart_mpc.ArmSolver(7).solve_batch(snap, prow)
    for k in ("qdd", "tau", "loss", "status", "iters"):
        assert np.array_equal(out[k], two[k], equal_nan=True), k


def test_control_on_xarm7_against_the_oracle():
    """36 xArm7 states inside the joint limits: the QP on the kernel's snapshots against oracle/arm_qp.py.  Statuses are
    equal; qdd and tau agree within test_gpu_arm.py's 1e-6 (1 + |.|).  Which statuses real dynamics give is printed."""
    from dart_mpc.arm import unpack_snapshot
    dyn, S, prm, prow = _xarm_control_case()
    out = dyn.control_batch(S, prow, want_snap=True)
    ref = arm_qp.solve_batch(unpack_snapshot(out["snap"], 7), prm)
    print("xArm7 QP statuses", np.unique(out["status"], return_counts=True), "iters min/median/max",
          out["iters"].min(), np.median(out["iters"]), out["iters"].max())
    assert np.array_equal(out["status"], ref["status"]), (out["status"], ref["status"])
    ok = ref["status"] >= 0
    dq = np.abs(out["qdd"] - ref["qdd"])[ok] / (1 + np.abs(ref["qdd"][ok]))
    dt = np.abs(out["tau"] - ref["tau"])[ok] / (1 + np.abs(ref["tau"][ok]))
    print("qdd / tau vs oracle", dq.max(initial=0.0), dt.max(initial=0.0))
    assert dq.max(initial=0.0) <= 1e-6 and dt.max(initial=0.0) <= 1e-6


def test_dual_arm_control_targets_and_instances():
    from dart_mpc.arm import ArmDynamics, DualArmControl
    from scipy.spatial.transform import Rotation as Rot
    xr, lim = _xarm()
    rng = np.random.default_rng(61)
    E = 3
    prm = arm_qp.default_params()
    pos = rng.uniform(-0.3, 0.3, (E, 3)) + [0, 0, 0.4]
    quat = Rot.from_euler("xyz", rng.uniform(-0.5, 0.5, (E, 3))).as_quat(scalar_first=True) * rng.choice([-1, 1], (E, 1))
    q = HOME + rng.uniform(-0.2, 0.2, (E, 2, 7))
    qd = rng.uniform(-0.5, 0.5, (E, 2, 7))
    ctl = DualArmControl(xr[0], xr[1], prm, prm, n=7)
    tau, loss = ctl.control(pos, quat, q, qd)
    for e in range(E):
        for a, (tp, tq) in enumerate(R.resolve_ee_targets(pos[e], quat[e])):
            mp, mq = ctl.last_mocap[e, a, :3], ctl.last_mocap[e, a, 3:]
            assert np.max(np.abs(mp - tp)) <= 1e-14
            assert min(np.max(np.abs(mq - tq)), np.max(np.abs(mq + tq))) <= 1e-14
    from dart_mpc.arm import pack_params
    for a in range(2):
        dyn = ArmDynamics(xr[a], 7)
        S = dyn.pack_state(q[:, a], qd[:, a], np.zeros((E, 7)), ctl.last_mocap[:, a, :3], ctl.last_mocap[:, a, 3:])
        one = dyn.control_batch(S, pack_params(prm))
        assert np.array_equal(one["tau"], tau[:, a]) and np.array_equal(one["loss"], loss[:, a])
        assert np.array_equal(one["qdd"], ctl.qdd_prev[:, a]) and np.array_equal(one["status"], ctl.last_status[:, a])
    # ArmControl.compute_torque_from_state: the single-arm call, qdd_prev kept
    from dart_mpc.arm import ArmControl
    ac, dyn = ArmControl(prm, 7), ArmDynamics(xr[1], 7)
    t1, l1 = ac.compute_torque_from_state(dyn, q[0, 1], qd[0, 1], ctl.last_mocap[0, 1, :3], ctl.last_mocap[0, 1, 3:])
    assert np.array_equal(t1, tau[0, 1]) and l1 == loss[0, 1] and np.array_equal(ac.qdd_prev, ctl.qdd_prev[0, 1])
    assert ac.last_status == ctl.last_status[0, 1]
    # the unbatched form and the kept qdd_prev
    c1 = DualArmControl(xr[0], xr[1], prm, prm, n=7)
    (tl, tr), (ll, lr) = c1.control(pos[0], quat[0], q[0], qd[0])
    assert np.array_equal(tl, tau[0, 0]) and np.array_equal(tr, tau[0, 1]) and (ll, lr) == (loss[0, 0], loss[0, 1])
    assert np.array_equal(c1.qdd_prev[0], ctl.qdd_prev[0])


# ---- the device-resident loop -------------------------------------------------------------------------------------
E_ROLL, K_ROLL = 2, 20


def _roll_inputs():
    from dart_mpc.harness import tray_poses_from_tilt
    xr, _ = _xarm()
    rng = np.random.default_rng(71)
    q0 = HOME + rng.uniform(-0.05, 0.05, (E_ROLL, 2, 7))
    qd0 = rng.uniform(-0.05, 0.05, (E_ROLL, 2, 7))
    u = 0.1 * np.sin(np.arange(K_ROLL)[:, None, None] * 0.3 + np.arange(E_ROLL)[None, :, None] + np.array([0.0, 1.0]))
    tray = tray_poses_from_tilt(u, [[0.0, 0.0, 0.4], [0.02, -0.01, 0.42]])
    return xr, q0, qd0, tray, arm_qp.default_params()


@functools.lru_cache(maxsize=None)
def _roll_reference():
    """The numpy loop, and its sensitivity to a perturbation of every snapshot by the snapshot bars (CPU only)."""
    xr, q0, qd0, tray, prm = _roll_inputs()
    nom = R.rollout_dual_arm(arm_qp.solve_arm, q0, qd0, tray, xr, prm, K_ROLL)
    # the snapshot bars on the loop's own states: the two formulations at every logged state
    S = np.concatenate([nom["logs"]["q"].reshape(-1, 7), nom["logs"]["qd"].reshape(-1, 7),
                        np.zeros((K_ROLL * 2 * E_ROLL, 7 + 3)), np.tile(IDENT, (K_ROLL * 2 * E_ROLL, 1))], axis=1)
    bars = _bars(*[R.snapshot_batch(xr[0], 7, S[::4], form=f) for f in ("jac", "rec")])
    rng = np.random.default_rng(72)

    def perturb(k, snap):
        for key, bar in bars.items():
            snap[key] = snap[key] + bar * (1 + np.abs(snap[key])) * rng.choice([-1.0, 1.0], np.shape(snap[key]))
    per = R.rollout_dual_arm(arm_qp.solve_arm, q0, qd0, tray, xr, prm, K_ROLL, perturb=perturb)
    sens = {k: float(np.max(np.abs(per["logs"][k] - nom["logs"][k]) / (1 + np.abs(nom["logs"][k]))))
            for k in ("q", "qd", "tau", "ee_pos", "loss")}
    return nom, sens, bars


@functools.lru_cache(maxsize=None)
def _roll_gpu():
    from dart_mpc.harness import rollout_dual_arm
    xr, q0, qd0, tray, prm = _roll_inputs()
    return rollout_dual_arm(q0, qd0, tray, xr, prm, K_ROLL)


def test_rollout_logs_against_the_numpy_loop():
    """E = 2, K = 20.  Margin per log: 4 x the numpy loop's own response to perturbing every snapshot by the snapshot
    bars (floor: the bar itself), relative to 1 + |.|; statuses equal."""
    nom, sens, bars = _roll_reference()
    res = _roll_gpu()
    print("numpy loop sensitivity to the snapshot bars:", sens)
    assert np.array_equal(res["logs"]["status"], nom["logs"]["status"])
    print("statuses in the loop", np.unique(nom["logs"]["status"], return_counts=True))
    for k, s in sens.items():
        d = float(np.max(np.abs(res["logs"][k] - nom["logs"][k]) / (1 + np.abs(nom["logs"][k]))))
        margin = max(4.0 * s, FLOOR)
        print(f"log {k}: device vs numpy {d:.2e}, margin {margin:.2e}")
        assert d <= margin, (k, d, margin)
    dm = np.abs(res["metrics"] - nom["metrics"]) / (1 + np.abs(nom["metrics"]))
    assert np.array_equal(res["metrics"][:, 3], nom["metrics"][:, 3])       # (iteration counts may differ by rounding)
    assert dm[:, [0, 1, 2, 5]].max() <= max(4.0 * max(sens.values()), FLOOR)


def test_rollout_metrics_only_and_chaining():
    from dart_mpc.harness import rollout_dual_arm
    xr, q0, qd0, tray, prm = _roll_inputs()
    full = _roll_gpu()
    mo = rollout_dual_arm(q0, qd0, tray, xr, prm, K_ROLL, metrics_only=True)
    assert mo["logs"] is None and np.array_equal(mo["metrics"], full["metrics"])
    for k in ("q", "qd", "qdd_prev"):
        assert np.array_equal(mo[k], full[k])
    a = rollout_dual_arm(q0, qd0, tray[:10], xr, prm, 10)
    b = rollout_dual_arm(a["q"], a["qd"], tray[10:], xr, prm, 10, qdd_prev0=a["qdd_prev"], metrics0=a["metrics"])
    for k in ("q", "qd", "qdd_prev", "metrics"):
        assert np.array_equal(b[k], full[k]), k
    for k, v in full["logs"].items():
        assert np.array_equal(np.concatenate([a["logs"][k], b["logs"][k]]), v), k
    # a held pose: one row
    h1 = rollout_dual_arm(q0, qd0, tray[:1], xr, prm, 5, metrics_only=True)
    h5 = rollout_dual_arm(q0, qd0, np.repeat(tray[:1], 5, axis=0), xr, prm, 5, metrics_only=True)
    assert np.array_equal(h1["q"], h5["q"]) and np.array_equal(h1["metrics"], h5["metrics"])


def test_rollout_payload_plant_differs():
    from dart_mpc.arm_model import ArmModel
    from dart_mpc.harness import rollout_dual_arm
    xr, q0, qd0, tray, prm = _roll_inputs()
    heavy = [ArmModel.from_row(r, 7).with_payload(1.0) for r in xr]
    res = rollout_dual_arm(q0, qd0, tray, xr, prm, K_ROLL, plant_models=heavy)
    full = _roll_gpu()
    assert np.all(np.isfinite(res["q"]))
    assert np.max(np.abs(res["q"] - full["q"])) > 1e-6
    assert np.array_equal(res["logs"]["q"][0], full["logs"]["q"][0])        # the first step sees the same state
