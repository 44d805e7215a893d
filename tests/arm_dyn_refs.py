"""CPU references for the arm dynamics kernel (csrc/arm_dyn.hip) -- TEST INFRASTRUCTURE ONLY, numpy, never imported by
the product.  Every snapshot field of ARMCONTROL.compute_dynamics by two formulations that differ from each other and
from the kernel's:

``form="jac"``  through per-link com Jacobians: M = sum_k (m_k Jv_k' Jv_k + Jw_k' I_k Jw_k) + armature, gravity
                -sum_k m_k Jv_k' g, Coriolis from the Christoffel symbols of M with analytic dM/dq, jacDot as
                sum_l dJ/dq_l qd_l, frames by rotation matrices, Mx_inv by numpy.linalg.solve.
``form="rec"``  recursive: frames by a quaternion chain, h by recursive Newton-Euler (forces passed link to link), M by the
                composite-rigid-body recursion (composites accumulated tip to base about the world origin), jacDot
                from link velocities, Mx_inv by scipy's Cholesky solve.

Also the numpy dual-arm closed loop of ``dart_dual_arm_rollout`` on oracle/arm_qp.solve_arm.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.spatial.transform import Rotation as Rot

JACDOT_REFERENCE, JACDOT_BODY = 0, 1
DACTL_GRASP = np.array([[-0.175, 0, 0, 0.5, 0.5, 0.5, 0.5], [0.175, 0, 0, 0.5, -0.5, -0.5, 0.5]])


def unpack(row, n):
    row = np.asarray(row, dtype=float)
    assert row.shape == (22 * n + 18,)
    L = row[7:7 + 22 * n].reshape(n, 22)
    e = row[7 + 22 * n:]
    return dict(n=n, base_pos=row[:3], base_quat=row[3:7], pos=L[:, :3], quat=L[:, 3:7], axis=L[:, 7:10],
                armature=L[:, 10], damping=L[:, 11], mass=L[:, 12], com=L[:, 13:16], inertia=L[:, 16:22],
                ee_pos=e[:3], ee_quat=e[3:7], offset=e[7], gravity=e[8:11])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def qmat(q):
    return Rot.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def sym6(v):
    return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])


def random_model(rng, n, offset=0.1):
    """A random chain: link offsets and coms of a few decimetres, SPD inertias, armature 0.05..0.2."""
    def uq():
        v = rng.standard_normal(4)
        return v / np.linalg.norm(v)
    links = []
    for _ in range(n):
        ax = rng.standard_normal(3)
        A = rng.standard_normal((3, 3)) * 0.05
        I = A @ A.T + 1e-3 * np.eye(3)
        links.append(np.concatenate([rng.uniform(-0.3, 0.3, 3), uq(), ax / np.linalg.norm(ax), [rng.uniform(0.05, 0.2)],
                                     [rng.uniform(0.5, 5.0)], [rng.uniform(0.2, 3.0)], rng.uniform(-0.1, 0.1, 3),
                                     [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]]))
    return np.concatenate([rng.uniform(-0.5, 0.5, 3), uq(), np.concatenate(links), rng.uniform(-0.1, 0.1, 3), uq(),
                           [offset], [0.0, 0.0, -9.81]])


# ---- frames -------------------------------------------------------------------------------------------------------
def frames_mat(m, q):
    """World frames by rotation matrices: R [n], p [n], (Re, pe)."""
    R, p = qmat(m["base_quat"]), m["base_pos"].copy()
    Rs, ps = [], []
    for i in range(m["n"]):
        p = p + R @ m["pos"][i]
        R = R @ qmat(m["quat"][i]) @ Rot.from_rotvec(m["axis"][i] * q[i]).as_matrix()
        Rs.append(R); ps.append(p.copy())
    return np.array(Rs), np.array(ps), R @ qmat(m["ee_quat"]), p + R @ m["ee_pos"]


def frames_quat(m, q):
    """The same by a quaternion chain; also the EE quaternion."""
    Q, p = m["base_quat"].copy(), m["base_pos"].copy()
    Rs, ps = [], []
    for i in range(m["n"]):
        p = p + qmat(Q) @ m["pos"][i]
        Q = qmul(qmul(Q, m["quat"][i]), np.concatenate([[np.cos(q[i] / 2)], np.sin(q[i] / 2) * m["axis"][i]]))
        Rs.append(qmat(Q)); ps.append(p.copy())
    Qe = qmul(Q, m["ee_quat"])
    return np.array(Rs), np.array(ps), qmat(Qe), p + qmat(Q) @ m["ee_pos"], Qe


def _geometry(m, R, p):
    n = m["n"]
    z = np.array([R[i] @ m["axis"][i] for i in range(n)])
    pc = np.array([p[i] + R[i] @ m["com"][i] for i in range(n)])
    Iw = np.array([R[i] @ sym6(m["inertia"][i]) @ R[i].T for i in range(n)])
    return z, pc, Iw


def point_jac(z, p, pt, upto):
    """[Jv; Jw] of a point attached to link ``upto``."""
    n = len(z)
    J = np.zeros((6, n))
    for i in range(upto + 1):
        J[:3, i] = np.cross(z[i], pt - p[i])
        J[3:, i] = z[i]
    return J


# ---- formulation "jac" -------------------------------------------------------------------------------------------------
def _dgeom(z, p, pc, Iw, l):
    """d/dq_l of z_i, p_i, pc_k, Iw_k."""
    n = len(z)
    dz = np.array([np.cross(z[l], z[i]) if l < i else np.zeros(3) for i in range(n)])
    dp = np.array([np.cross(z[l], p[i] - p[l]) if l < i else np.zeros(3) for i in range(n)])
    dpc = np.array([np.cross(z[l], pc[k] - p[l]) if l <= k else np.zeros(3) for k in range(n)])
    S = skew(z[l])
    dI = np.array([S @ Iw[k] - Iw[k] @ S if l <= k else np.zeros((3, 3)) for k in range(n)])
    return dz, dp, dpc, dI


def mass_matrix_jac(m, z, p, pc, Iw, with_grad=False):
    n = m["n"]
    M = np.diag(m["armature"]).astype(float)
    dM = np.zeros((n, n, n))            # dM[l] = dM / dq_l
    dg = [_dgeom(z, p, pc, Iw, l) for l in range(n)] if with_grad else None
    for k in range(n):
        J = point_jac(z, p, pc[k], k)
        M += m["mass"][k] * J[:3].T @ J[:3] + J[3:].T @ Iw[k] @ J[3:]
        if with_grad:
            for l in range(n):
                dz, dp, dpc, dI = dg[l]
                dJ = np.zeros((6, n))
                for i in range(k + 1):
                    dJ[:3, i] = np.cross(dz[i], pc[k] - p[i]) + np.cross(z[i], dpc[k] - dp[i])
                    dJ[3:, i] = dz[i]
                A = m["mass"][k] * dJ[:3].T @ J[:3] + dJ[3:].T @ Iw[k] @ J[3:]
                dM[l] += A + A.T + J[3:].T @ dI[k] @ J[3:]
    return (M, dM) if with_grad else M


def coriolis_matrix(dM, qd):
    """C_ij = sum_k Gamma_ijk qd_k, Gamma_ijk = (dM_ij/dq_k + dM_ik/dq_j - dM_jk/dq_i) / 2."""
    G = 0.5 * (np.einsum("kij->ijk", dM) + np.einsum("jik->ijk", dM) - np.einsum("ijk->ijk", dM))
    return np.einsum("ijk,k->ij", G, qd)


def bias_jac(m, z, p, pc, dM, qd):
    g = np.zeros(m["n"])
    for k in range(m["n"]):
        g -= m["mass"][k] * point_jac(z, p, pc[k], k)[:3].T @ m["gravity"]
    return coriolis_matrix(dM, qd) @ qd + g


def jacdot_jac(z, p, pc, Iw, pt, qd):
    """sum_l dJ/dq_l qd_l of a point attached to the last link."""
    n = len(z)
    Jd = np.zeros((6, n))
    for l in range(n):
        dz, dp, _, _ = _dgeom(z, p, pc, Iw, l)
        dpt = np.cross(z[l], pt - p[l])
        for i in range(n):
            Jd[:3, i] += qd[l] * (np.cross(dz[i], pt - p[i]) + np.cross(z[i], dpt - dp[i]))
            Jd[3:, i] += qd[l] * dz[i]
    return Jd


# ---- formulation "rec" -------------------------------------------------------------------------------------------------
def velocities(z, p, qd):
    n = len(z)
    w, v = np.zeros((n, 3)), np.zeros((n, 3))
    wp, vp, pp = np.zeros(3), np.zeros(3), p[0]
    for i in range(n):
        v[i] = vp + np.cross(wp, p[i] - pp)
        w[i] = wp + z[i] * qd[i]
        wp, vp, pp = w[i], v[i], p[i]
    return w, v


def bias_rnea(m, z, p, pc, Iw, qd):
    """Recursive Newton-Euler at qdd = 0, base accelerated by -gravity; forces passed tip to base."""
    n = m["n"]
    w, _ = velocities(z, p, qd)
    al, a = np.zeros((n, 3)), np.zeros((n, 3))
    wp, alp, ap, pp = np.zeros(3), np.zeros(3), -m["gravity"], p[0]
    for i in range(n):
        r = p[i] - pp
        a[i] = ap + np.cross(alp, r) + np.cross(wp, np.cross(wp, r))
        al[i] = alp + np.cross(wp, z[i] * qd[i])
        wp, alp, ap, pp = w[i], al[i], a[i], p[i]
    f, t = np.zeros(3), np.zeros(3)        # force and moment (about p[i + 1]) the link passes down
    h = np.zeros(n)
    for i in reversed(range(n)):
        c = pc[i] - p[i]
        F = m["mass"][i] * (a[i] + np.cross(al[i], c) + np.cross(w[i], np.cross(w[i], c)))
        N = Iw[i] @ al[i] + np.cross(w[i], Iw[i] @ w[i])
        if i + 1 < n:
            t = t + np.cross(p[i + 1] - p[i], f)
        t = t + N + np.cross(c, F)
        f = f + F
        h[i] = z[i] @ t
    return h


def mass_matrix_crba(m, z, p, pc, Iw):
    """Composite rigid bodies accumulated tip to base as (mass, first moment, inertia about the world origin)."""
    n = m["n"]
    M = np.zeros((n, n))
    mc, s, I0 = 0.0, np.zeros(3), np.zeros((3, 3))
    for i in reversed(range(n)):
        mk, c = m["mass"][i], pc[i]
        mc += mk
        s = s + mk * c
        I0 = I0 + Iw[i] + mk * ((c @ c) * np.eye(3) - np.outer(c, c))
        # unit acceleration of joint i: the composite turns about the axis through p[i]
        # force F = z_i x s - mc z_i x p_i, moment about the origin n0 = I0 z_i - s x (z_i x p_i)
        F = np.cross(z[i], s) - mc * np.cross(z[i], p[i])
        n0 = I0 @ z[i] - np.cross(s, np.cross(z[i], p[i]))
        for j in range(i + 1):
            M[i, j] = M[j, i] = z[j] @ (n0 - np.cross(p[j], F))
        M[i, i] += m["armature"][i]
    return M


def jacdot_vel(z, p, w, v, pt, vpt):
    n = len(z)
    Jd = np.zeros((6, n))
    for i in range(n):
        zd = np.cross(w[i], z[i])
        Jd[:3, i] = np.cross(zd, pt - p[i]) + np.cross(z[i], vpt - v[i])
        Jd[3:, i] = zd
    return Jd


# ---- the snapshot ----------------------------------------------------------------------------------------------------
def rotvec_error(mocap_quat, ee_quat):
    e = qmul(np.asarray(mocap_quat, dtype=float), np.array([ee_quat[0], -ee_quat[1], -ee_quat[2], -ee_quat[3]]))
    return Rot.from_quat([e[1], e[2], e[3], e[0]]).as_rotvec()


def snapshot(row, n, q, qd, qdd_prev, mocap_pos, mocap_quat, jacdot_point=JACDOT_REFERENCE, form="jac"):
    """The dict ``dart_mpc.arm.pack_snapshot`` takes, plus ee_quat (w, x, y, z; sign as the formulation gives it)."""
    m = unpack(row, n)
    q, qd = np.asarray(q, dtype=float), np.asarray(qd, dtype=float)
    if form == "jac":
        R, p, Re, pe = frames_mat(m, q)
        xyzw = Rot.from_matrix(Re).as_quat()
        Qe = np.array([xyzw[3], xyzw[0], xyzw[1], xyzw[2]])
    else:
        R, p, Re, pe, Qe = frames_quat(m, q)
    z, pc, Iw = _geometry(m, R, p)
    J = point_jac(z, p, pe, n - 1)
    pt = pe if jacdot_point == JACDOT_BODY else np.array([0.0, 0.0, m["offset"]])
    if form == "jac":
        M, dM = mass_matrix_jac(m, z, p, pc, Iw, with_grad=True)
        h = bias_jac(m, z, p, pc, dM, qd)
        Jd = jacdot_jac(z, p, pc, Iw, pt, qd)
        Mx_inv = J @ np.linalg.solve(M, J.T)
    else:
        M = mass_matrix_crba(m, z, p, pc, Iw)
        h = bias_rnea(m, z, p, pc, Iw, qd)
        w, v = velocities(z, p, qd)
        ve = v[-1] + np.cross(w[-1], pe - p[-1])
        Jd = jacdot_vel(z, p, w, v, pt, ve + np.cross(w[-1], pt - pe))
        Mx_inv = J @ cho_solve(cho_factor(M), J.T)
    return {"q": q, "qd": qd, "qdd_prev": np.asarray(qdd_prev, dtype=float), "mocap_pos": np.asarray(mocap_pos, dtype=float),
            "ee_pos": pe + m["offset"] * Re[:, 2], "rotvec": rotvec_error(mocap_quat, Qe), "jac": J, "jacDot": Jd,
            "M": M, "h": h, "Mx_inv": Mx_inv, "ee_quat": Qe}


SNAP_KEYS = ("q", "qd", "qdd_prev", "mocap_pos", "ee_pos", "rotvec", "jac", "jacDot", "M", "h", "Mx_inv")


def snapshot_batch(rows, n, state, jacdot_point=JACDOT_REFERENCE, form="jac"):
    """state [B, 3 n + 7] rows; rows [22 n + 18] shared or [B, .]: dict of stacked fields."""
    rows = np.asarray(rows)
    outs = [snapshot(rows if rows.ndim == 1 else rows[b], n, s[:n], s[n:2 * n], s[2 * n:3 * n], s[3 * n:3 * n + 3],
                     s[3 * n + 3:], jacdot_point, form) for b, s in enumerate(np.asarray(state))]
    return {k: np.stack([o[k] for o in outs]) for k in SNAP_KEYS + ("ee_quat",)}


def form_difference(a, b):
    """Largest |a - b| / (1 + |b|) per field between two snapshot dicts (ee_quat aside: its sign is free)."""
    return {k: float(np.max(np.abs(a[k] - b[k]) / (1.0 + np.abs(b[k])))) for k in SNAP_KEYS}


# ---- the dual-arm coordinator and the closed loop ---------------------------------------------------------------------
def resolve_ee_targets(tray_pos, tray_quat, grasp=DACTL_GRASP):
    """DACTL._resolve_ee_pos (dualctl.py:22-56) restated with scipy: [(pos, quat wxyz)] for the two arms."""
    Rw = Rot.from_quat(tray_quat, scalar_first=True).as_matrix()
    out = []
    for g in grasp:
        Rg = Rot.from_quat(g[3:], scalar_first=True).as_matrix()
        out.append((np.asarray(tray_pos) + Rw @ g[:3], Rot.from_matrix(Rw @ Rg).as_quat(scalar_first=True)))
    return out


def plant_step(row, n, q, qd, tau, dt, form="rec"):
    m = unpack(row, n)
    R, p, _, _ = frames_mat(m, q)
    z, pc, Iw = _geometry(m, R, p)
    M = mass_matrix_crba(m, z, p, pc, Iw)
    h = bias_rnea(m, z, p, pc, Iw, qd)
    d = m["damping"]
    a = np.linalg.solve(M + dt * np.diag(d), tau - h - d * qd)
    qd1 = qd + dt * a
    return q + dt * qd1, qd1


def rollout_dual_arm(solve_arm, q0, qd0, tray_poses, rows, prm, steps, plant_rows=None, jacdot_point=JACDOT_REFERENCE,
                     grasp=DACTL_GRASP, qdd_prev0=None, perturb=None):
    """The numpy loop of dart_dual_arm_rollout: q0, qd0 [E, 2, n]; tray_poses [K or 1, E, 7]; rows [2, .]; prm one
    parameter dict.  ``perturb(k, snap)`` may alter a step's snapshot in place (sensitivity measurements)."""
    q, qd = np.array(q0, dtype=float), np.array(qd0, dtype=float)
    E, _, n = q.shape
    plant_rows = rows if plant_rows is None else plant_rows
    qp = np.zeros_like(q) if qdd_prev0 is None else np.array(qdd_prev0, dtype=float)
    dt = prm["dt"]
    logs = {k: np.zeros((steps, 2 * E) + s) for k, s in (("q", (n,)), ("qd", (n,)), ("tau", (n,)), ("ee_pos", (3,)),
                                                          ("loss", ()))}
    logs["status"] = np.zeros((steps, 2 * E), dtype=np.int32)
    metrics = np.zeros((2 * E, 6))
    for k in range(steps):
        tp = tray_poses[0 if len(tray_poses) == 1 else k]
        for e in range(E):
            targets = resolve_ee_targets(tp[e, :3], tp[e, 3:], grasp)
            for a in range(2):
                b = 2 * e + a
                s = snapshot(rows[a], n, q[e, a], qd[e, a], qp[e, a], targets[a][0], targets[a][1], jacdot_point, "rec")
                s.pop("ee_quat")
                if perturb is not None:
                    perturb(k, s)
                r = solve_arm(s, prm)
                st = int(r["status"])
                tau = r["tau"] if st >= 0 else np.zeros(n)
                logs["q"][k, b], logs["qd"][k, b], logs["tau"][k, b] = q[e, a], qd[e, a], tau
                logs["ee_pos"][k, b], logs["loss"][k, b], logs["status"][k, b] = s["ee_pos"], r["loss"], st
                err = float(np.linalg.norm(s["ee_pos"] - s["mocap_pos"]))
                mt = metrics[b]
                mt[0], mt[1], mt[2] = err, max(mt[1], err), float(np.linalg.norm(s["rotvec"]))
                mt[3] += st != 0
                mt[4] += int(r["iters"])
                mt[5] = max(mt[5], float(np.max(np.abs(tau) / prm["taumax"])))
                q[e, a], qd[e, a] = plant_step(plant_rows[a], n, q[e, a], qd[e, a], tau, dt)
                if st >= 0:
                    qp[e, a] = r["qdd"]
    return {"q": q, "qd": qd, "qdd_prev": qp, "metrics": metrics, "logs": logs}
