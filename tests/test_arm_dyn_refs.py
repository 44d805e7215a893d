"""The CPU references of the arm dynamics (tests/arm_dyn_refs.py) against each other, against finite differences and
against closed forms; no GPU.  The two formulations' largest difference (printed) is what the GPU bars of
tests/test_gpu_arm_dyn.py are built on."""
import os

import numpy as np
import pytest

import arm_dyn_refs as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "xarm7_arm_models.npz")


def _states(rng, n, count, limits=None):
    lo, hi = (-np.pi * np.ones(n), np.pi * np.ones(n)) if limits is None else (limits[:, 0], limits[:, 1])
    for _ in range(count):
        v = rng.standard_normal(4)
        yield np.concatenate([rng.uniform(lo, hi), rng.uniform(-2, 2, n), rng.uniform(-5, 5, n), rng.uniform(-1, 1, 3),
                              v / np.linalg.norm(v)])


def _cases():
    g = np.load(GOLD)
    rng = np.random.default_rng(11)
    cases = [("xarm7", g["rows"][0], 7, g["limits"][0], 100), ("xarm7R", g["rows"][1], 7, g["limits"][1], 100)]
    cases += [(f"random{n}", R.random_model(rng, n), n, None, 25) for n in range(1, 9)]
    return cases


def test_two_formulations_agree():
    """200 states of the xArm7 fixture and 200 of random chains with n = 1..8, both jacDot modes."""
    rng = np.random.default_rng(3)
    worst = {}
    for name, row, n, lim, count in _cases():
        for i, s in enumerate(_states(rng, n, count, lim)):
            mode = i % 2
            a = R.snapshot_batch(row, n, s[None], mode, "jac")
            b = R.snapshot_batch(row, n, s[None], mode, "rec")
            for k, v in R.form_difference(a, b).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("largest relative difference between the two CPU formulations:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-11, worst


@pytest.mark.parametrize("mode", [R.JACDOT_REFERENCE, R.JACDOT_BODY])
def test_jac_and_jacdot_against_central_differences(mode):
    """jac qd = d/dt of the EE origin; jacDot = d/de J(q + e qd) of the mode's own point, e = 1e-6: truncation e^2,
    rounding eps / e = 2e-10, against 1e-7 (1 + |.|)."""
    eps = 1e-6
    rng = np.random.default_rng(5)
    for name, row, n, lim, _ in _cases():
        m = R.unpack(row, n)
        for s in _states(rng, n, 4, lim):
            q, qd = s[:n], s[n:2 * n]
            snap = R.snapshot(row, n, q, qd, s[2 * n:3 * n], s[3 * n:3 * n + 3], s[3 * n + 3:], mode, "rec")
            Rs, ps, Re, pe = R.frames_mat(m, q)
            pt = pe if mode == R.JACDOT_BODY else np.array([0.0, 0.0, m["offset"]])
            rb = Re.T @ (pt - pe)                    # the point in the EE body's frame

            def J_at(qq):
                R2, p2, Re2, pe2 = R.frames_mat(m, qq)
                z2, _, _ = R._geometry(m, R2, p2)
                return R.point_jac(z2, p2, pe2 + Re2 @ rb, n - 1), pe2
            Jp, pp = J_at(q + eps * qd)
            Jm, pm = J_at(q - eps * qd)
            v_fd = (pp - pm) / (2 * eps)
            v = snap["jac"][:3] @ qd
            assert np.all(np.abs(v - v_fd) <= 1e-7 * (1 + np.abs(v_fd))), name
            Jd_fd = (Jp - Jm) / (2 * eps)
            assert np.all(np.abs(snap["jacDot"] - Jd_fd) <= 1e-7 * (1 + np.abs(Jd_fd))), (name, mode)


def test_mdot_minus_2c_is_skew():
    rng = np.random.default_rng(6)
    for name, row, n, lim, _ in _cases():
        m = R.unpack(row, n)
        for s in _states(rng, n, 4, lim):
            q, qd = s[:n], s[n:2 * n]
            Rs, ps, _, _ = R.frames_mat(m, q)
            z, pc, Iw = R._geometry(m, Rs, ps)
            _, dM = R.mass_matrix_jac(m, z, ps, pc, Iw, with_grad=True)
            Md = np.einsum("lij,l->ij", dM, qd)
            C = R.coriolis_matrix(dM, qd)
            val = qd @ (Md - 2 * C) @ qd
            assert abs(val) <= 1e-7 * (1 + abs(qd @ Md @ qd)), name
            # and dM itself against central differences of M
            l = int(rng.integers(n))
            e = np.zeros(n); e[l] = 1e-6
            Ms = []
            for qq in (q + e, q - e):
                R2, p2, _, _ = R.frames_mat(m, qq)
                Ms.append(R.mass_matrix_jac(m, *((R._geometry(m, R2, p2)[0], p2) + R._geometry(m, R2, p2)[1:])))
            fd = (Ms[0] - Ms[1]) / 2e-6
            assert np.all(np.abs(dM[l] - fd) <= 1e-7 * (1 + np.abs(fd))), name


def pendulum_row(mass=1.3, d=0.4, Iax=0.02, arm=0.1):
    """One hinge about world y at the origin, com at distance d along the link's -z at q = 0 (hanging)."""
    link = [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, arm, 0.7, mass, 0, 0, -d, 0.01, Iax, 0.03, 0, 0, 0]
    return np.array([0, 0, 0, 1, 0, 0, 0] + link + [0, 0, -2 * d, 1, 0, 0, 0, 0.05, 0, 0, -9.81], dtype=float)


def planar_2r_row(m1=1.1, m2=0.7, l1=0.5, r1=0.2, r2=0.3, I1=0.03, I2=0.02, arm=0.0):
    """Planar 2R in the world x-y plane about z, gravity along -y: the textbook arm."""
    k1 = [0, 0, 0, 1, 0, 0, 0, 0, 0, 1, arm, 0.3, m1, r1, 0, 0, 0.001, 0.002, I1, 0, 0, 0]
    k2 = [l1, 0, 0, 1, 0, 0, 0, 0, 0, 1, arm, 0.2, m2, r2, 0, 0, 0.001, 0.002, I2, 0, 0, 0]
    return np.array([0, 0, 0, 1, 0, 0, 0] + k1 + k2 + [0.4, 0, 0, 1, 0, 0, 0, 0.0, 0, -9.81, 0], dtype=float)


def pendulum_exact(q, mass=1.3, d=0.4, Iax=0.02, arm=0.1):
    return Iax + mass * d * d + arm, mass * 9.81 * d * np.sin(q)


def planar_2r_exact(q, qd, m1=1.1, m2=0.7, l1=0.5, r1=0.2, r2=0.3, I1=0.03, I2=0.02, arm=0.0, g=9.81):
    c2, s2 = np.cos(q[1]), np.sin(q[1])
    M = np.array([[I1 + I2 + m1 * r1 ** 2 + m2 * (l1 ** 2 + r2 ** 2 + 2 * l1 * r2 * c2), I2 + m2 * (r2 ** 2 + l1 * r2 * c2)],
                  [I2 + m2 * (r2 ** 2 + l1 * r2 * c2), I2 + m2 * r2 ** 2]]) + arm * np.eye(2)
    hh = m2 * l1 * r2 * s2
    c = np.array([-hh * (2 * qd[0] * qd[1] + qd[1] ** 2), hh * qd[0] ** 2])
    grav = np.array([(m1 * r1 + m2 * l1) * g * np.cos(q[0]) + m2 * r2 * g * np.cos(q[0] + q[1]),
                     m2 * r2 * g * np.cos(q[0] + q[1])])
    return M, c + grav


@pytest.mark.parametrize("form", ["jac", "rec"])
def test_closed_forms(form):
    rng = np.random.default_rng(8)
    ident = [1.0, 0, 0, 0]
    for _ in range(10):
        q, qd = rng.uniform(-3, 3, 1), rng.uniform(-2, 2, 1)
        s = R.snapshot(pendulum_row(), 1, q, qd, [0.0], np.zeros(3), ident, form=form)
        M, h = pendulum_exact(q[0])
        assert abs(s["M"][0, 0] - M) <= 1e-12 * (1 + abs(M)) and abs(s["h"][0] - h) <= 1e-12 * (1 + abs(h))
        q, qd = rng.uniform(-3, 3, 2), rng.uniform(-2, 2, 2)
        s = R.snapshot(planar_2r_row(), 2, q, qd, np.zeros(2), np.zeros(3), ident, form=form)
        M, h = planar_2r_exact(q, qd)
        assert np.all(np.abs(s["M"] - M) <= 1e-12 * (1 + np.abs(M)))
        assert np.all(np.abs(s["h"] - h) <= 1e-12 * (1 + np.abs(h)))
