"""Inputs and exact references of the device tests of csrc/arm_qp.hip (tests/test_gpu_arm_edges.py, through the
fixture tests/golden/arm_edge_goldens.npz) and their host-only checks (tests/test_arm_refs.py).

TEST INFRASTRUCTURE ONLY.  It imports mpmath, which a GPU machine need not have: no test marked ``gpu`` imports this
module; the exact answers travel in the fixture (tests/golden/make_arm_edge_goldens.py writes it from here).

Nothing here shares code with the kernel.  ``build_exact`` evaluates the formulas of PMPC/src/controller/arm.py:335-388
in mpmath (50 digits) from ONE symmetric eigen-decomposition per matrix, with the reference's cutoffs decided in exact
arithmetic, and takes the |.|-square root of Mx from the same decomposition: sqrt of the kept weights, exactly 0 for
the dropped ones.  oracle/arm_qp.py follows the reference literally and takes a second ``eigh`` of the computed Mx;
on the pinv branch the dropped eigenvalues come back from it as ~1e-17 noise whose square root is ~3e-9, so the
oracle's D is ~1e-8 relative away from the exact one there (tests/test_arm_refs.py pins that).
"""
from __future__ import annotations

import numpy as np

import arm_qp

N_TASK = 6
EPS = 2.0 ** -52
ABSENT = 1e20                       # a bound the kernel and IPOPT both treat as absent (|.| >= 1e19)
BOUND_GROUPS = (("Qmin", "Qmax"), ("Qdotmin", "Qdotmax"), ("taumin", "taumax"))
TAUMAX7 = np.array([50.0, 50, 30, 30, 30, 20, 20])

# spectra of the classes: M (n x n, by joint count) and Mx_inv (6 x 6)
M_SPECS = {
    "m_well": lambda n: np.linspace(0.5, 3.0, n) if n > 1 else np.array([1.5]),
    "m_equal": lambda n: np.full(n, 2.0),
    "m_pairs": lambda n: np.array([1.0, 1, 2, 2, 5, 5, 9, 9])[:n],
    "m_graded": lambda n: np.logspace(-3, 0, n),
    "m_diag": lambda n: np.linspace(0.5, 3.0, n) if n > 1 else np.array([1.5]),
    "m_trunc": lambda n: np.concatenate([np.linspace(1.0, 3.0, n - 1), [9e-8]]),      # 3e-8 lmax: pinv(M) truncates
}
M_MIN_N = {"m_pairs": 2, "m_graded": 2, "m_trunc": 2}
X_SPECS = {
    "x_inv_well": [0.5, 1, 2, 3, 4, 5],
    "x_inv_small": [50, 60, 70, 80, 90, 0.02],          # 2.2e-4 lmax on the inv path: kept
    "x_inv_indef": [0.5, -1, 2, -3, 4, 5],
    "x_pinv_drop2": [3, 2, 1, 0.5, 1e-5, 1e-6],
    "x_pinv_rank3": [3, 2, 1, 0, 0, 0],
    "x_pinv_keepall": [0.02, 0.015, 0.025, 0.03, 0.01, 0.02],   # |det| = 4.5e-11, nothing below 1e-3 lmax
    "x_pinv_near_cutoff": [3, 2, 1, 9e-3, 9e-4, 1e-6],    # 3e-3 lmax kept, 3e-4 lmax dropped: brackets the 1e-3 cutoff
    "x_zero": [0] * 6,
    "x_equal": [2.0] * 6,
    "x_diag": [0.5, 1, 2, 3, 4, 5],
}
# the branch a class is named after: (path of Mx, eigenvalues of Mx_inv dropped)
X_BRANCH = {"x_inv_well": ("inv", 0), "x_inv_small": ("inv", 0), "x_inv_indef": ("inv", 0), "x_pinv_drop2": ("pinv", 2),
            "x_pinv_rank3": ("pinv", 3), "x_pinv_keepall": ("pinv", 0), "x_pinv_near_cutoff": ("pinv", 2), "x_zero": ("pinv", 6), "x_equal": ("inv", 0),
            "x_diag": ("inv", 0)}
# The one class that sits closer to a cutoff than margin_ok's factor 10, on purpose: a cutoff moved by a factor 10
# (1e-3 -> 1e-4) changes nothing in a class that keeps a factor 10 from it.  A factor 2.5 is still 1e15 roundings wide.
NEAR_CUTOFF = {"x_pinv_near_cutoff": 2.5}
MIXED = ("mix_torque_only", "mix_upper_only", "mix_lower_only", "mix_pos_even_joints", "mix_at_1e19")


def joint_limits(n):
    """The reference's joint limits (rob_ctrl.py:238-251) for any n: the 7 entries repeated."""
    idx = np.arange(n) % 7
    return arm_qp.QMIN[idx].copy(), arm_qp.QMAX[idx].copy()


def _orth(rng, k):
    Q, _ = np.linalg.qr(rng.normal(size=(k, k)))
    return Q


def _perm(rng, k):
    return np.eye(k)[rng.permutation(k)]


def instance(rng, n, m_spec, x_spec, m_diag=False, x_diag=False, big=False):
    """One snapshot for any n in 1..8: M = Q diag(m_spec) Q', Mx_inv = P diag(x_spec) P' with random orthogonal Q, P
    (permutation matrices for the "diagonal" classes: the products are then exactly diagonal in permuted order).
    ``x_spec`` None: the structural Mx_inv = J M^-1 J' (rank n by construction for n < 6).  ``big``: a target 0.1 m
    away (active torque rows) instead of 3 mm.  q lies inside ``joint_limits(n)``."""
    m_spec = np.asarray(m_spec, float)
    Q = _perm(rng, n) if m_diag else _orth(rng, n)
    M = Q @ np.diag(m_spec) @ Q.T
    M = 0.5 * (M + M.T)
    J = rng.normal(0, 0.4, (6, n))
    Jd = rng.normal(0, 0.1, (6, n))
    if x_spec is None:
        X = J @ np.linalg.inv(M) @ J.T
    else:
        P = _perm(rng, 6) if x_diag else _orth(rng, 6)
        X = P @ np.diag(np.asarray(x_spec, float)) @ P.T
    X = 0.5 * (X + X.T)
    lo, hi = joint_limits(n)
    ee = rng.normal(0, 0.3, 3)
    return {"q": rng.uniform(np.maximum(lo + 0.3, -2.0), np.minimum(hi - 0.3, 2.0)), "qd": rng.normal(0, 0.05, n),
            "qdd_prev": rng.normal(0, 1, n), "mocap_pos": ee + rng.normal(0, 0.1 if big else 0.003, 3), "ee_pos": ee,
            "rotvec": rng.normal(0, 0.02, 3), "jac": J, "jacDot": Jd, "M": M, "h": rng.normal(0, 5, n), "Mx_inv": X}


def params(n, rng=None, absent=(), nonsym=False, full=False, dt=0.002):
    """The reference parameter set (arm_qp.default_params) generalised to n joints.

    ``absent``: bound names ("Qmin", "taumax", ...) set to -+1e20 on every row, or (name, rows) pairs for some rows.
    ``nonsym``: a non-symmetric Wimp and Wsmooth > 0 (non-symmetric too).  ``full``: a full SPD Wpos and K_null
    (both need ``rng``)."""
    idx = np.arange(n) % 7
    qmin, qmax = joint_limits(n)
    p = {"Wimp": np.diag([10.0, 10.0, 10.0, 1.0, 1.0, 1.0]), "Wpos": np.eye(n) * 0.1, "Wsmooth": np.zeros((n, n)),
         "Qmin": qmin, "Qmax": qmax, "Qdotmin": np.full(n, -20.0), "Qdotmax": np.full(n, 20.0),
         "taumin": -TAUMAX7[idx], "taumax": TAUMAX7[idx].copy(),
         "K": np.diag([5000.0, 5000.0, 5000.0, 50.0, 50.0, 50.0]), "K_null": np.eye(n), "dt": float(dt)}
    if nonsym:
        p["Wimp"] = p["Wimp"] + np.triu(np.full((6, 6), 0.3), 1)
        p["Wsmooth"] = np.eye(n) * 1e-7 + np.triu(np.full((n, n), 2e-8), 1)
    if full:
        W = rng.normal(size=(n, n))
        p["Wpos"] = W @ W.T * 0.01 + 0.05 * np.eye(n)
        W = rng.normal(size=(n, n))
        p["K_null"] = W @ W.T * 0.2 + np.eye(n)
    for a in absent:
        name, rows = (a, slice(None)) if isinstance(a, str) else a
        p[name] = p[name].copy()
        p[name][rows] = -ABSENT if name.endswith("min") else ABSENT
    return p


def mixed_params(n, pattern):
    """The bound patterns of the mixed-bounds test."""
    lows, highs = [g[0] for g in BOUND_GROUPS], [g[1] for g in BOUND_GROUPS]
    if pattern == "mix_torque_only":
        return params(n, absent=("Qmin", "Qmax", "Qdotmin", "Qdotmax"))
    if pattern == "mix_upper_only":
        return params(n, absent=lows)
    if pattern == "mix_lower_only":
        return params(n, absent=highs)
    if pattern == "mix_pos_even_joints":          # position rows absent on the odd joints
        odd = np.arange(n) % 2 == 1
        return params(n, absent=(("Qmin", odd), ("Qmax", odd)))
    if pattern == "mix_at_1e19":                  # exactly 1e19 is absent in both codes (hi < 1e19 is false)
        p = params(n)
        p["Qdotmax"] = np.full(n, 1e19)
        p["taumin"] = np.full(n, -1e19)
        return p
    raise KeyError(pattern)


def strip_bounds(prm):
    """``prm`` with all six bound groups absent."""
    p = dict(prm)
    n = len(prm["Qmin"])
    for lo, hi in BOUND_GROUPS:
        p[lo], p[hi] = np.full(n, -ABSENT), np.full(n, ABSENT)
    return p


def constraints(snap, prm):
    """A, b and the relaxed bounds lo, hi (+-inf where absent) exactly as oracle/arm_qp.py:build_qp states them."""
    n, dt = snap["q"].shape[0], prm["dt"]
    A = np.vstack([0.5 * dt ** 2 * np.eye(n), dt * np.eye(n), snap["M"]])
    b = np.concatenate([snap["qd"] * dt + snap["q"], snap["qd"], snap["h"]])
    lo = np.concatenate([prm["Qmin"], prm["Qdotmin"], prm["taumin"]]).astype(float)
    hi = np.concatenate([prm["Qmax"], prm["Qdotmax"], prm["taumax"]]).astype(float)
    lo = np.where(lo <= -arm_qp.INF_BOUND, -np.inf, lo - arm_qp.BOUND_RELAX * np.maximum(1.0, np.abs(lo)))
    hi = np.where(hi >= arm_qp.INF_BOUND, np.inf, hi + arm_qp.BOUND_RELAX * np.maximum(1.0, np.abs(hi)))
    return A, b, lo, hi


# ---------------------------------------------------------------------------------------------------------
# the QP build: exact (mpmath) and its float64 restatement
# ---------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    return mpmath


def _tomp(mp, a):
    a = np.asarray(a, float)
    if a.ndim == 1:
        return mp.matrix([mp.mpf(float(v)) for v in a])
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _tonp(mp, m, shape):
    return np.array([float(m[i, j]) for i in range(m.rows) for j in range(m.cols)]).reshape(shape)


def _spectral(mp, E, Q, w):
    """Q diag(w) Q'."""
    k = len(w)
    return Q * mp.diag(list(w)) * Q.T if k else Q


def build_exact(snap, prm, dps=50):
    """H, c, const, e0, beta, Mx, D of arm.py:335-388 evaluated in mpmath and rounded to float64, and the branch
    taken: dict(m_lam, m_dropped, x_lam, x_det, x_path, x_dropped).  One ``eigsy`` per (symmetrised) matrix; the
    cutoffs 1e-6 lmax (pinv M), |det| > 1e-8 (inv / pinv of Mx_inv) and 1e-3 lmax are decided in exact arithmetic."""
    mp = _mp()
    with mp.workdps(dps):
        n = snap["q"].shape[0]
        q, qd, qp = (_tomp(mp, snap[k]) for k in ("q", "qd", "qdd_prev"))
        J, Jd, h = _tomp(mp, snap["jac"]), _tomp(mp, snap["jacDot"]), _tomp(mp, snap["h"])
        M, X = _tomp(mp, snap["M"]), _tomp(mp, snap["Mx_inv"])
        Em, Qm = mp.eigsy((M + M.T) / 2)
        Ex, Qx = mp.eigsy((X + X.T) / 2)
        lmax_m = max(abs(e) for e in Em)
        keep_m = [abs(e) > mp.mpf("1e-6") * lmax_m for e in Em]
        Minv = _spectral(mp, Em, Qm, [1 / e if k else mp.mpf(0) for e, k in zip(Em, keep_m)])
        det = mp.mpf(1)
        for e in Ex:
            det *= e
        lmax_x = max(abs(e) for e in Ex)
        inv_path = abs(det) > mp.mpf("1e-8")
        keep_x = [bool(inv_path or abs(e) > mp.mpf("1e-3") * lmax_x) for e in Ex]
        wx = [1 / e if k else mp.mpf(0) for e, k in zip(Ex, keep_x)]
        Mx = _spectral(mp, Ex, Qx, wx)
        S = _spectral(mp, Ex, Qx, [mp.sqrt(abs(w)) for w in wx])
        K = _tomp(mp, prm["K"])
        sK = mp.matrix(6, 6)
        for i in range(6):
            for j in range(6):
                sK[i, j] = mp.sqrt(K[i, j])
        mu = Mx * (J * (Minv * h) + Jd * qd)
        D = S * sK + sK * S
        tw = _tomp(mp, np.concatenate([snap["mocap_pos"], snap["rotvec"]]))
        ee = _tomp(mp, snap["ee_pos"])
        for i in range(3):
            tw[i] -= ee[i]
        F = -(D * (J * qd)) + K * tw + mu
        e0 = Jd * qd - X * F
        Kn = _tomp(mp, prm["K_null"])
        beta = -(Kn * q)
        for i in range(n):
            beta[i] -= 2 * mp.sqrt(Kn[i, i]) * qd[i]
        dt = mp.mpf(float(prm["dt"]))
        Wi, Wp, Ws = _tomp(mp, prm["Wimp"]), _tomp(mp, prm["Wpos"]), _tomp(mp, prm["Wsmooth"])
        Wi, Wp, Ws = (Wi + Wi.T) / 2, (Wp + Wp.T) / 2, (Ws + Ws.T) / (2 * dt * dt)
        H = 2 * (J.T * Wi * J + Wp + Ws)
        c = 2 * (J.T * (Wi * e0) - Wp * beta - Ws * qp)
        const = (e0.T * Wi * e0)[0] + (beta.T * Wp * beta)[0] + (qp.T * Ws * qp)[0]
        out = {"H": _tonp(mp, H, (n, n)), "c": _tonp(mp, c, (n,)), "const": float(const), "e0": _tonp(mp, e0, (6,)),
               "beta": _tonp(mp, beta, (n,)), "Mx": _tonp(mp, Mx, (6, 6)), "D": _tonp(mp, D, (6, 6)),
               "xunc": _tonp(mp, mp.lu_solve(H, -c), (n,)) if _definite(mp, H) else None}
        branch = {"m_lam": np.array([float(e) for e in Em]), "m_dropped": int(n - sum(keep_m)),
                  "x_lam": np.array([float(e) for e in Ex]), "x_det": float(det), "x_path": "inv" if inv_path else "pinv",
                  "x_dropped": int(6 - sum(keep_x))}
    return out, branch


def _definite(mp, H):
    try:
        mp.cholesky(H)
        return True
    except (ValueError, ZeroDivisionError):
        return False


def build_f64(snap, prm):
    """The statement of ``build_exact`` in numpy float64: one ``eigh`` per matrix, explicit cutoffs, the square root
    from the same decomposition.  Returns the same dict (``xunc`` by ``np.linalg.solve``) and branch."""
    n = snap["q"].shape[0]
    q, qd, qp, J, Jd, h = snap["q"], snap["qd"], snap["qdd_prev"], snap["jac"], snap["jacDot"], snap["h"]
    M, X = snap["M"], snap["Mx_inv"]
    Em, Qm = np.linalg.eigh(0.5 * (M + M.T))
    Ex, Qx = np.linalg.eigh(0.5 * (X + X.T))
    keep_m = np.abs(Em) > 1e-6 * np.max(np.abs(Em))
    with np.errstate(divide="ignore", invalid="ignore"):
        Minv = Qm @ np.diag(np.where(keep_m, 1.0 / Em, 0.0)) @ Qm.T
        det = float(np.prod(Ex))
        inv_path = abs(det) > 1e-8
        keep_x = inv_path | (np.abs(Ex) > 1e-3 * np.max(np.abs(Ex)))
        wx = np.where(keep_x, 1.0 / Ex, 0.0)
    Mx = Qx @ np.diag(wx) @ Qx.T
    S = Qx @ np.diag(np.sqrt(np.abs(wx))) @ Qx.T
    K = prm["K"]
    mu = Mx @ (J @ (Minv @ h) + Jd @ qd)
    D = S @ np.sqrt(K) + np.sqrt(K) @ S
    tw = np.concatenate([snap["mocap_pos"] - snap["ee_pos"], snap["rotvec"]])
    F = -(D @ (J @ qd)) + K @ tw + mu
    e0 = Jd @ qd - X @ F
    Kn = prm["K_null"]
    beta = 2.0 * np.sqrt(np.diag(Kn)) * (-qd) + Kn @ (-q)
    dt = prm["dt"]
    sym = lambda W: 0.5 * (W + W.T)                  # noqa: E731
    Wi, Wp, Ws = sym(prm["Wimp"]), sym(prm["Wpos"]), sym(prm["Wsmooth"]) / dt ** 2
    H = 2.0 * (J.T @ Wi @ J + Wp + Ws)
    c = 2.0 * (J.T @ (Wi @ e0) - Wp @ beta - Ws @ qp)
    const = float(e0 @ Wi @ e0 + beta @ Wp @ beta + qp @ Ws @ qp)
    try:
        np.linalg.cholesky(H)
        xunc = np.linalg.solve(H, -c)
    except np.linalg.LinAlgError:
        xunc = None
    out = {"H": H, "c": c, "const": const, "e0": e0, "beta": beta, "Mx": Mx, "D": D, "xunc": xunc}
    branch = {"m_lam": Em, "m_dropped": int(n - keep_m.sum()), "x_lam": Ex, "x_det": det,
              "x_path": "inv" if inv_path else "pinv", "x_dropped": int(6 - keep_x.sum())}
    return out, branch


def rel_dist(a, b):
    """max |a - b| over max |b| (absolute where b is all zero)."""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    s = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / (s if s > 0.0 else 1.0)


def rounding_scale(f64, exact):
    """The instance's float64 rounding scale r_i: the largest relative distance (``rel_dist``) of the float64
    restatement from the exact evaluation over every returned quantity -- the QP data H, c, const, e0, beta, Mx, D and
    the unconstrained minimiser -H^-1 c, which carries the data's error times H's conditioning and is what the device
    test bounds.  Not below 2^-52: the exact values are themselves rounded to float64 and the kernel's inputs and
    outputs are float64, so no distance below one unit roundoff can be told from zero."""
    r = EPS
    for k in ("H", "c", "const", "e0", "beta", "Mx", "D", "xunc"):
        if exact[k] is not None and f64[k] is not None:
            r = max(r, rel_dist(f64[k], exact[k]))
    return r


def margin_ok(branch, prm, factor=10.0):
    """True when every branch decision has room: |det Mx_inv| a factor >= 100 from 1e-8; every eigenvalue ratio
    |lam| / lmax a factor >= ``factor`` (10) from its cutoff (1e-6 for M; 1e-3 for Mx_inv where the pinv path is taken -- the inv
    path keeps every eigenvalue whatever its ratio); no bound within a factor 10 of 1e19 (exactly +-1e19 is
    decided without rounding: absent in the kernel and in the oracle)."""
    det = abs(branch["x_det"])
    if 1e-10 < det < 1e-6:
        return False

    def ratios_ok(lam, cut):
        lam = np.abs(lam)
        if lam.max() == 0.0:
            return True
        r = lam / lam.max()
        return not np.any((r > cut / factor) & (r < cut * factor))
    if not ratios_ok(branch["m_lam"], 1e-6):
        return False
    if branch["x_path"] == "pinv" and not ratios_ok(branch["x_lam"], 1e-3):
        return False
    for lo, hi in BOUND_GROUPS:
        for v in np.concatenate([np.abs(prm[lo]), np.abs(prm[hi])]):
            if v != 1e19 and 1e18 < v < 1e20:
                return False
    return True


# ---------------------------------------------------------------------------------------------------------
# the exact KKT point of the relaxed QP
# ---------------------------------------------------------------------------------------------------------
def kkt_point_exact(H, c, A, b, lo, hi, x_ipm, zu, zl, dps=50):
    """The exact KKT point of min 1/2 x'Hx + c'x s.t. lo <= Ax + b <= hi with the active set read from an
    ``arm_qp.qp_ipm`` solve (x_ipm, zu, zl): a row side is active when its multiplier exceeds its slack.  The
    equality-constrained KKT system is solved in mpmath.  Returns (x*, strictly_complementary); the flag is true only
    if for every present row side z / slack lies outside [1e-3, 1e3], the exact multipliers are positive and x* is
    feasible (a singular KKT system -- dependent active rows -- gives (x_ipm, False))."""
    mp = _mp()
    n = H.shape[0]
    r = A @ x_ipm + b
    act, clear = [], True                       # (row, sign, bound)
    for i in range(A.shape[0]):
        for z, slack, sgn, bound in ((zu[i], hi[i] - r[i], 1, hi[i]), (zl[i], r[i] - lo[i], -1, lo[i])):
            if not np.isfinite(bound):
                continue
            ratio = z / slack if slack > 0 else np.inf
            if 1e-3 <= ratio <= 1e3:
                clear = False
            if z > slack:
                act.append((i, sgn, bound))
    with mp.workdps(dps):
        Hm, cm = _tomp(mp, H), _tomp(mp, c)
        k = len(act)
        if k > n:
            return np.array(x_ipm, float), False
        KK = mp.matrix(n + k, n + k)
        rhs = mp.matrix(n + k, 1)
        for i in range(n):
            rhs[i] = -cm[i]
            for j in range(n):
                KK[i, j] = Hm[i, j]
        for a, (i, sgn, bound) in enumerate(act):
            for j in range(n):
                KK[n + a, j] = KK[j, n + a] = sgn * mp.mpf(float(A[i, j]))
            rhs[n + a] = sgn * (mp.mpf(float(bound)) - mp.mpf(float(b[i])))
        try:
            sol = mp.lu_solve(KK, rhs)
        except ZeroDivisionError:
            return np.array(x_ipm, float), False
        xs = [sol[i] for i in range(n)]
        ok = clear and all(sol[n + a] > 0 for a in range(k))
        for i in range(A.shape[0]):
            g = mp.mpf(float(b[i]))
            for j in range(n):
                g += mp.mpf(float(A[i, j])) * xs[j]
            slop = mp.mpf(10) ** -40                  # active rows hold to the working precision, not exactly
            if (np.isfinite(hi[i]) and g > mp.mpf(float(hi[i])) + slop * (1 + abs(g))) or \
               (np.isfinite(lo[i]) and g < mp.mpf(float(lo[i])) - slop * (1 + abs(g))):
                ok = False
        return np.array([float(v) for v in xs]), bool(ok)


def exact_outputs(snap, prm, ex, x):
    """(f, tau) the kernel publishes at x, from the exact QP data: f = const + c'x + x'Hx / 2, tau = M x + h, in
    mpmath from the float64 x."""
    mp = _mp()
    with mp.workdps(50):
        xm = _tomp(mp, x)
        H, c = _tomp(mp, ex["H"]), _tomp(mp, ex["c"])
        f = mp.mpf(ex["const"]) + (c.T * xm)[0] + (xm.T * H * xm)[0] / 2
        tau = _tomp(mp, snap["M"]) * xm + _tomp(mp, snap["h"])
        return float(f), np.array([float(tau[i]) for i in range(len(x))])
