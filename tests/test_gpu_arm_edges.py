"""The arm-QP kernel (csrc/arm_qp.hip) against EXACT answers at every joint count n = 1..8, through the public entry
``dart_arm_solve_batch`` (the product object; no probe build).

tests/test_gpu_arm.py compares n = 7 (and one n = 6 batch) with oracle/arm_qp.py at 1e-6: that is the oracle's noise
floor on the pinv branch, six of the eight instantiations never ran, and whole branches of the QP build were never
taken.  Here the reference is tests/golden/arm_edge_goldens.npz: the formulas of arm.py:335-388 evaluated in mpmath
(tests/arm_refs.py via tests/golden/make_arm_edge_goldens.py; this module reads only the fixture, which also holds
what oracle/arm_qp.py:qp_ipm gives on the exact data).
Classes, each at every n it applies to:
  M spectra    well conditioned, all equal, equal in pairs, graded over 1e3, exactly diagonal (permuted), one eigenvalue
               at 3e-8 lmax (pinv(M) truncates);
  Mx_inv       inv path (well conditioned; one eigenvalue 2e-4 lmax, kept; indefinite; all equal; exactly diagonal),
               pinv path (two dropped; rank 3 with exact zeros; all six kept; one kept at 3e-3 lmax and one dropped
               at 3e-4 lmax, either side of the cutoff; the zero matrix; J M^-1 J' for n < 6);
  parameters   non-symmetric Wimp and Wsmooth > 0; full Wpos and K_null; five patterns of absent bounds;
  statuses     infeasible (-3), breakdown (-2), max_iter (-1); hard-hard pairs at n = 7, 8.
DART_ARM_ACCEPTABLE (1) is NOT tested: it needs a pivot to fail with the KKT error between tol and acceptable_tol,
and no deterministic input for that is known.

Tolerances.  r_i is the instance's float64 rounding scale: the distance of a float64 numpy restatement of the build
from the exact one (>= 2^-52).  With all bounds absent the IPM is a 0.99-damped Newton iteration on H x = -c, so
  |qdd - x*|_inf  <= tol sd |H^-1|_inf + 64 r_i (1 + |x*|_inf)     (the stopping rule on the exact H, c + the scale),
  |loss - f*|     <= 64 r_i (|const| + |c'x*| + |x*'Hx*| / 2)       (second order in the error of x),
  |tau - tau*|_inf <= |M|_inf (the qdd bound) + 64 r_i |h|_inf      (tau = M x + h).
The factor 64 is a margin over LAPACK-based float64 for ~112 Jacobi rotations per index on v_rsq / v_rcp + Newton.
Measured on an MI355X, worst over n = 1..8 per class, in units of r_i x scale (printed per instance with -s):
  loss   x_zero 0.94, p_full 0.47, m_diag 0.29, mix_lower_only 0.27, x_equal 0.25, x_pinv_keepall 0.22,
         mix_at_1e19 0.19, m_pairs 0.18, m_equal 0.17, st_infeasible 0.15, m_well 0.13, mix_torque_only 0.11,
         every other class <= 0.09 (the hard-hard pairs <= 0.02);
  qdd    beyond the stopping term: m_well 0.25, mix_lower_only 0.21, every other class 0 (the raw error is up to
         2300 r_i scales: the stopping term tol sd |H^-1| is what the iteration leaves, the loss is the sharp check);
  tau    beyond |M| (the qdd bound): 0 in every class.
No class comes near 64.  Iterations: 6 or 7 in every instance.
With the rows' own bounds, |qdd - x*| / (1 + |x*|) <= max(8 d_i, 1e-9) where d_i is the distance of the oracle's
qp_ipm (same algorithm, same tol) from x* on that instance.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = tuple(range(1, 9))
MARGIN = 64.0
STATUS_CLASSES = ("st_infeasible", "st_breakdown")
BOUNDS = ("Qmin", "Qmax", "Qdotmin", "Qdotmax", "taumin", "taumax")


@pytest.fixture(scope="module")
def edge():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "arm_edge_goldens.npz"))
    return {k: d[k] for k in d.files}


def _at(g, n):
    pre = f"n{n}_"
    e = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    e["prm"] = e["prmtab"][e["prmid"]]
    e["cls"] = np.array([str(c) for c in e["cls"]])
    return e


def _field(n, name, table):
    """Slice of ``name`` in a snapshot / parameter row (include/dart_mpc.h layouts)."""
    from dart_mpc.arm import _width
    o = 0
    for k, w in table:
        m = _width(w, n)
        if k == name:
            return slice(o, o + m)
        o += m
    raise KeyError(name)


def _without_bounds(rows, n):
    from dart_mpc.arm import PARAM_FIELDS
    rows = np.array(rows, dtype=np.float64)
    for k in BOUNDS:
        rows[..., _field(n, k, PARAM_FIELDS)] = -1e20 if k.endswith("min") else 1e20
    return rows


def _bits(out, i):
    return b"".join(np.ascontiguousarray(out[k][i]).tobytes() for k in ("qdd", "tau", "loss", "status", "iters"))


def test_fixture_covers_every_joint_count(edge):
    for n in NS:
        e = _at(edge, n)
        assert e["snap"].shape[0] >= 19 and np.all(e["r"] >= 2.0 ** -52) and np.all(e["r"] <= 1e-12)
        assert np.all(e["margin"] == (e["cls"] != "x_pinv_near_cutoff"))


@pytest.mark.parametrize("n", NS)
def test_qp_build_bounds_absent(edge, n):
    """H, c and the cost (e0, beta, Mx, D, mu, F behind them) of every class against the exact build."""
    import dart_mpc
    from dart_mpc.arm import SNAP_FIELDS
    e = _at(edge, n)
    use = np.flatnonzero(np.isfinite(e["func"]))
    assert len(use) == len(e["cls"]) - 1                                   # all but st_breakdown (H indefinite)
    tol = 1e-12
    solver = dart_mpc.ArmSolver(n, tol=tol, acceptable_tol=1e-7)
    out = {}
    for pid in np.unique(e["prmid"][use]):                                 # one shared parameter row per launch
        idx = use[e["prmid"][use] == pid]
        o = solver.solve_batch(e["snap"][idx], _without_bounds(e["prmtab"][pid], n))
        for j, i in enumerate(idx):
            out[i] = {k: v[j] for k, v in o.items()}
    bad = []
    for i in use:
        o, cls, r = out[i], e["cls"][i], e["r"][i]
        H, c, xs = e["H"][i], e["c"][i], e["xunc"][i]
        M = e["snap"][i][_field(n, "M", SNAP_FIELDS)].reshape(n, n)
        h = e["snap"][i][_field(n, "h", SNAP_FIELDS)]
        stop = tol * (1.0 + np.max(np.abs(c))) * np.linalg.norm(np.linalg.inv(H), np.inf)
        sx = r * (1.0 + np.max(np.abs(xs)))
        sf = r * (abs(e["const"][i]) + abs(c @ xs) + abs(xs @ H @ xs) / 2.0)
        st = r * np.max(np.abs(h))
        mn = np.linalg.norm(M, np.inf)
        ex = float(np.max(np.abs(o["qdd"] - xs)))
        ef = float(abs(o["loss"] - e["func"][i]))
        et = float(np.max(np.abs(o["tau"] - e["tauunc"][i])))
        raw = ex / sx
        ratios = (max(0.0, ex - stop) / sx, ef / sf, max(0.0, et - mn * (stop + MARGIN * sx)) / st if st > 0 else 0.0)
        print(f"n={n} {cls:28s} status {o['status']} iters {o['iters']:2d} r_i {r:.1e} qdd {ratios[0]:7.2f} (raw {raw:9.2f}) "
              f"loss {ratios[1]:7.2f} tau-excess {ratios[2]:7.2f}  (x r_i scale)")
        if o["status"] != 0 or ex > stop + MARGIN * sx or ef > MARGIN * sf or et > mn * (stop + MARGIN * sx) + MARGIN * st:
            bad.append((cls, int(o["status"]), ratios))
    assert not bad, bad


def _constrained(edge, n, pick, **cfg):
    import dart_mpc
    e = _at(edge, n)
    idx = np.flatnonzero(pick(e) & (e["st"] == 0) & e["sc"] & e["margin"])      # (status parity: only with margin)
    out = dart_mpc.ArmSolver(n, **cfg).solve_batch(e["snap"][idx], e["prm"][idx])      # per-instance rows
    assert np.array_equal(out["status"], np.zeros(len(idx), np.int32)), (n, e["cls"][idx], out["status"])
    err = np.max(np.abs(out["qdd"] - e["x"][idx]) / (1.0 + np.abs(e["x"][idx])), axis=1)
    lim = np.maximum(8.0 * e["d"][idx], 1e-9)
    for c, a, b_, k, kk in zip(e["cls"][idx], err, lim, out["iters"], e["it"][idx]):
        print(f"n={n} {c:28s} err {a:.1e} bound {b_:.1e} iters {k} (qp_ipm {kk})")
    assert np.all(err <= lim), (n, e["cls"][idx][err > lim], err[err > lim], lim[err > lim])
    return out["iters"] == e["it"][idx]


def test_constrained_solve_vs_exact_kkt_point(edge):
    """Default config, the classes' own bounds, the strictly complementary instances: the exact KKT point.
    Measured on an MI355X: median error 3.4e-12, the worst 0.43 of its bound, iteration counts equal on all."""
    same = np.concatenate([_constrained(edge, n, lambda e: ~np.isin(e["cls"], STATUS_CLASSES) &
                                        ~np.char.startswith(e["cls"], "mix_")) for n in NS])
    assert len(same) >= 100 and same.mean() >= 0.95, (len(same), same.mean())


def test_mixed_bounds(edge):
    """Torque rows only, upper sides only, lower sides only, position rows absent on odd joints, bounds exactly at
    1e19: ``cnt``, ``nact`` and ``z0`` of the kernel; one launch per n with parameter rows that differ."""
    same = np.concatenate([_constrained(edge, n, lambda e: np.char.startswith(e["cls"], "mix_")) for n in NS])
    assert len(same) >= 35 and same.mean() >= 0.95, (len(same), same.mean())


@pytest.mark.parametrize("cls,want", [("st_infeasible", -3), ("st_breakdown", -2)])
def test_failure_statuses(edge, cls, want):
    """A joint beyond its limit (-3) and a negative definite Wpos (-2) at each n.  Status parity is asserted where the
    branch decisions have room and qp_ipm gives the same status on 8 copies perturbed by 1e-12 (the fixture says)."""
    import dart_mpc
    for n in NS:
        e = _at(edge, n)
        i = np.flatnonzero(e["cls"] == cls)
        assert len(i) == 1 and e["st"][i[0]] == want and e["margin"][i[0]] and e["stable"][i[0]]
        out = dart_mpc.ArmSolver(n).solve_batch(e["snap"][i], e["prm"][i])
        assert out["status"][0] == want, (n, out["status"])


def test_max_iter_returns_the_third_iterate(edge):
    """max_iter = 3: DART_ARM_MAXITER, iters == 3 and the iterate of qp_ipm(max_iter=3) on the exact data."""
    import dart_mpc
    count = 0
    for n in NS:
        e = _at(edge, n)
        idx = np.flatnonzero((e["st3"] == -1) & (e["st"] == 0) & (e["it"] >= 5) & e["stable"] & e["margin"])
        out = dart_mpc.ArmSolver(n, max_iter=3).solve_batch(e["snap"][idx], e["prm"][idx])
        assert np.all(out["status"] == -1) and np.all(out["iters"] == 3), (n, out["status"], out["iters"])
        err = np.max(np.abs(out["qdd"] - e["x3"][idx]) / (1.0 + np.abs(e["x3"][idx])), axis=1)
        assert np.all(err <= 1e-9), (n, e["cls"][idx][err > 1e-9], err.max())
        count += len(idx)
    assert count >= 150


@pytest.mark.parametrize("n", [7, 8])
def test_outputs_do_not_depend_on_batch_position(edge, n):
    """One mixed batch, the same in permuted order, and one launch per instance: all five outputs bit-identical per
    instance (LDS state read before it is written, padding lanes)."""
    import dart_mpc
    e = _at(edge, n)
    B = len(e["cls"])
    s = dart_mpc.ArmSolver(n)
    a = s.solve_batch(e["snap"], e["prm"])
    perm = np.random.default_rng(n).permutation(B)
    p = s.solve_batch(e["snap"][perm], e["prm"][perm])
    for j, i in enumerate(perm):
        assert _bits(p, j) == _bits(a, i), (n, e["cls"][i], "permuted")
    for i in range(B):
        o = s.solve_batch(e["snap"][i:i + 1], e["prm"][i:i + 1])
        assert _bits(o, 0) == _bits(a, i), (n, e["cls"][i], "alone")


@pytest.mark.parametrize("n", [1, 7, 8])
def test_non_finite_input_is_a_breakdown(edge, n):
    """A NaN or inf in each snapshot field in turn, and in Wpos and dt of the parameter row: DART_ARM_BREAKDOWN, never
    a status >= 0, and the call returns (every loop of the kernel is bounded: 16 sweeps, max_iter).  Finite instances
    of the same batch are solved bit-identically to a batch without the bad rows."""
    import dart_mpc
    from dart_mpc.arm import PARAM_FIELDS, SNAP_FIELDS
    e = _at(edge, n)
    good = np.flatnonzero(np.isin(e["cls"], ("m_well", "x_pinv_drop2")))
    snaps, prms, names = [e["snap"][good[0]]], [e["prm"][good[0]]], ["good"]
    for val in (np.nan, np.inf):
        for tab, fields in ((SNAP_FIELDS, [k for k, _ in SNAP_FIELDS]), (PARAM_FIELDS, ["Wpos", "dt"])):
            for k in fields:
                s, p = e["snap"][good[0]].copy(), e["prm"][good[0]].copy()
                (s if tab is SNAP_FIELDS else p)[_field(n, k, tab)][-1:] = val
                snaps.append(s), prms.append(p), names.append(f"{val} in {k}")
    snaps.append(e["snap"][good[1]]), prms.append(e["prm"][good[1]]), names.append("good")
    s = dart_mpc.ArmSolver(n)
    out = s.solve_batch(np.array(snaps), np.array(prms))
    ref = s.solve_batch(e["snap"][good], e["prm"][good])
    assert ref["status"].tolist() == [0, 0]
    assert _bits(out, 0) == _bits(ref, 0) and _bits(out, len(names) - 1) == _bits(ref, 1)
    got = {nm: int(st) for nm, st in zip(names[1:-1], out["status"][1:-1])}
    assert all(v == -2 for v in got.values()), {k: v for k, v in got.items() if v != -2}
