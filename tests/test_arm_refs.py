"""Host-only checks of what the device tests of csrc/arm_qp.hip stand on (tests/arm_refs.py and the fixture
tests/golden/arm_edge_goldens.npz of tests/golden/make_arm_edge_goldens.py): the exact build against the oracle
where the oracle is good (inv path) and away from it where it is not (pinv path), the float64 restatement against
the exact build, the branch every class claims, the classes present per joint count, and the fixture's bits."""
import os
import sys

import numpy as np
import pytest

import arm_qp

pytest.importorskip("mpmath")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import arm_refs as ar  # noqa: E402
import make_arm_edge_goldens as gen  # noqa: E402
from test_oracle_arm import _unpack  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def edge():
    d = np.load(os.path.join(GOLD, "arm_edge_goldens.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def rebuilt(edge):
    """(exact, float64, branch, snapshot, parameters) of every fixture case, from its stored rows: computed once."""
    out = {}
    for n in gen.NS:
        for i, cls in enumerate(edge[f"n{n}_cls"]):
            s, p = _unpack(edge[f"n{n}_snap"][i], edge[f"n{n}_prmtab"][edge[f"n{n}_prmid"][i]], n)
            ex, br = ar.build_exact(s, p)
            out[n, i] = (ex, ar.build_f64(s, p)[0], br, s, p, str(cls))
    return out


def test_exact_build_vs_oracle_on_the_workload_goldens():
    """arm_goldens.npz (the n = 7 workload mix).  On the inv path the exact build and oracle/arm_qp.py:build_qp agree
    to the oracle's rounding level, cond(Mx_inv) x eps.  On the pinv path with two eigenvalues dropped the oracle's D
    is more than 1e-10 relative away from the exact one (4e-9 .. 2.8e-8 here): its second eigh of Mx returns the two
    dropped eigenvalues as ~1e-17 noise, whose square roots are ~3e-9.  This half pins the gap, so that nobody later
    "fixes" the exact reference towards the oracle.  With ONE eigenvalue dropped the gap is smaller (3e-13 .. 8e-11
    here: a single noise eigenvalue comes back closer to zero), so those entries are only required to take the pinv
    path; Mx itself agrees on both paths."""
    g = np.load(os.path.join(GOLD, "arm_goldens.npz"))
    seen = {("inv", 0): 0, ("pinv", 1): 0, ("pinv", 2): 0}
    for i in range(len(g["kinds"])):
        s, p = _unpack(g["snap"][i], g["prm"][i])
        ex, br = ar.build_exact(s, p)
        H, c, const, A, b, lo, hi, aux = arm_qp.build_qp(s, p)
        dD = ar.rel_dist(aux["D"], ex["D"])
        lam = np.abs(br["x_lam"])
        assert ar.rel_dist(H, ex["H"]) <= 1e-13, i
        if br["x_path"] == "inv":
            level = 16 * ar.EPS * lam.max() / lam.min()
            assert dD <= level and ar.rel_dist(aux["Mx"], ex["Mx"]) <= level and ar.rel_dist(c, ex["c"]) <= level, (i, dD)
        else:
            assert ar.rel_dist(aux["Mx"], ex["Mx"]) <= 1e-12, i            # kept ratios >= 1e-3
            if br["x_dropped"] >= 2:
                assert dD > 1e-10, (i, dD)
        seen[br["x_path"], br["x_dropped"]] += 1
    assert seen["inv", 0] >= 50 and seen["pinv", 2] >= 5 and seen["pinv", 1] >= 5, seen


def test_float64_restatement_agrees_with_exact(rebuilt, edge):
    """1e-12 relative on every fixture case and every returned quantity; the stored r_i is that distance."""
    for (n, i), (ex, f64, br, s, p, cls) in rebuilt.items():
        r = ar.rounding_scale(f64, ex)
        assert r <= 1e-12, (n, cls, r)
        assert r == edge[f"n{n}_r"][i], (n, cls)
        for k in ("H", "c"):
            assert np.array_equal(ex[k], edge[f"n{n}_{k}"][i]), (n, cls, k)


def test_every_case_takes_its_branch_with_margin(rebuilt, edge):
    for (n, i), (ex, f64, br, s, p, cls) in rebuilt.items():
        e = {"margin": edge[f"n{n}_margin"][i], "st": edge[f"n{n}_st"][i], "stable": edge[f"n{n}_stable"][i]}
        assert e["margin"] == ar.margin_ok(br, p)
        gen.check_branch(n, cls, br, p, e)


def test_margin_ok_refuses_decisions_without_room():
    rng = np.random.default_rng(3)
    p = ar.params(7)
    ok = ar.instance(rng, 7, ar.M_SPECS["m_well"](7), ar.X_SPECS["x_pinv_drop2"])
    assert ar.margin_ok(ar.build_f64(ok, p)[1], p)
    for spec in ([3, 2, 1, 0.5, 2e-3, 1e-6],            # an eigenvalue 6.7e-4 lmax on the pinv path
                 [0.1, 0.1, 0.1, 0.1, 0.1, 0.05]):      # |det| = 5e-7
        s = ar.instance(rng, 7, ar.M_SPECS["m_well"](7), spec)
        assert not ar.margin_ok(ar.build_f64(s, p)[1], p), spec
    s = ar.instance(rng, 7, np.concatenate([np.linspace(1, 3, 6), [6e-6]]), ar.X_SPECS["x_inv_well"])
    assert not ar.margin_ok(ar.build_f64(s, p)[1], p)   # an eigenvalue of M at 2e-6 lmax
    assert not ar.margin_ok(ar.build_f64(ok, p)[1], dict(p, taumax=np.full(7, 5e18)))
    assert ar.margin_ok(ar.build_f64(ok, p)[1], ar.mixed_params(7, "mix_at_1e19"))


def test_every_class_present_for_every_joint_count(edge):
    for n in gen.NS:
        have = [str(c) for c in edge[f"n{n}_cls"]]
        assert have == gen.class_list(n)
        want = {k for k in ar.M_SPECS if n >= ar.M_MIN_N.get(k, 1)} | (set(ar.X_SPECS) - {"x_inv_well"}) | \
            set(ar.MIXED) | {"p_nonsym", "p_full", "st_infeasible", "st_breakdown"} | ({"x_struct"} if n < 6 else set())
        assert want <= set(have), (n, want - set(have))
        assert len(np.unique(edge[f"n{n}_prmid"])) >= 8          # parameter rows that differ within one batch
    assert sum(c.startswith("hard_") for n in (7, 8) for c in map(str, edge[f"n{n}_cls"])) == 8
    # the exclusion cap of the constrained test, as the generator asserts it
    sc = np.concatenate([edge[f"n{n}_sc"][~np.isin(edge[f"n{n}_cls"], gen.STATUS_CLASSES)] for n in gen.NS])
    assert sc.mean() >= 0.8
    assert sum(int(np.sum(edge[f"n{n}_nact"] > 0)) for n in gen.NS) >= 100      # active rows in most instances
    assert os.path.getsize(os.path.join(GOLD, "arm_edge_goldens.npz")) <= 4 * os.path.getsize(
        os.path.join(GOLD, "arm_goldens.npz"))


def test_kkt_point_exact_on_a_hand_made_qp():
    """min 1/2 |x|^2 - (3, 1).x  s.t.  x0 <= 1 (active, multiplier 2), x1 <= 5 (inactive): x* = (1, 1)."""
    H, c = np.eye(2), np.array([-3.0, -1.0])
    A, b = np.eye(2), np.zeros(2)
    lo, hi = np.full(2, -np.inf), np.array([1.0, 5.0])
    x, st, it, zu, zl = arm_qp.qp_ipm(H, c, A, b, lo, hi)
    xs, sc = ar.kkt_point_exact(H, c, A, b, lo, hi, x, zu, zl)
    assert st == 0 and sc and np.array_equal(xs, [1.0, 1.0])
    hi2 = np.array([3.0, 5.0])                           # the bound touches the free minimiser: not strictly complementary
    x, st, it, zu, zl = arm_qp.qp_ipm(H, c, A, b, lo, hi2)
    assert not ar.kkt_point_exact(H, c, A, b, lo, hi2, x, zu, zl)[1]


@pytest.mark.parametrize("n,idx", [(1, 3), (4, 14), (7, 5), (8, 9), (8, 23), (5, 19)])
def test_generator_reproduces_fixture_entries_bit_for_bit(edge, n, idx):
    e = gen.make_entry(n, idx)[0]
    assert e["cls"] == str(edge[f"n{n}_cls"][idx])
    assert np.array_equal(e["prm"], edge[f"n{n}_prmtab"][edge[f"n{n}_prmid"][idx]])
    for k in gen.KEYS:
        if k not in ("cls", "prmid"):
            assert np.array_equal(np.asarray(e[k]), edge[f"n{n}_{k}"][idx], equal_nan=True), (n, idx, k)


def test_non_finite_input_is_a_breakdown_in_the_oracle():
    """The contract of include/dart_mpc.h mirrored by oracle/arm_qp.py:solve_arm: status -2, no exception."""
    rng = np.random.default_rng(5)
    s = ar.instance(rng, 7, ar.M_SPECS["m_well"](7), ar.X_SPECS["x_inv_well"])
    p = arm_qp.default_params()
    assert arm_qp.solve_arm(s, p)["status"] == 0
    for k, v in (("h", np.nan), ("Mx_inv", np.inf), ("jac", np.nan), ("qdd_prev", np.inf)):
        bad = {kk: vv.copy() for kk, vv in s.items()}
        bad[k].flat[-1] = v
        r = arm_qp.solve_arm(bad, p)
        assert r["status"] == -2 and r["iters"] == 0 and np.array_equal(r["qdd"], bad["qdd_prev"], equal_nan=True)
    assert arm_qp.solve_arm(s, dict(p, dt=np.nan))["status"] == -2
    assert arm_qp.solve_arm(s, dict(p, Wpos=np.full((7, 7), np.inf)))["status"] == -2
