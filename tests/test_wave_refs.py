"""Host-only checks of what the device tests of csrc/wave.h and csrc/ocp_wave.h stand on (tests/wave_refs.py,
tests/ocp_refs.py): the longdouble references against mpmath, the input generators against the seams they claim,
the Python restatement of the LDS layout against the compiled one, and the Riccati references against each other."""
import numpy as np
import pytest

import ocp_refs as ocp
import wave_refs as wr


def test_longdouble_is_extended():
    wr.require_longdouble()


@pytest.mark.parametrize("ref,gen", wr.REGIONS, ids=[r for r, _ in wr.REGIONS])
def test_longdouble_references_agree_with_mpmath(ref, gen):
    """4096 points of every region: the longdouble library functions against mpmath at 40 digits, to 4 units of
    the longdouble's last place (2^-9 of a double's ulp)."""
    mpmath = pytest.importorskip("mpmath")
    wr.require_longdouble()
    mpmath.mp.dps = 40
    f = {"rcp": lambda v: 1 / v, "log": mpmath.log, "exp": mpmath.exp, "tanh": mpmath.tanh, "sin": mpmath.sin,
         "cos": mpmath.cos, "log2": lambda v: mpmath.log(v, 2)}[ref]
    eps = float(np.finfo(wr.LD).eps)
    for reg, x in gen().items():
        x = x[:: max(1, x.size // 4096)][:4096]
        x = x[np.isfinite(x)]
        got = wr.REFS[ref](x)
        worst = 0.0
        for xi, gi in zip(x, got):
            want = f(mpmath.mpf(float(xi)))
            hi, lo = float(gi), float(gi - wr.LD(float(gi)))          # the longdouble as two doubles, exactly
            err = abs(mpmath.mpf(hi) + mpmath.mpf(lo) - want)
            unit = max(abs(want), mpmath.mpf(2) ** -1074 / eps) * eps  # relative; absolute below the subnormals
            worst = max(worst, float(err / unit))
        assert worst <= 4.0, (ref, reg, worst)


def test_log_inputs_straddle_the_mantissa_switch():
    x = wr.log_seam_inputs()
    m, e = np.frexp(x)
    assert (m < wr.SQRT_HALF).any() and (m >= wr.SQRT_HALF).any()
    for ee in np.unique(e):                   # at every exponent, points on both sides
        mm = m[e == ee]
        assert (mm < wr.SQRT_HALF).any() and (mm >= wr.SQRT_HALF).any()
    reg = wr.log_inputs()
    assert reg["exponents -1020..1020"].max() < 1e308 and reg["exponents -1020..1020"].min() >= 2.0 ** -1020
    assert np.all(wr.log_subnormal_inputs() < 2.0 ** -1022) and np.all(wr.log_subnormal_inputs() > 0)


def test_exp_inputs_straddle_every_reduction_tie():
    x, n = wr.exp_tie_inputs()
    got = wr.reduction_index(x)
    for nn in np.unique(n):
        s = got[n == nn]
        assert (s == nn).any() and (s == nn + 1).any(), nn
    reg = wr.exp_inputs()
    sub = reg["[-745, -708] (subnormal results)"]
    assert sub.min() >= -745.0 and (np.exp(sub.astype(wr.LD)) < wr.LD(2.0) ** -1022).mean() > 0.9
    assert reg["reduction ties"].min() < -744.0 and reg["reduction ties"].max() > 708.0


def test_tanh_inputs_straddle_the_first_seams():
    n = wr.reduction_index(wr.tanh_inputs()["[-0.6, 0.6]"], 2.0)
    assert set(np.unique(n)) >= {-1.0, 0.0, 1.0}
    n = wr.reduction_index(wr.tanh_inputs()["[-45, 45]"], 2.0)
    assert n.min() <= -115 and n.max() >= 115            # up to the clamp |2x| <= 80
    assert 5e-324 in wr.tanh_inputs()["+-2^-k, +-0"]


# ---------------------------------------------------------------------------------------------------------
# Riccati references
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", (1, 2))
def test_layout_restatement_matches_the_compiled_probes(waves):
    """The NodeArr strides and image sizes written in Python from the header against the library's (no GPU)."""
    from dart_mpc import _lib
    lay = _lib.probe_layout(waves)
    a, s = ocp.layout("aug", waves), ocp.layout("s", waves)
    assert (lay["threads"], lay["aug_nmaxs"], lay["s_nmaxs"]) == (64 * waves, a["nmaxs"], s["nmaxs"])
    assert (lay["aug_M"], lay["aug_G"], lay["s_M"], lay["s_G"]) == (a["msize"], a["gsize"], s["msize"], s["gsize"])
    assert (a["swm"], a["swg"], s["swm"], s["swg"]) == (74, 46, 42, 30)
    if waves == 2:
        assert lay["aug_bytes"] == 134784


SHAPES = sorted(set(ocp.ONE_WAVE_N + ocp.TWO_WAVE_N))


@pytest.mark.parametrize("form", ("aug", "s"))
@pytest.mark.parametrize("N", SHAPES)
def test_riccati_references(form, N):
    """Conditions on the inputs: the refined dense solution satisfies the KKT system to 1e-15 relative in
    longdouble, and the float64 textbook recursion agrees with it to 1e-10 relative (e_ref)."""
    wr.require_longdouble()
    for inst in range(ocp.INSTANCES):
        for half, sub in enumerate(ocp.problem(form, N, inst)):
            assert np.max(np.abs(np.linalg.eigvals(sub["A"]))) <= 0.95 + 1e-12
            ref = ocp.dense_reference(form, N, inst, half)
            assert ref["resid"] <= 1e-15, (inst, half, ref["resid"])
            # the value function of node 0 from the dense solves against the recursion's
            tb = ocp.textbook_recursion(sub)
            nxa = sub["nxa"]
            assert np.max(np.abs(ref["Pt0"][:nxa, :nxa] - tb["P"][0])) <= 1e-10 * np.max(np.abs(tb["P"][0]))
    e = ocp.e_ref(form, N)
    print(f"{form} N = {N}: e_ref = {e:.3e}, tolerance {ocp.tolerance(form, N):.3e}")
    assert e <= 1e-10


@pytest.mark.parametrize("form", ("aug", "s"))
@pytest.mark.parametrize("N", (3, 22, 33, 62))
def test_negative_quu_modification(form, N):
    """The inertia cases: the modified stage's reference Quu is below -1e-3 |Quu| in every eigenvalue."""
    sub = ocp.problem(form, N, 0)[0]
    for node in ocp.flag_nodes(N):
        mod = ocp.with_negative_quu(sub, node)
        Q = ocp.textbook_recursion(mod)["Quu"][node]
        assert np.max(np.linalg.eigvalsh(Q)) < -1e-3 * np.max(np.abs(Q))
        assert np.all(np.linalg.eigvalsh(ocp.textbook_recursion(sub)["Quu"][node]) > 0)


def test_packing_round_trip():
    """G[N] of the packed image holds the terminal value function: its Schur complement on u is Pt_N."""
    for form in ("aug", "s"):
        subs = ocp.problem(form, 4, 0)
        lay = ocp.layout(form, 1)
        Mi, Hi, Gi, dx0 = ocp.pack(form, 1, subs)
        assert Mi.size == lay["msize"] and Hi.size == Gi.size == lay["gsize"] and dx0.size == lay["nxa"] * len(subs)
        for h, sub in enumerate(subs):
            G = ocp.unpack_g(form, 1, Gi, lay["nmaxs"] * h + 4)
            Pt = ocp.value_of_g(G, lay["nxa"], lay["nu"])
            assert np.array_equal(Pt.astype(np.float64), ocp.terminal_value(sub))
            Ht, M = ocp.stage_matrices(sub, 2)
            s = lay["nmaxs"] * h + 2
            assert Mi[s * lay["swm"] + (lay["ND"] - 1) * lay["NC"] + lay["nxa"]] == 1.0     # the homogeneous row
            assert np.array_equal(ocp.unpack_g(form, 1, Hi, s).astype(np.float64), Ht)
