"""The Riccati engine of csrc/ocp_wave.h on the device (csrc/wave_probe.hip instantiates it as the solvers do:
sweep -> closed loop -> forward sweep -> multipliers) against a dense KKT solve of the problem the header documents
(tests/ocp_refs.py; refined with longdouble residuals).

Tolerance per shape: 16 e_ref with a floor of 64 x 2^-53, e_ref the distance of an independent float64 textbook
recursion from the dense solution -- a margin over another fp64 implementation, not over the kernel.  The horizons
cover N = 1, the odd terminal node, no pair at all (np2 = 0), one and two rounds of compose_pairs, and both sides of
the two-wave split at node 32.  Each case prints its error as a fraction of the tolerance."""
import numpy as np
import pytest

import ocp_refs as ocp

pytestmark = pytest.mark.gpu

SHAPES = [(1, N) for N in ocp.ONE_WAVE_N] + [(2, N) for N in ocp.TWO_WAVE_N + ocp.TWO_WAVE_SMALL_N]
FLAG_SHAPES = [(1, 3), (1, 22), (2, 33), (2, 62)]


def _run(form, waves, subs):
    from dart_mpc import _lib
    N = subs[0]["N"]
    Mi, Hi, Gi, dx0 = ocp.pack("aug" if form == "aug" else "s", waves, subs)
    out = _lib.probe_riccati(form, N, Mi, Hi, Gi, dx0, waves)
    nm = 32 * waves
    per = [dict(dx=out["dx"][nm * h:nm * h + N + 1], du=out["du"][nm * h:nm * h + N], lam=out["lam"][nm * h:nm * h + N + 1])
           for h in range(len(subs))]
    return out, per


_CACHE = {}


def _device(form, waves, N, inst):
    key = (form, waves, N, inst)
    if key not in _CACHE:
        _CACHE[key] = _run(form, waves, ocp.problem("aug" if form == "aug" else "s", N, inst))
    return _CACHE[key]


@pytest.mark.parametrize("waves,N", SHAPES, ids=[f"wg{w}-N{n}" for w, n in SHAPES])
@pytest.mark.parametrize("form", ("aug", "s", "sp"))
def test_engine_against_dense_solve(form, waves, N):
    pform = "aug" if form == "aug" else "s"
    tol = ocp.tolerance(pform, N)
    worst = worst_p = 0.0
    for inst in range(ocp.INSTANCES):
        out, per = _device(form, waves, N, inst)
        assert np.all(out["ok"] == 1), "the sweep's flag of an unmodified instance"
        for half, got in enumerate(per):
            ref = ocp.dense_reference(pform, N, inst, half)
            worst = max(worst, ocp.rel_err(got, ref))
            if form != "aug":        # G_0's Schur complement on u is the value function of node 0
                lay = ocp.layout("s", waves)
                P0 = ocp.value_of_g(ocp.unpack_g("s", waves, out["G"], lay["nmaxs"] * half), lay["nxa"], lay["nu"])
                worst_p = max(worst_p, float(np.max(np.abs(P0 - ref["Pt0"])) / np.max(np.abs(ref["Pt0"]))))
    print(f"{form} wg{waves} N = {N}: dx/du/lam error {worst:.3e} = {worst / tol:.3f} of the tolerance {tol:.3e}"
          + (f"; Pt_0 error {worst_p:.3e} = {worst_p / tol:.3f}" if form != "aug" else ""))
    assert worst <= tol
    assert worst_p <= tol


@pytest.mark.parametrize("N", ocp.TWO_WAVE_SMALL_N)
@pytest.mark.parametrize("form", ("aug", "s", "sp"))
def test_one_and_two_wave_builds_agree(form, N):
    """N <= 31 runs in either build: the two agree to the shape's tolerance (bit equality is recorded, not required)."""
    tol = ocp.tolerance("aug" if form == "aug" else "s", N)
    same = True
    for inst in range(ocp.INSTANCES):
        (_, a), (_, b) = _device(form, 1, N, inst), _device(form, 2, N, inst)
        for ga, gb in zip(a, b):
            assert ocp.rel_err(ga, gb) <= tol
            same = same and all(np.array_equal(ga[q], gb[q]) for q in ("dx", "du", "lam"))
    print(f"{form} N = {N}: one-wave and two-wave results bit-identical: {same}")


@pytest.mark.parametrize("waves,N", FLAG_SHAPES, ids=[f"wg{w}-N{n}" for w, n in FLAG_SHAPES])
@pytest.mark.parametrize("form", ("aug", "s", "sp"))
def test_inertia_flag(form, waves, N):
    """A negative Quu at node 0, a middle node (and node 32 beyond the split) or node N - 1: the sweep returns false
    in every wave and lane; on the two-subsystem form either half alone.  The unmodified instance returns true."""
    pform = "aug" if form == "aug" else "s"
    subs = ocp.problem(pform, N, 0)
    assert np.all(_device(form, waves, N, 0)[0]["ok"] == 1)
    for node in ocp.flag_nodes(N):
        for half in range(len(subs)):
            mod = list(subs)
            mod[half] = ocp.with_negative_quu(subs[half], node)
            ok = _run(form, waves, tuple(mod))[0]["ok"]
            assert np.all(ok == 0), f"node {node}, half {half}: flags {ok}"
