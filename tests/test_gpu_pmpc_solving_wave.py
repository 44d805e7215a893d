"""The solving wave of the overlapped PMPC builds between barriers B and A (pmpc_ipm.hip, OVL) against
the one-wave builds.

After barrier B the solving wave reads the helper waves' verdict as one 16-byte record (the factor wave's use_scan and
ok in one word, the evaluation wave's converged and mu-decreased in another, the updated mu in the last two) beside
the six factor rows, and takes its scalars once every read is issued.  Nothing that is computed changes, so every
comparison is np.array_equal against the one-wave builds (DART_PMPC_OVERLAP=0) of the same library: there is no
tolerance.

What the cases aim at: every bit of the record on both overlapped builds.  Both ends of both builds' N ranges at
B = 1 and B = 32, at tol 1e-8 and 1e-11 (mu run down to its floor: many rounds with mu decreased, the converged bit
at the end), on the default tilt box (about half of the instances end with u0 at the tilt bound, half inside it: the
fractions to the boundary bind in some iterations and not in others) and on the wide box with far targets (rejected
first trials: a verdict dropped unread, then the accepted point's).  A tight tilt box (+-0.05) with far targets, where
every instance ends at the bound and the primal fraction binds for many iterations.  max_iter 1 and 2 (the exit right
after a hand-over, the record of the last round unread), a warm start from the converged point (the converged bit in
the start point's round), max_soc 0 and 4 and the restoration phases off and on on the wide box (failed line searches,
the fused tail), and launches back to back (nothing of the record leaks from launch to launch).

The knob is read once per process, so every setting runs in a fresh child process (this file run as a script), one
after the other, and hands its arrays back as .npy files.  Preconditions are asserted from the C oracle alone, on the
CPU.
"""
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, inputs as _inputs, wide_inputs as _wide_inputs

NS = (16, 23, 24, 31)       # both overlapped builds at both ends of their N ranges (SHORT2: 16..23, full scan: 24..31)
BS = (1, 32)
TOLS = (1e-8, 1e-11)
NS_TIGHT = (16, 20, 31)
NS_ORACLE = (16, 20, 31)
MAX_ITERS = (1, 2)
B2B = 50
GRID = [(kind, N, B, t) for kind in ("def", "wide") for N in NS for B in BS for t in range(len(TOLS))]
OPTS = [(soc, r) for soc in (0, 4) for r in (0, 1)]
CASES = ([f"{kind}_n{N}_b{B}_t{t}" for kind, N, B, t in GRID] + [f"tight_n{N}" for N in NS_TIGHT] +
         [f"devbox_n{N}" for N in NS_ORACLE] + [f"maxit{m}" for m in MAX_ITERS] + ["cold", "warm"] +
         [f"opts_soc{soc}_r{r}" for soc, r in OPTS])


def _tight_inputs():
    """inputs() with the tilt box set to +-0.05 and the far targets of wide_inputs()."""
    S, T, P = _inputs()
    P = P.copy(); P[:, 4] = -0.05; P[:, 5] = 0.05
    T = T.copy(); T[:, 0] = np.where(S[:, 0] > 0, -0.6, 0.6); T[:, 2] = np.where(S[:, 2] > 0, -0.5, 0.5)
    return S, T, P


def _wide32():
    """wide_inputs() (18 instances), its rows cycled to 32."""
    return tuple(np.resize(a, (32,) + a.shape[1:]) for a in _wide_inputs())


def _at_bound(u0, P):
    """Per instance: a component of u0 within 1e-6 of the tilt box's lower or upper bound."""
    d = np.minimum(np.abs(u0 - P[:, 4:5]), np.abs(u0 - P[:, 5:6]))
    return d.min(axis=1) < 1e-6


def _child(outdir):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir."""
    import dart_mpc

    def save(case, out):
        H.save(outdir, case, out)

    data = {"def": _inputs(), "wide": _wide32()}
    for kind, N, B, t in GRID:
        S, T, P = data[kind]
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=TOLS[t], B_max=B)
        save(f"{kind}_n{N}_b{B}_t{t}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
        s.close()
    S, T, P = _tight_inputs()
    for N in NS_TIGHT:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=32)
        save(f"tight_n{N}", s.solve_batch(S, T, P, want_w=True))
        s.close()
    S, T, P = _inputs()
    for N in NS_ORACLE:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=32)
        save(f"devbox_n{N}", s.solve_batch(S, T, P, want_w=True))
        s.close()
    S18, T18, P18 = S[:18], T[:18], P[:18]
    for m in MAX_ITERS:
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_iter=m)
        save(f"maxit{m}", s.solve_batch(S18, T18, P18, want_w=True))
        s.close()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18)
    cold = s.solve_batch(S18, T18, P18, want_w=True)
    save("cold", cold)
    save("warm", s.solve_batch(S18, T18, P18, w_warm=cold["w"], want_w=True))
    s.close()
    # the wide box at N = 20, B = 18: the correction passes off and on, the restoration phases off (the non-fused
    # kernel) and on (the fused one); 50 launches back to back at max_soc = 0 on one stream, no synchronisation
    Sw, Tw, Pw = _wide_inputs()
    nw = cold["w"].shape[1]
    for soc, r in OPTS:
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_soc=soc, restoration=bool(r))
        save(f"opts_soc{soc}_r{r}", s.solve_batch(Sw, Tw, Pw, want_w=True))
        if soc == 0:
            save(f"b2b_r{r}", H.back_to_back(s, Sw, Tw, Pw, nw, B2B))
        s.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    return H.run_settings(tmp_path_factory, __file__, "solwave")


@pytest.fixture(scope="module")
def oracle_runs():
    """The C oracle at tol 1e-8 on the 32 harness instances: {("def" | "tight", N): (dict, params)}."""
    import oracle_lib
    res = {}
    for kind, (S, T, P), ns in (("def", _inputs(), NS_ORACLE), ("tight", _tight_inputs(), NS_TIGHT)):
        for N in ns:
            res[(kind, N)] = (oracle_lib.solve_batch(S, T, P, N=N, tol=1e-8, Ts=0.002, max_iter=3000, nthreads=8), P)
    return res


@pytest.mark.parametrize("N", NS_ORACLE)
def test_default_box_ends_at_the_bound_for_about_half_of_the_instances(oracle_runs, N):
    """Precondition, from the C oracle alone: every instance converges, at least 12 of the 32 end with u0 at the tilt
    bound and at least 10 inside the box, so the primal fraction's test meets binding and non-binding iterations."""
    o, P = oracle_runs[("def", N)]
    at = int(np.sum(_at_bound(o["u0"], P)))
    print(N, "status 0:", int(np.sum(o["status"] == 0)), "at a bound:", at, "iterations:", o["iters"].min(), o["iters"].max())
    assert np.all(o["status"] == 0), o["status"]
    assert at >= 12 and 32 - at >= 10, at


@pytest.mark.parametrize("N", NS_TIGHT)
def test_tight_box_ends_at_the_bound_for_every_instance(oracle_runs, N):
    """Precondition, from the C oracle alone: every instance converges with u0 at the tilt bound."""
    o, P = oracle_runs[("tight", N)]
    at = int(np.sum(_at_bound(o["u0"], P)))
    print(N, "status 0:", int(np.sum(o["status"] == 0)), "at a bound:", at, "iterations:", o["iters"].min(), o["iters"].max())
    assert np.all(o["status"] == 0), o["status"]
    assert at == 32, at


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_solving_wave_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N", [("def", N) for N in NS_ORACLE] + [("tight", N) for N in NS_TIGHT])
def test_status_and_iterations_equal_the_oracles(runs, oracle_runs, kind, N):
    """The overlapped kernels take the C oracle's iterations on the preconditions' inputs."""
    o, _ = oracle_runs[(kind, N)]
    r = runs["default"]
    case = f"devbox_n{N}" if kind == "def" else f"tight_n{N}"
    assert np.array_equal(r[f"{case}__status"], o["status"]), (r[f"{case}__status"], o["status"])
    assert np.array_equal(r[f"{case}__iters"], o["iters"]), (r[f"{case}__iters"], o["iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("m", MAX_ITERS)
def test_short_loops_exit_right_after_a_hand_over(runs, m):
    """max_iter = 1, 2: status -1 and iters = max_iter for every instance."""
    r = runs["default"]
    assert np.all(r[f"maxit{m}__status"] == -1), r[f"maxit{m}__status"]
    assert np.all(r[f"maxit{m}__iters"] == m), r[f"maxit{m}__iters"]


@pytest.mark.gpu
def test_warm_start_ends_in_the_start_points_round(runs):
    """From the converged point the solve ends within the first rounds, sooner than the cold start."""
    r = runs["default"]
    assert np.all(r["warm__status"] == 0), r["warm__status"]
    assert np.all(r["warm__iters"] < r["cold__iters"]), (r["warm__iters"], r["cold__iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "0"])
@pytest.mark.parametrize("resto", [0, 1])
def test_back_to_back_launches_give_equal_outputs(runs, setting, resto):
    """50 launches of the wide case at N = 20, B = 18, max_soc = 0 on one stream without synchronisation, non-fused
    and fused: every launch gives the outputs of the first, which are those of the blocking call."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b_r{resto}__{k}"]
        assert x.shape[0] == B2B
        for i in range(1, B2B):
            assert np.array_equal(x[i], x[0]), (k, i)
        assert np.array_equal(x[0], r[f"opts_soc0_r{resto}__{k}"]), k


if __name__ == "__main__":
    _child(sys.argv[1])
