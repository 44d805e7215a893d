"""The evaluation wave of the overlapped PMPC builds (pmpc_ipm.hip, OVL) against the one-wave builds.

In the overlapped builds a third wave forms the optimality-error measures of every handed-over point, tests
convergence and runs the monotone mu update; the solving wave takes "converged", the new mu and "mu decreased" with
the factors after barrier B.  Nothing that is computed changes, so every comparison is np.array_equal against the
one-wave builds (DART_PMPC_OVERLAP=0) of the same library: there is no tolerance.

The cases aim at what the evaluation wave decides: convergence while mu is still large (tol 1e-4) and with mu run
down to its floor (tol 1e-11) beside the default, at both ends of both builds' N ranges, at B = 1 and B = 32, in the
fused (restoration on) and the non-fused kernels; loops of no, one and two Newton iterations; a warm start from the
converged point (several mu decreases in one evaluation, convergence within the first rounds); accepted correction
passes (a verdict dropped with the rejected trial point, then convergence after the miss); launches back to back.

The knob is read once per process, so every setting runs in a fresh child process (this file run as a script), one
after the other, and hands its arrays back as .npy files.  Preconditions are asserted from the C oracle alone, on
the CPU, where it can show them.  It cannot show mu itself (it returns status and iteration counts), so "mu still
large" and "mu at its floor" stand on the iteration counts only: every instance converges sooner at 1e-4 and most go
on longer at 1e-11.  It takes no warm start either, so the warm case has no oracle precondition; the test asserts on
the GPU that it converges, and sooner than the cold start.
"""
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, inputs as _inputs

# both overlapped builds at both ends of their N ranges (SHORT2: 16..23, full scan: 24..31)
NS = (16, 23, 24, 31)
TOLS = (1e-4, 1e-8, 1e-11)
GRID = [(N, B, r, t) for N in NS for B in (1, 32) for r in (0, 1) for t in range(len(TOLS))]
SOC4 = [(N, 32) for N in (20, 31)]
MAX_ITERS = (0, 1, 2)
B2B = 50
CASES = ([f"n{N}_b{B}_r{r}_t{t}" for N, B, r, t in GRID] + [f"soc4_n{N}_b{B}" for N, B in SOC4] +
         [f"maxit{m}" for m in MAX_ITERS] + ["cold", "warm"])


def _child(outdir):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir."""
    import dart_mpc

    def save(case, out):
        H.save(outdir, case, out)

    S, T, P = _inputs()
    for N, B, r, t in GRID:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=TOLS[t], B_max=B, restoration=bool(r))
        save(f"n{N}_b{B}_r{r}_t{t}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
        s.close()
    for N, B in SOC4:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B, max_soc=4)
        save(f"soc4_n{N}_b{B}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
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
    # back-to-back launches at N = 20, B = 18 on one stream, no synchronisation between them: the non-fused
    # (restoration off) and the fused (restoration on) kernels
    nw = cold["w"].shape[1]
    for r in (0, 1):
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, restoration=bool(r))
        save(f"b2b_ref_r{r}", s.solve_batch(S18, T18, P18, want_w=True))
        save(f"b2b_r{r}", H.back_to_back(s, S18, T18, P18, nw, B2B))
        s.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    return H.run_settings(tmp_path_factory, __file__, "evalwave")


@pytest.fixture(scope="module")
def oracle_runs():
    """The C oracle on the 32 instances: {(N, tol index, soc): dict(status, iters)} (restoration phases off; with
    correction passes none of these line searches fails, so on or off they give the same iterates)."""
    import oracle_lib
    S, T, P = _inputs()
    kw = dict(Ts=0.002, max_iter=3000, nthreads=8, want_w=False, resto=False)
    res = {(N, t, 4): oracle_lib.solve_batch(S, T, P, N=N, tol=TOLS[t], soc=4, **kw) for N in NS for t in range(3)}
    for N, _ in SOC4:
        for soc in (0, 4):
            res[(N, 1, soc)] = oracle_lib.solve_batch(S, T, P, N=N, tol=1e-8, soc=soc, **kw)
    return res


@pytest.mark.parametrize("N", NS)
def test_tolerances_end_the_solve_at_different_iterations(oracle_runs, N):
    """Precondition, from the C oracle alone: all 32 instances converge at each tolerance; each converges sooner at
    1e-4 than at 1e-8 (mu has not reached its floor), and more than half go on longer at 1e-11."""
    it = [oracle_runs[(N, t, 4)]["iters"] for t in range(3)]
    print(N, "iters sums", [int(x.sum()) for x in it], "longer at 1e-11:", int(np.sum(it[2] > it[1])))
    for t in range(3):
        assert np.all(oracle_runs[(N, t, 4)]["status"] == 0), (t, oracle_runs[(N, t, 4)]["status"])
    assert np.all(it[0] < it[1]), (it[0], it[1])
    assert int(np.sum(it[2] > it[1])) > 16, (it[1], it[2])


@pytest.mark.parametrize("N", [n for n, _ in SOC4])
def test_correction_passes_are_accepted(oracle_runs, N):
    """Precondition, from the C oracle alone: the correction passes change the iteration count of at least three of
    the 32 instances, so corrected steps are accepted (misses of the speculative hand-over)."""
    s0, s4 = oracle_runs[(N, 1, 0)], oracle_runs[(N, 1, 4)]
    print(N, "iters differ:", int(np.sum(s0["iters"] != s4["iters"])))
    assert int(np.sum(s0["iters"] != s4["iters"])) >= 3, (s0["iters"], s4["iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_three_wave_build_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_every_tolerance_converges(runs, N):
    """B = 1 and B = 32, non-fused and fused kernels: status 0 for every instance at every tolerance, and every
    instance stops sooner at 1e-4 than at 1e-8 (the evaluation wave's convergence test, not max_iter, ends it)."""
    r = runs["default"]
    for B in (1, 32):
        for rs in (0, 1):
            for t in range(3):
                assert np.all(r[f"n{N}_b{B}_r{rs}_t{t}__status"] == 0), (B, rs, t, r[f"n{N}_b{B}_r{rs}_t{t}__status"])
            assert np.all(r[f"n{N}_b{B}_r{rs}_t0__iters"] < r[f"n{N}_b{B}_r{rs}_t1__iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("m", MAX_ITERS)
def test_short_loops_leave_through_the_funnel(runs, m):
    """max_iter = 0, 1, 2: no Newton iteration at all (the helper waves meet the stop barrier first), and the exit
    right after the start point's round and the next; status -1 and iters = max_iter for every instance."""
    r = runs["default"]
    assert np.all(r[f"maxit{m}__status"] == -1), r[f"maxit{m}__status"]
    assert np.all(r[f"maxit{m}__iters"] == m), r[f"maxit{m}__iters"]


@pytest.mark.gpu
def test_warm_start_converges_within_the_first_rounds(runs):
    r = runs["default"]
    assert np.all(r["warm__status"] == 0), r["warm__status"]
    assert np.all(r["warm__iters"] < r["cold__iters"]), (r["warm__iters"], r["cold__iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "0"])
@pytest.mark.parametrize("resto", [0, 1])
def test_back_to_back_launches_give_equal_outputs(runs, setting, resto):
    """50 launches at N = 20, B = 18 on one stream without synchronisation, non-fused and fused: every launch gives
    the outputs of the first (nothing leaks through LDS from launch to launch), which are those of the blocking
    call."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b_r{resto}__{k}"]
        assert x.shape[0] == B2B
        for i in range(1, B2B):
            assert np.array_equal(x[i], x[0]), (k, i)
        assert np.array_equal(x[0], r[f"b2b_ref_r{resto}__{k}"]), k


if __name__ == "__main__":
    _child(sys.argv[1])
