"""The split hand-over of the overlapped PMPC builds (pmpc_ipm.hip, OVL) against the one-wave builds.

The solving wave hands the first line-search trial point over with less than it used to form for it.  Of the
line-search preparation only the two fraction minima are reduced ahead of the hand-over; the sums, the tiny-step
maximum, lg_sw, amin and tiny are formed behind barrier A.  The sine of the trial angle is no row of the hand-over any
more: the first trial evaluates its own, and the factor wave and the evaluation wave form it from the handed-over
theta with the trial's own function and mask, for speculated points, for the start point and for every point
published after a rejected first trial.  Nothing that is computed changes, so every comparison is np.array_equal
against the one-wave builds (DART_PMPC_OVERLAP=0) of the same library: there is no tolerance.

What the cases aim at: the library trig path (tilt box +-1.2, `poly` false, where the helper waves' sine is the
library's and not the polynomial) at both overlapped builds, with first trials rejected (a publish() right after a
speculative hand-over) and line searches that fail (the funnel and the fused restoration tail after a speculative
hand-over); both ends of both builds' N ranges at B = 1 and B = 32 with mu run down to its floor; loops of no, one
and two Newton iterations (the exit right after a speculative hand-over, with the sums behind barrier A formed and
not used); a warm start from the converged point (the start point's round only); launches back to back.

The kappa_sigma clamp of the bound multipliers stays where it was: the solving wave evaluates it for the hand-over
and takes the values back on a hit (handing raw multipliers over for the helper waves to clamp was built, measured
slower and dropped).  The clamp almost never binds (its factors are 1e10 and 1e-10) and no oracle
precondition can show it binding, so this file does not claim to cover a binding clamp; the bit-for-bit comparison
is what holds the hand-over's statement of it and the update's together.

The knob is read once per process, so every setting runs in a fresh child process (this file run as a script), one
after the other, and hands its arrays back as .npy files.  Preconditions are asserted from the C oracle alone, on the
CPU.
"""
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, inputs as _inputs, wide_inputs as _wide_inputs

# the wide box: SHORT2 (16, 20, 23) and the full scan (24); N = 31 has no rejected first trial on these inputs
NS_WIDE = (16, 20, 23, 24)
TOLS = (1e-8, 1e-11)
WIDE = [(N, soc, r, t) for N in NS_WIDE for soc in (0, 4) for r in (0, 1) for t in range(len(TOLS))]
# both overlapped builds at both ends of their N ranges (SHORT2: 16..23, full scan: 24..31)
NS = (16, 23, 24, 31)
GRID = [(N, B) for N in NS for B in (1, 32)]
MAX_ITERS = (0, 1, 2)
B2B = 50
CASES = ([f"wide_n{N}_soc{soc}_r{r}_t{t}" for N, soc, r, t in WIDE] + [f"n{N}_b{B}" for N, B in GRID] +
         [f"maxit{m}" for m in MAX_ITERS] + ["cold", "warm"])


def _child(outdir):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir."""
    import dart_mpc

    def save(case, out):
        H.save(outdir, case, out)

    Sw, Tw, Pw = _wide_inputs()
    for N, soc, r, t in WIDE:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=TOLS[t], B_max=18, max_soc=soc, restoration=bool(r))
        save(f"wide_n{N}_soc{soc}_r{r}_t{t}", s.solve_batch(Sw, Tw, Pw, want_w=True))
        s.close()
    S, T, P = _inputs()
    for N, B in GRID:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-11, B_max=B)
        save(f"n{N}_b{B}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
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
    # back-to-back launches of the wide case at N = 20, B = 18, max_soc = 0 on one stream, no synchronisation between
    # them: the non-fused (restoration off) and the fused (restoration on) kernels
    nw = cold["w"].shape[1]
    for r in (0, 1):
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_soc=0, restoration=bool(r))
        save(f"b2b_ref_r{r}", s.solve_batch(Sw, Tw, Pw, want_w=True))
        save(f"b2b_r{r}", H.back_to_back(s, Sw, Tw, Pw, nw, B2B))
        s.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    return H.run_settings(tmp_path_factory, __file__, "hosplit")


@pytest.fixture(scope="module")
def oracle_runs():
    """The C oracle on the 18 wide-box instances with the restoration phases off: {(N, tol index, soc): dict}."""
    import oracle_lib
    S, T, P = _wide_inputs()
    kw = dict(Ts=0.002, max_iter=3000, nthreads=8, want_w=True, resto=False)
    return {(N, t, soc): oracle_lib.solve_batch(S, T, P, N=N, tol=TOLS[t], soc=soc, **kw)
            for N in NS_WIDE for t in range(len(TOLS)) for soc in (0, 4)}


@pytest.mark.parametrize("t", range(len(TOLS)))
@pytest.mark.parametrize("N", NS_WIDE)
def test_wide_inputs_reject_first_trials_on_the_library_trig_path(oracle_runs, N, t):
    """Preconditions, from the C oracle alone: the correction passes change the iteration count of at least two of
    the 18 instances (first trials are rejected, so a publish() follows a speculative hand-over), at least one
    instance ends in a failed line search at max_soc = 0 (status -2), and the solution leaves |theta| <= 1 (the
    library sine and cosine, not the polynomials)."""
    s0, s4 = oracle_runs[(N, t, 0)], oracle_runs[(N, t, 4)]
    differ, failed = int(np.sum(s0["iters"] != s4["iters"])), int(np.sum(s0["status"] == -2))
    th_max = float(np.max(np.abs(s4["w"][s4["status"] == 0][:, 6 * (N + 1):])))
    print(N, TOLS[t], "iters differ:", differ, "status -2:", failed, "max |theta|:", th_max)
    assert differ >= 2, (s0["iters"], s4["iters"])
    assert failed >= 1, s0["status"]
    assert th_max > 1.0, th_max


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_split_hand_over_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS_WIDE)
def test_wide_box_fails_line_searches_and_leaves_the_polynomial_range(runs, N):
    """The overlapped kernels on the wide box: at max_soc = 0 without the restoration phases at least one instance
    ends at status -2 (the funnel after a speculative hand-over), with the correction passes every instance
    converges, and the solution has |theta| > 1."""
    r = runs["default"]
    for t in range(len(TOLS)):
        assert int(np.sum(r[f"wide_n{N}_soc0_r0_t{t}__status"] == -2)) >= 1, r[f"wide_n{N}_soc0_r0_t{t}__status"]
        assert np.all(r[f"wide_n{N}_soc4_r0_t{t}__status"] == 0), r[f"wide_n{N}_soc4_r0_t{t}__status"]
        assert np.max(np.abs(r[f"wide_n{N}_soc4_r0_t{t}__w"][:, 6 * (N + 1):])) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("m", MAX_ITERS)
def test_short_loops_exit_right_after_a_hand_over(runs, m):
    """max_iter = 0, 1, 2: status -1 and iters = max_iter for every instance."""
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
    and fused: every launch gives the outputs of the first (nothing leaks through LDS from launch to launch), which
    are those of the blocking call."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b_r{resto}__{k}"]
        assert x.shape[0] == B2B
        for i in range(1, B2B):
            assert np.array_equal(x[i], x[0]), (k, i)
        assert np.array_equal(x[0], r[f"b2b_ref_r{resto}__{k}"]), k


if __name__ == "__main__":
    _child(sys.argv[1])
