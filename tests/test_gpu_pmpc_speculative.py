"""The speculative hand-over of the overlapped PMPC builds (pmpc_ipm.hip, OVL) against the one-wave builds.

The solving wave hands the first line-search trial point (the Newton step at alpha = amax) to the factor wave before
it evaluates the trial.  Where that trial is accepted the update crosses no barrier (a hit); a backtracked step, an
accepted correction pass or the Newton step again after failed passes drops the speculated factors and hands the
accepted point over (a miss); a failed line search, max_iter and convergence leave through the exit funnel with a
speculated point outstanding.  Nothing that is computed changes, so every comparison is np.array_equal against the
one-wave builds (DART_PMPC_OVERLAP=0) of the same library: there is no tolerance.

The knob is read once per process, so every setting runs in a fresh child process (this file run as a script), one
after the other, and hands its arrays back as .npy files.  The preconditions (that the inputs really take the miss
paths) are asserted from the C oracle alone, on the CPU.
"""
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, inputs as _inputs, wide_inputs as _wide_inputs

# both overlapped builds at both ends of their N ranges (SHORT2: 16..23, full scan: 24..31)
NS1 = (16, 23, 24, 31)
# case 1: max_soc = 0, without the restoration phases (the non-fused kernels, status -2 through the funnel) and with
# them (the fused kernels, the hand-over to pmpc_resto_tail); case 2: accepted correction passes
CASE1 = [(N, B, r) for N in NS1 for B in (1, 32) for r in (0, 1)]
CASE2 = [(N, 32) for N in (20, 31)]
MAX_ITERS = (1, 2, 3)
B2B = 50
CASES = ([f"soc0_n{N}_b{B}_r{r}" for N, B, r in CASE1] + [f"soc4_n{N}_b{B}" for N, B in CASE2] +
         [f"maxit{m}" for m in MAX_ITERS] + ["warm", "wide"])


def _child(outdir):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir."""
    import dart_mpc

    def save(case, out):
        H.save(outdir, case, out)

    S, T, P = _inputs()
    for N, B, r in CASE1:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B, max_soc=0, restoration=bool(r))
        save(f"soc0_n{N}_b{B}_r{r}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
        s.close()
    for N, B in CASE2:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B, max_soc=4)
        save(f"soc4_n{N}_b{B}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
        s.close()
    S18, T18, P18 = S[:18], T[:18], P[:18]
    for m in MAX_ITERS:
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_iter=m)
        save(f"maxit{m}", s.solve_batch(S18, T18, P18, want_w=True))
        s.close()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18)
    first = s.solve_batch(S18, T18, P18, want_w=True)
    save("warm", s.solve_batch(S18, T18, P18, w_warm=first["w"], want_w=True))
    s.close()
    Sw, Tw, Pw = _wide_inputs()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-11, B_max=18)
    save("wide", s.solve_batch(Sw, Tw, Pw, want_w=True))
    s.close()
    # back-to-back launches of case 1 at N = 20, B = 18 on one stream, no synchronisation between them
    nw = first["w"].shape[1]
    for r in (0, 1):
        s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_soc=0, restoration=bool(r))
        save(f"b2b_ref_r{r}", s.solve_batch(S18, T18, P18, want_w=True))
        save(f"b2b_r{r}", H.back_to_back(s, S18, T18, P18, nw, B2B))
        s.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    return H.run_settings(tmp_path_factory, __file__, "spec")


@pytest.fixture(scope="module")
def oracle_runs():
    """The C oracle on the 32 instances with the restoration phases off: {(N, soc): dict(status, iters)}."""
    import oracle_lib
    S, T, P = _inputs()
    kw = dict(Ts=0.002, tol=1e-8, max_iter=3000, nthreads=8, want_w=False, resto=False)
    return {(N, soc): oracle_lib.solve_batch(S, T, P, N=N, soc=soc, **kw) for N in NS1 for soc in (0, 4)}


@pytest.mark.parametrize("N", NS1)
def test_inputs_take_the_miss_paths(oracle_runs, N):
    """Preconditions, from the C oracle alone: at max_soc = 0 and without the restoration phases at least two of the
    32 instances end in a failed line search (status -2: the exit funnel with a speculated point outstanding), and
    the correction passes change the iteration count of at least three (so first trials are rejected: backtracked
    accepts at max_soc = 0, accepted correction passes at max_soc = 4)."""
    s0, s4 = oracle_runs[(N, 0)], oracle_runs[(N, 4)]
    print(N, "status -2:", int(np.sum(s0["status"] == -2)), "iters differ:", int(np.sum(s0["iters"] != s4["iters"])))
    assert int(np.sum(s0["status"] == -2)) >= 2, s0["status"]
    assert int(np.sum(s0["iters"] != s4["iters"])) >= 3, (s0["iters"], s4["iters"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_speculative_build_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS1)
def test_failed_line_searches_leave_through_the_funnel(runs, N):
    """max_soc = 0 without the restoration phases, B = 32: the overlapped kernel too ends at least two instances at
    status -2, each with a speculated point outstanding."""
    st = runs["default"][f"soc0_n{N}_b32_r0__status"]
    assert int(np.sum(st == -2)) >= 2, st


@pytest.mark.gpu
@pytest.mark.parametrize("m", MAX_ITERS)
def test_max_iter_exit_after_a_speculated_hand_over(runs, m):
    """max_iter = 1, 2, 3: the exit at the loop head comes right after a speculated hand-over; status -1 and
    iters = max_iter for every instance."""
    r = runs["default"]
    assert np.all(r[f"maxit{m}__status"] == -1), r[f"maxit{m}__status"]
    assert np.all(r[f"maxit{m}__iters"] == m), r[f"maxit{m}__iters"]


@pytest.mark.gpu
def test_warm_start_exits_before_any_speculation(runs):
    r = runs["default"]
    assert np.all(r["warm__status"] == 0), r["warm__status"]


@pytest.mark.gpu
def test_wide_tilt_box_takes_the_library_trig_path(runs):
    r = runs["default"]
    assert np.all(r["wide__status"] == 0), r["wide__status"]
    assert np.max(np.abs(r["wide__w"][:, 6 * 21:])) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "0"])
@pytest.mark.parametrize("resto", [0, 1])
def test_back_to_back_launches_give_equal_outputs(runs, setting, resto):
    """50 launches at N = 20, B = 18, max_soc = 0 on one stream without synchronisation: every launch gives the
    outputs of the first (nothing leaks through LDS from launch to launch), which are those of the blocking call."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b_r{resto}__{k}"]
        assert x.shape[0] == B2B
        for i in range(1, B2B):
            assert np.array_equal(x[i], x[0]), (k, i)
        assert np.array_equal(x[0], r[f"b2b_ref_r{resto}__{k}"]), k


if __name__ == "__main__":
    _child(sys.argv[1])
