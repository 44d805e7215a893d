"""What the solving wave of the overlapped PMPC builds (pmpc_ipm.hip, OVL) takes off its scans and carries from
iteration to iteration, against the one-wave builds.

The cases are those drawn up for handing the matrix halves of direction()'s two affine scans to the factor wave
(built, measured slower, not kept).  What is kept rests on the same properties and is caught by the
same cases: the z scan's per-level multipliers are lane constants of the launch, formed once before the loop, so
every direction() call of every kind (the first of an iteration, the in-wave fallback, the correction passes, the
Newton step again) must see the products its own levels would form, at every N, since which lanes are final after
which level changes with N; and the barrier logarithm of the current point is carried from the accepted trial,
whichever trial that was (the first, a backtracked one, a correction pass), instead of being evaluated again.
Nothing that is computed changes, so every comparison is np.array_equal against the one-wave builds
(DART_PMPC_OVERLAP=0) of the same library: there is no tolerance.

The knob is read once per process, so every setting runs in a fresh child process (this file run as a script), one
after the other, and hands its arrays back as .npy files.  The preconditions are asserted from the C oracle alone,
on the CPU.  What the oracle cannot show is whether the warm-started wide-box case really leaves the scan path in
the factor wave (the oracle has no warm start); that case is compared all the same.
"""
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, inputs as _inputs, wide_inputs as _wide_inputs

# every N of the overlapped builds: which lanes are final after which level changes with N, and 23 / 24 is the
# boundary between the SHORT2 and the full-scan instantiations
NS = tuple(range(16, 32))
B1 = 3
NS_SOC = (20, 31)
B2B = 5
CASES = ([f"n{N}_r{r}" for N in NS for r in (0, 1)] + [f"soc4_n{N}" for N in NS_SOC] + ["wide", "wide_warm"])


def _child(outdir, bsoc):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir.  bsoc: the batch
    sizes of the correction-pass cases, one per N of NS_SOC (the parent takes them from the oracle)."""
    import dart_mpc

    def save(case, out):
        H.save(outdir, case, out)

    S, T, P = _inputs()
    for N in NS:
        for r in (0, 1):
            s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B1, restoration=bool(r))
            save(f"n{N}_r{r}", s.solve_batch(S[:B1], T[:B1], P[:B1], want_w=True))
            s.close()
    for N, B in zip(NS_SOC, bsoc):
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B, max_soc=4)
        save(f"soc4_n{N}", s.solve_batch(S[:B], T[:B], P[:B], want_w=True))
        s.close()
    Sw, Tw, Pw = _wide_inputs()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-11, B_max=18)
    first = s.solve_batch(Sw, Tw, Pw, want_w=True)
    save("wide", first)
    save("wide_warm", s.solve_batch(Sw, Tw, Pw, w_warm=first["w"], want_w=True))
    s.close()
    # back-to-back launches at N = 20, B = 18 on one stream, no synchronisation between them
    S18, T18, P18 = S[:18], T[:18], P[:18]
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18)
    ref = s.solve_batch(S18, T18, P18, want_w=True)
    save("b2b_ref", ref)
    save("b2b", H.back_to_back(s, S18, T18, P18, ref["w"].shape[1], B2B))
    s.close()


@pytest.fixture(scope="module")
def oracle_soc():
    """The C oracle on the 32 instances without the restoration phases: {(N, soc): dict(status, iters)}."""
    import oracle_lib
    S, T, P = _inputs()
    kw = dict(Ts=0.002, tol=1e-8, max_iter=3000, nthreads=8, want_w=False, resto=False)
    return {(N, soc): oracle_lib.solve_batch(S, T, P, N=N, soc=soc, **kw) for N in NS_SOC for soc in (0, 4)}


def _soc_prefix(oracle_soc, N):
    """The smallest prefix of the 32 instances in which the correction passes change an iteration count (so the
    oracle runs an iteration with a correction in it), the way test_gpu_pmpc_speculative.py takes it."""
    differ = np.nonzero(oracle_soc[(N, 0)]["iters"] != oracle_soc[(N, 4)]["iters"])[0]
    assert differ.size >= 1, (N, oracle_soc[(N, 0)]["iters"], oracle_soc[(N, 4)]["iters"])
    return int(differ[0]) + 1


@pytest.fixture(scope="module")
def runs(tmp_path_factory, oracle_soc):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    bsoc = [str(_soc_prefix(oracle_soc, N)) for N in NS_SOC]
    return H.run_settings(tmp_path_factory, __file__, "scan", bsoc)


@pytest.mark.parametrize("N", NS)
def test_every_horizon_iterates(N):
    """Precondition of the per-N cases, from the C oracle alone: the three instances converge after several Newton
    iterations at every N, so the carried values are used more than once."""
    import oracle_lib
    S, T, P = _inputs()
    ref = oracle_lib.solve_batch(S[:B1], T[:B1], P[:B1], N=N, Ts=0.002, tol=1e-8, max_iter=3000, want_w=False)
    print(N, "status", ref["status"].tolist(), "iters", ref["iters"].tolist())
    assert np.all(ref["status"] == 0), ref["status"]
    assert np.all(ref["iters"] >= 3), ref["iters"]


@pytest.mark.parametrize("N", NS_SOC)
def test_inputs_run_correction_passes(oracle_soc, N):
    """Precondition of the correction-pass cases, from the C oracle alone: the correction passes change the
    iteration count of at least one of the 32 instances, and the prefix ends at the first of them."""
    B = _soc_prefix(oracle_soc, N)
    s0, s4 = oracle_soc[(N, 0)], oracle_soc[(N, 4)]
    print(N, "prefix", B, "iters soc0", s0["iters"][:B].tolist(), "soc4", s4["iters"][:B].tolist())
    assert 1 <= B <= 32
    assert s0["iters"][B - 1] != s4["iters"][B - 1]
    assert np.array_equal(s0["iters"][:B - 1], s4["iters"][:B - 1])


def test_wide_inputs_leave_the_polynomial_trig_range():
    """Precondition of the fallback case, from the C oracle alone: the wide-box instances converge at tol 1e-11
    with tilt angles beyond 1 rad."""
    import oracle_lib
    Sw, Tw, Pw = _wide_inputs()
    ref = oracle_lib.solve_batch(Sw, Tw, Pw, N=20, Ts=0.002, tol=1e-11, max_iter=3000, nthreads=8)
    assert np.all(ref["status"] == 0), ref["status"]
    assert np.max(np.abs(ref["w"][:, 6 * 21:])) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_scan_handover_build_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_every_horizon_converges_on_the_gpu(runs, N):
    """Both kernels of every N (fused and not) end the three instances at status 0."""
    for r in (0, 1):
        st = runs["default"][f"n{N}_r{r}__status"]
        assert np.all(st == 0), (N, r, st)


@pytest.mark.gpu
def test_warm_start_of_the_wide_box_converges(runs):
    r = runs["default"]
    assert np.all(r["wide__status"] == 0), r["wide__status"]
    assert np.all(r["wide_warm__status"] == 0), r["wide_warm__status"]
    assert np.max(np.abs(r["wide_warm__w"][:, 6 * 21:])) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "0"])
def test_back_to_back_launches_equal_a_single_launch(runs, setting):
    """Five launches at N = 20, B = 18 on one stream without synchronisation: every launch gives the outputs of the
    blocking single launch (nothing carried by one launch is seen by the next)."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b__{k}"]
        assert x.shape[0] == B2B
        for i in range(B2B):
            assert np.array_equal(x[i], r[f"b2b_ref__{k}"]), (k, i)


if __name__ == "__main__":
    _child(sys.argv[1], [int(x) for x in sys.argv[2:]])
