"""The overlapped PMPC builds (pmpc_ipm.hip, OVL: a second wave factors the Riccati scan of the point while the
solving wave evaluates it) against the one-wave builds of the same library.

Batches of at most 32 at N = 16..31 take the overlapped builds; DART_PMPC_OVERLAP=0 selects the one-wave builds
everywhere.  The knob is read once per process, so every setting runs in a fresh child process (this file run as
a script), one after the other, and hands its arrays back as .npy files.  The factor wave runs the arithmetic of
the one-wave build on the same operands, so every comparison is np.array_equal: there is no tolerance.
"""
import os
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from pmpc_overlap_harness import KEYS, wide_inputs as _wide_inputs

pytestmark = pytest.mark.gpu

# the smallest and largest N of the two overlapped builds (SHORT2: 16..23, full scan: 24..31) and the C2 horizon;
# B = 33 is the first batch that must take the one-wave path (the launcher's condition)
SHAPES = [(N, B) for N in (16, 20, 23, 24, 31) for B in (1, 18, 32)] + [(20, 33)]
CASES = [f"n{N}_b{B}" for N, B in SHAPES] + ["warm", "mult_init_off", "resto", "wide"]
B2B = 50


def _resto_pool():
    from dart_mpc.workload import pmpc_batch
    return pmpc_batch(n_seeds=64, seed0=300000)


def _child(outdir):
    """Every case on the GPU with this process's DART_PMPC_OVERLAP; <case>__<key>.npy into outdir."""
    import dart_mpc
    from dart_mpc.workload import pmpc_batch

    def save(case, out):
        H.save(outdir, case, out)

    S2, T2, P2 = pmpc_batch(2)
    for N, B in SHAPES:
        s = dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=B)
        save(f"n{N}_b{B}", s.solve_batch(S2[:B], T2[:B], P2[:B], want_w=True))
        s.close()
    S, T, P = S2[:18], T2[:18], P2[:18]
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18)
    first = s.solve_batch(S, T, P, want_w=True)
    save("warm", s.solve_batch(S, T, P, w_warm=first["w"], want_w=True))
    # back-to-back launches of the C2 shape on one stream, no synchronisation between them
    save("b2b", H.back_to_back(s, S, T, P, first["w"].shape[1], B2B))
    s.close()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, constr_mult_init_max=0.0)
    save("mult_init_off", s.solve_batch(S, T, P, want_w=True))
    s.close()
    # C4's seeds with the correction off: about one instance in ten fails the filter line search.  Those are
    # found with the restoration phases off (1152 instances: the one-wave build under either setting), then a
    # batch of 18 holding two of them runs with the phases on (in the solving wave: stop, the tail, its barriers)
    Sr, Tr, Pr = _resto_pool()
    off = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=Sr.shape[0], max_soc=0, restoration=False)
    st_off = off.solve_batch(Sr, Tr, Pr)["status"]
    off.close()
    hard, easy = np.flatnonzero(st_off == -2), np.flatnonzero(st_off == 0)
    sel = np.concatenate([hard[:2], easy[:16]])
    np.save(os.path.join(outdir, "resto__sel.npy"), sel)
    np.save(os.path.join(outdir, "resto__nhard.npy"), np.array([hard.size]))
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-8, B_max=18, max_soc=0)
    save("resto", s.solve_batch(Sr[sel], Tr[sel], Pr[sel], want_w=True))
    s.close()
    Sw, Tw, Pw = _wide_inputs()
    s = dart_mpc.Solver(N=20, Ts=0.002, tol=1e-11, B_max=18)
    save("wide", s.solve_batch(Sw, Tw, Pw, want_w=True))
    s.close()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {name: array}} of a fresh child per setting: "0" (one-wave builds) and "default" (overlap on)."""
    return H.run_settings(tmp_path_factory, __file__, "ovl")


@pytest.mark.parametrize("case", CASES)
def test_overlapped_build_equals_one_wave_build(runs, case):
    """u0, f, status, iters and the full w of every case, bit for bit: cold starts at both ends of each
    overlapped build's N range with B = 1, 18, 32 (and B = 33, one-wave either way), a warm start, the
    least-square multiplier estimate off, a batch with restored instances (max_soc = 0) and the wide tilt box."""
    a, b = runs["0"], runs["default"]
    for k in KEYS:
        assert np.array_equal(a[f"{case}__{k}"], b[f"{case}__{k}"]), (case, k)
    if case not in ("resto",):
        assert np.all(b[f"{case}__status"] == 0), b[f"{case}__status"]


def test_restored_instances_in_the_overlapped_kernel_match_oracle(runs):
    """The batch of 18 with two instances handed over to the restoration phases inside the overlapped kernel
    (the exit funnel, then pmpc_resto_tail with the factor wave gone): statuses equal to the C oracle's."""
    import oracle_lib
    r = runs["default"]
    assert int(r["resto__nhard"][0]) >= 2
    Sr, Tr, Pr = _resto_pool()
    sel = r["resto__sel"]
    kw = dict(N=20, Ts=0.002, tol=1e-8, max_iter=3000, nthreads=8, soc=0, want_w=False)
    off = oracle_lib.solve_batch(Sr[sel], Tr[sel], Pr[sel], resto=False, **kw)
    assert np.all(off["status"][:2] == -2), off["status"]          # the oracle hands the same two over
    o = oracle_lib.solve_batch(Sr[sel], Tr[sel], Pr[sel], **kw)
    assert np.array_equal(r["resto__status"], o["status"]), (r["resto__status"], o["status"])
    assert np.array_equal(runs["0"]["resto__sel"], sel)


def test_wide_tilt_box_in_the_overlapped_kernel_matches_oracle(runs):
    import oracle_lib
    Sw, Tw, Pw = _wide_inputs()
    r = runs["default"]
    ref = oracle_lib.solve_batch(Sw, Tw, Pw, N=20, Ts=0.002, tol=1e-11, nthreads=8, want_w=False)
    assert np.array_equal(r["wide__status"], ref["status"])
    assert np.max(np.abs(r["wide__w"][:, 6 * 21:])) > 1.0          # the library trig path was exercised
    assert np.max(np.abs(r["wide__u0"] - ref["u0"])) <= 1e-6       # (the bound of the test the inputs come from)


@pytest.mark.parametrize("setting", ["default", "0"])
def test_back_to_back_launches_give_equal_outputs(runs, setting):
    """50 launches of the C2 shape on one stream without synchronisation, the same inputs: every launch gives the
    outputs of the first (nothing leaks through LDS from launch to launch), which are those of the blocking call."""
    r = runs[setting]
    for k in KEYS:
        x = r[f"b2b__{k}"]
        assert x.shape[0] == B2B
        for i in range(1, B2B):
            assert np.array_equal(x[i], x[0]), (k, i)
        assert np.array_equal(x[0], r[f"n20_b18__{k}"]), k


if __name__ == "__main__":
    _child(sys.argv[1])
