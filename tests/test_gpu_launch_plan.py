"""The launch plan on a device: for PMPC calls on both sides of every N and B boundary, under the default knobs and three
knob settings, the library's own answer to "which build serves this call" (dartmpc_plan_query, internal) equals the
row of the host table (tests/test_launch_plan.py), and the call itself solves its instances as the same instances solved
one by one.

The knobs are read once per process, so every setting runs in a fresh child process (this file run as a script, with
the helpers of pmpc_overlap_harness.py).  A batch and its instances one by one run builds of the same arithmetic: the
same kernel, or the overlapped build against the one-wave build of the same scan, which tests/test_gpu_pmpc_overlap.py
holds bit for bit.  So every comparison is np.array_equal: there is no tolerance.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import pmpc_overlap_harness as H
from test_launch_plan import PMPC, fmt, pmpc_rows

pytestmark = pytest.mark.gpu

# setting -> (its name in the host table, the child's environment)
SETTINGS = {"default": ("default", {}), "ovl0": ("overlap=0", {"DART_PMPC_OVERLAP": "0"}),
            "occ2": ("occ2_min_b=1", {"DART_PMPC_OCC2_MIN_B": "1"}), "seq": ("qscan_max_b=0", {"DART_PMPC_QSCAN_MAX_B": "0"})}
# (N, B, reduced path, restoration): both sides of N = 15/16, 23/24, 31/32 and of B = 32/33; the reduced path's builds
SHAPES = ([(N, B, 0, r) for N in (15, 16, 23, 24, 31, 32) for B in (1, 32, 33) for r in (0, 1)] +
          [(N, 32, 1, 0) for N in (15, 20, 31, 40)])
OUT = ("u0", "f", "iters", "status")


def _name(N, B, red, r):
    return f"n{N}_b{B}_red{red}_r{r}"


def _resto_in(N, B, red, r):
    """PmpcArgs::resto of the host entry (dart_mpc_abi.hip host_resto_mode): IPOPT's path at N <= 31 with the phases
    on; in the solving wave's launch for B <= 32 (1), host-driven beyond (2)."""
    return (1 if B <= 32 else 2) if (r and not red and N <= 31) else 0


def _child(outdir):
    """Every shape with this process's knobs: plan__<shape>.npy (the ints of dartmpc_plan_query), <shape>__<key>.npy
    (the batch) and one__<N>_<red>_<r>__<key>.npy (the first 33 instances, each solved alone)."""
    import dart_mpc
    import dart_mpc._lib as L
    from dart_mpc.workload import pmpc_batch
    S2, T2, P2 = (a[:33] for a in pmpc_batch(2))
    lib = L.lib()
    lib.dartmpc_plan_query.restype = ctypes.c_int
    for N, red, r in sorted({(N, red, r) for N, _, red, r in SHAPES}):
        Bs = [B for n, B, rd, rr in SHAPES if (n, rd, rr) == (N, red, r)]
        with dart_mpc.Solver(N=N, Ts=0.002, tol=1e-8, B_max=33, path="reduced" if red else "ipopt",
                             restoration=bool(r)) as s:
            for B in Bs:
                q = (ctypes.c_int * 4)(N, B, red, _resto_in(N, B, red, r))
                o = (ctypes.c_int * 16)()
                n = lib.dartmpc_plan_query(PMPC, q, o)
                np.save(os.path.join(outdir, f"plan__{_name(N, B, red, r)}.npy"), np.array(o[:max(n, 0)]))
                out = s.solve_batch(S2[:B], T2[:B], P2[:B])
                for k in OUT:
                    np.save(os.path.join(outdir, f"{_name(N, B, red, r)}__{k}.npy"), np.array(out[k]))
            one = [s.solve_batch(S2[i:i + 1], T2[i:i + 1], P2[i:i + 1]) for i in range(max(Bs))]
            for k in OUT:
                np.save(os.path.join(outdir, f"one__{N}_{red}_{r}__{k}.npy"), np.concatenate([np.array(x[k]) for x in one]))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return H.run_settings(tmp_path_factory, __file__, "plan", settings={k: v[1] for k, v in SETTINGS.items()})


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_library_plans_what_the_host_table_says(runs, setting):
    """dartmpc_plan_query in a process with the setting's environment, on this device (its CU count sets the
    two-waves-per-SIMD threshold): the row of tests/test_launch_plan.py for the same input."""
    rows = pmpc_rows()
    for N, B, red, r in SHAPES:
        got = fmt(PMPC, runs[setting][f"plan__{_name(N, B, red, r)}"].tolist())
        assert got == rows[(SETTINGS[setting][0], N, B, red, _resto_in(N, B, red, r))], (setting, N, B, red, r)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_batch_equals_its_instances_one_by_one(runs, setting):
    """Every status 0; u0, f and iters of the first B instances of pmpc_batch(2) in one launch, bit for bit those of the
    same instances solved with B = 1."""
    res = runs[setting]
    for N, B, red, r in SHAPES:
        name = _name(N, B, red, r)
        assert np.all(res[f"{name}__status"] == 0), (setting, name, res[f"{name}__status"])
        for k in ("u0", "f", "iters"):
            assert np.array_equal(res[f"{name}__{k}"], res[f"one__{N}_{red}_{r}__{k}"][:B]), (setting, name, k)


if __name__ == "__main__":
    _child(sys.argv[1])
