"""Outputs of every PMPC kernel of pmpc_ipm.hip for the library named by DART_MPC_LIB (+ DART_MPC_AB=1), for a
bit-for-bit comparison of two builds: python tools/pmpc_fold_cases.py <outdir>, once per library, then tools/ab_compare.py on each
pair of <outdir>/<case>.npz (u0, f, st, it, w).

The cases together launch every kernel of the three objects built from pmpc_ipm.hip at the smallest shape that selects
it.  The launcher reads its knobs once per process, so every knob setting (GROUPS) runs in a fresh child process: this
file again, with --group.  Inputs: the first 32 instances of pmpc_batch(2); the wide-box inputs of
tests/pmpc_overlap_harness.py with max_soc = 0, whose line searches fail (the restoration hand-over, the fused tail,
status -2); the 1152 instances of the bench's C4 line at N = 40 (the soft phase); a warm start; the least-square
multiplier estimate on (default) and off.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))

GROUPS = {"default": {}, "ovl0": {"DART_PMPC_OVERLAP": "0"}, "occ2": {"DART_PMPC_OCC2_MIN_B": "1"},
          "seq": {"DART_PMPC_QSCAN_MAX_B": "0"}, "seqlong": {"DART_PMPC_SEQ_LONG": "1"}}
KNOBS = sorted({k for env in GROUPS.values() for k in env})


def cases(group):
    """(name, inputs, B, Solver keywords, mode) of one group; mode: "" (one launch), "warm" or "serve"."""
    out = []

    def add(N, B, inp="pm", mode="", **kw):
        tag = "".join(f"_{k}{v}" for k, v in sorted(kw.items())).replace("restoration", "r").replace("False", "0") \
            .replace("True", "1").replace("max_soc", "soc").replace("path", "").replace("constr_mult_init_max", "lsm")
        out.append((f"{group}_{inp}{mode}_n{N}_b{B}{tag}", inp, B, dict(N=N, **kw), mode))

    def soft_phase():
        # N = 40 settles its failed line searches in the soft phase, which the small inputs do not reach: the 1152
        # instances of the bench's C4 line (41 of them at the default options), and with the correction off
        add(40, 1152, "c4")
        for r in (False, True):
            add(40, 1152, "c4", max_soc=0, restoration=r)

    if group == "default":
        for N in (15, 16, 23, 24, 31, 32, 40, 63):
            for B in (1, 32):                                   # the three-wave and fused kernels, the two-wave workgroups
                for r in (False, True):
                    add(N, B, restoration=r)
        for N in (15, 16, 23, 24, 31):                          # pack == 1: the one-wave kernels
            add(N, 33)
        for N in (15, 20, 31, 40):
            add(N, 32, path="reduced")
        for N in (15, 20, 31, 40):
            for r in (False, True):
                add(N, 18, "wide", max_soc=0, restoration=r)
        add(20, 18, mode="warm")
        add(20, 18, constr_mult_init_max=0.0)
        for N in (15, 20, 31):                                  # the resident server
            for r in (False, True):
                add(N, 18, mode="serve", restoration=r)
        add(20, 18, "wide", mode="serve", max_soc=0)
        soft_phase()
    elif group == "ovl0":                                       # the fused and plain one-wave kernels at B <= 32
        for N in (16, 23, 24, 31):
            for B in (1, 32):
                for r in (False, True):
                    add(N, B, restoration=r)
        for N in (20, 31):
            for r in (False, True):
                add(N, 18, "wide", max_soc=0, restoration=r)
    elif group == "occ2":                                       # two waves per SIMD
        for N in (15, 16, 23, 24, 31):
            add(N, 18)
        for r in (False, True):
            add(20, 18, "wide", max_soc=0, restoration=r)
    elif group == "seq":                                        # the sequential kernels
        for N in (15, 16, 23, 24, 31, 40):
            add(N, 18)
        add(20, 18, path="reduced")
        for r in (False, True):
            add(20, 18, "wide", max_soc=0, restoration=r)
    elif group == "seqlong":                                    # NAX == 2
        for N in (32, 40, 63):
            for r in (False, True):
                add(N, 18, restoration=r)
        for r in (False, True):
            add(40, 18, "wide", max_soc=0, restoration=r)
        soft_phase()
    return out


def child(group, outdir):
    import dart_mpc
    from dart_mpc.workload import pmpc_batch
    S, T, P = pmpc_batch(2)
    Sw, Tw, Pw = pmpc_batch(1)
    Pw = Pw.copy(); Pw[:, 4] = -1.2; Pw[:, 5] = 1.2
    Tw = Tw.copy(); Tw[:, 0] = np.where(Sw[:, 0] > 0, -0.6, 0.6); Tw[:, 2] = np.where(Sw[:, 2] > 0, -0.5, 0.5)
    data = {"pm": (S, T, P), "wide": (Sw, Tw, Pw), "c4": pmpc_batch(64, seed0=300000)}
    for name, inp, B, kw, mode in cases(group):
        x = [a[:B] for a in data[inp]]
        with dart_mpc.Solver(Ts=0.002, tol=1e-8, B_max=B, **kw) as s:
            if mode == "serve":
                s.serve_start(B_serve=B, idle_timeout=5.0)
            r = s.solve_batch(*x, want_w=True)
            if mode == "warm":
                r = s.solve_batch(*x, w_warm=r["w"], want_w=True)
            if mode == "serve":
                s.serve_stop()
        np.savez(os.path.join(outdir, name + ".npz"), u0=r["u0"], f=r["f"], st=r["status"], it=r["iters"], w=r["w"])
        print(name, "status", np.unique(r["status"]).tolist(), "iters_sum", int(r["iters"].sum()), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--group":
        child(sys.argv[2], sys.argv[3])
    else:
        os.makedirs(sys.argv[1], exist_ok=True)
        for group, knobs in GROUPS.items():
            env = {k: v for k, v in os.environ.items() if k not in KNOBS}
            env.update(knobs)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group, sys.argv[1]], env=env,
                           check=True, timeout=300)
