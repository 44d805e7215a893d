"""Outputs of the twelve PMPC / RMPC closed-loop entries (dart_{pmpc,rmpc}[_lm]_{loop_step_dev,rollout_dev,rollout}) at
small shapes, for a bit-for-bit comparison of two builds of the library (DART_MPC_LIB + DART_MPC_AB=1 name the other):

    python tools/loop_cases.py dump OUT.npz           once per library
    python tools/loop_cases.py compare A.npz B.npz    one line per array; exit status 1 if any differs

dump runs the four loop-step entries at B in (1, 5, 67) with the three (post, pre) pairs (RMPC at N in (1, 31, 32,
63), PMPC at N = 10), and the eight rollout entries at B = 5, N = 10 (RMPC also N = 40) over 12 steps, once in one
call and once as 5 + 7 steps, the _lm_ ones in logging and in metrics-only mode.  It stores every state, solve I/O,
log and metrics array, NaN / LOG_INT_FILL prefill included.  Inputs: those of tests/loop_harness.py and
tests/test_gpu_cross_plant.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"), os.path.join(ROOT, "tests")]

TS = 0.002
PAIRS = ((0, 1), (1, 1), (1, 0))


def dump(path):
    import torch
    from dart_mpc import _lib as L
    from dart_mpc.workload import pmpc_batch
    from loop_harness import RMPC_PRM, X_LO, _metrics_midrun, _nan_io, _ptrs, _rmpc_case, _to_dev
    out = {}

    def keep(case, **groups):
        torch.cuda.synchronize()
        for g, d in groups.items():
            for n, v in (d or {}).items():
                out[f"{case}/{g}/{n}"] = v.cpu().numpy() if hasattr(v, "cpu") else np.array(v)

    def ptr(c, *names):
        return [c[n].data_ptr() for n in names]

    # ---- the loop-step entries
    rows, k = 4, 3
    rs = {N: L.RmpcSolver(N=N, Ts=TS, B_max=67) for N in (1, 31, 32, 63)}
    ps = L.Solver(N=10, Ts=TS, B_max=67)
    for lm in (False, True):
        for B in (1, 5, 67):
            for post, pre in PAIRS:
                for N in (1, 31, 32, 63):
                    rng = np.random.default_rng(100 * N + 10 * B + 2 * post + pre + 7000 * lm)
                    state, target, prm, plant, io = _rmpc_case(L, rng, B, N, lm=lm)
                    c = _to_dev(torch, dict(target=target, prm=prm, plant=plant))
                    ds, dio = _to_dev(torch, state), _to_dev(torch, io)
                    dl = _to_dev(torch, L.loop_logs(L.RMPC_LM_LOOP_LOGS if lm else L.RMPC_LOOP_LOGS, rows, B))
                    s = rs[N]
                    (s.loop_step_lm_dev if lm else s.loop_step_dev)(B, k, post, pre, rows, *ptr(c, "target", "prm", "plant"),
                                                                    _ptrs(ds), _ptrs(dio), _ptrs(dl))
                    s.sync()
                    keep(f"rmpc_step_lm{int(lm)}_B{B}_N{N}_{post}{pre}", state=ds, io=dio, logs=dl)
                rng = np.random.default_rng(10 * B + 2 * post + pre + 9000 * lm)
                x = rng.uniform(X_LO, -X_LO, (B, 8)) if lm else rng.uniform(-0.3, 0.3, (B, 6))
                state = dict(x=x, tilt=rng.uniform(-0.3, 0.3, (B, 2)))
                if lm:
                    state["metrics"] = _metrics_midrun(L, B)
                prm = np.tile([0.4, 100.0, 0.0, 0.1, -0.5, 0.5], (B, 1)); prm[:, 0] = rng.uniform(0.05, 0.6, B)
                target = np.zeros((B, 6)); target[:, [0, 2]] = rng.uniform(-0.15, 0.15, (B, 2)); target[:, 4] = 0.4
                io = _nan_io(L, L.PMPC_LOOP_IO, B)
                io.update(u0=rng.uniform(-0.5, 0.5, (B, 2)), f=rng.uniform(0, 1, B),
                          status=rng.integers(-2, 1, B).astype(np.int32), iters=rng.integers(1, 60, B).astype(np.int32))
                c = _to_dev(torch, dict(target=target, prm=prm, pvec=rng.uniform(0.01, 1.9, (B, 34)),
                                        pz_vz=np.stack([np.full(B, 0.43), rng.uniform(-0.01, 0.01, B)], axis=1)))
                ds, dio = _to_dev(torch, state), _to_dev(torch, io)
                dl = _to_dev(torch, L.loop_logs(L.PMPC_LM_LOOP_LOGS if lm else L.PMPC_LOOP_LOGS, rows, B))
                if lm:
                    ps.loop_step_lm_dev(B, k, post, pre, rows, *ptr(c, "target", "pvec", "pz_vz"), _ptrs(ds), _ptrs(dio),
                                        _ptrs(dl))
                else:
                    ps.loop_step_dev(B, k, post, pre, rows, c["prm"].data_ptr(), _ptrs(ds), _ptrs(dio), _ptrs(dl))
                ps.sync()
                keep(f"pmpc_step_lm{int(lm)}_B{B}_{post}{pre}", state=ds, io=dio, logs=dl)
    for s in list(rs.values()) + [ps]:
        s.close()

    # ---- the rollout entries: device and host forms, one call and 5 + 7, logging and metrics-only
    B, K = 5, 12
    S, T, P = (a[:B].copy() for a in pmpc_batch(1, seed0=2))
    pvec = np.random.default_rng(11).uniform(0.01, 1.9, (B, 34))
    mu = np.random.default_rng(12).uniform(0.05, 0.3, B)
    Tr = T[:, :4].copy(); Tr[0, [0, 2]] = S[0, [0, 2]] + 2e-3        # one RMPC episode closes at its first step
    rprm = np.tile(RMPC_PRM, (B, 1))
    x8 = np.zeros((B, 8)); x8[:, :4] = S[:, :4]
    c = _to_dev(torch, dict(T=T, P=P, Tr=Tr, rprm=rprm, mu=mu, pvec=pvec, pz_vz=S[:, 4:6]))
    for lm in (False, True):
        for logging in ((True, False) if lm else (True,)):
            for chunks in ((K,), (5, 7)):
                for host in (False, True):
                    tag = f"lm{int(lm)}_logs{int(logging)}_{'+'.join(map(str, chunks))}_{'host' if host else 'dev'}"
                    # PMPC
                    st = dict(x=x8.copy(), tilt=np.zeros((B, 2)), metrics=L.loop_metrics(B)) if lm else \
                        dict(x=S.copy(), tilt=np.zeros((B, 2)))
                    lg = L.loop_logs(L.PMPC_LM_LOOP_LOGS if lm else L.PMPC_LOOP_LOGS, K, B) if logging else None
                    if not host:
                        st, lg = _to_dev(torch, st), (None if lg is None else _to_dev(torch, lg))
                    with L.Solver(N=10, Ts=TS, B_max=B) as s:
                        k0 = 0
                        for n in chunks:
                            if host and lm:
                                s.rollout_lm(k0, n, T, P, pvec, S[:, 4:6], st, lg)
                            elif host:
                                s.rollout(k0, n, T, P, st, lg)
                            elif lm:
                                s.rollout_lm_dev(B, k0, n, K if logging else 0, *ptr(c, "T", "P", "pvec", "pz_vz"), _ptrs(st),
                                                 _ptrs(lg))
                            else:
                                s.rollout_dev(B, k0, n, K, *ptr(c, "T", "P"), _ptrs(st), _ptrs(lg))
                            k0 += n
                        s.sync()
                    keep("pmpc_rollout_" + tag, state=st, logs=lg)
                    # RMPC
                    for N in (10, 40):
                        with L.RmpcSolver(N=N, Ts=TS, B_max=B) as s:
                            st = s.loop_state_lm(S[:, :4]) if lm else s.loop_state(S[:, :4])
                            lg = L.loop_logs(L.RMPC_LM_LOOP_LOGS if lm else L.RMPC_LOOP_LOGS, K, B) if logging else None
                            if not host:
                                st, lg = _to_dev(torch, st), (None if lg is None else _to_dev(torch, lg))
                            k0 = 0
                            for n in chunks:
                                if host and lm:
                                    s.rollout_lm(k0, n, Tr, rprm, pvec, st, lg)
                                elif host:
                                    s.rollout(k0, n, Tr, rprm, mu, st, lg)
                                elif lm:
                                    s.rollout_lm_dev(B, k0, n, K if logging else 0, *ptr(c, "Tr", "rprm", "pvec"), _ptrs(st),
                                                     _ptrs(lg))
                                else:
                                    s.rollout_dev(B, k0, n, K, *ptr(c, "Tr", "rprm", "mu"), _ptrs(st), _ptrs(lg))
                                k0 += n
                            s.sync()
                        keep(f"rmpc_rollout_N{N}_" + tag, state=st, logs=lg)
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for n in bad:
        print(f"{n}: only in one file")
    for n in sorted(set(a.files) & set(b.files)):
        x, y = a[n], b[n]
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print(f"{n} {x.dtype}{list(x.shape)}: {'equal' if same else 'DIFFERENT'}")
        if not same:
            bad.append(n)
    print(f"{len(a.files)} arrays against {len(b.files)}: " + ("every array equal" if not bad else f"{len(bad)} DIFFER"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
