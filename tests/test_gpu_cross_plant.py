"""The PMPC and RMPC closed loops on the LMPC plant, with streaming metrics (csrc/loop_step.hip pmpc_loop_kernel<true> /
rmpc_loop_kernel<true>, dart_pmpc_lm_* / dart_rmpc_lm_*).

Bars:
  * one loop step against the numpy code it restates (harness.LmpcPlant.step with -u, rollout_metrics, the RMPC glue
    of test_gpu_rollout.py): absolute 1e-13, the bar of the existing loop-step tests with the same argument (values
    below 1 in magnitude, a few dozen fp64 operations and a few transcendentals from the inputs, numpy's operation
    order, no fma contraction);
  * the next x of the new posts against dart_lmpc_loop_step_dev's post on (x, -tilt, -u, pvec): bit for bit, tilt
    equal with the sign flipped;
  * rollout against the same launches issued by hand, K1 + K2 against one call, metrics-only against logging mode:
    bit for bit; the metrics against rollout_metrics of the logs: bit for bit for the slots that are sums, maxima or
    counts of logged values (1, 4, 5, 6, 7), relative 1e-12 for those that pass through a square root first (0, 2, 3),
    and relative 1e-12 against logger_metrics (numpy sums pairwise, the accumulator sequentially);
  * resident against host loop: equal statuses; |dU_cmd|, |dX| (PMPC) and |du_cmd|, |dpos_err| (RMPC) at most ten
    times the values measured on one MI355X (the constants below), which must themselves stay below 1e-6;
  * point-mass reduction end to end: equal statuses, |dU_cmd| at most ten times the measured value, itself <= 1e-4
    (the plants alone differ by 1.3e-7 over 200 steps; the closed loop's gain on that is not derived).
Inputs of the closed-loop tests: rows of workload.pmpc_batch(1), zero rotation and pz_vz, pvec =
default_rng(11).uniform(0.01, 1.9, (B, 34)), N = 10, 40 steps, tol 1e-8.  With the C oracle in these loops on the CPU
every PMPC solve (4 and 18 rows) ends at status 0 in at most 17 iterations with |x| < 0.28, and every RMPC solve of
the first 4 rows ends at status 0 (18 rows: 718 of 720; the velocity cap binds twice, status 2).
"""
import numpy as np
import pytest

from loop_harness import (RMPC_PRM, TS, X_LO, L, torch, _bits, _close, _host, _metrics_midrun, _nan_io, _ptrs,  # noqa: F401
                          _rmpc_case, _rmpc_expected, _same, _to_dev)
from loop_harness import _lm_step as _plant_step

pytestmark = pytest.mark.gpu

N = 10

# largest differences between the resident loops and the host loops (harness.run_pmpc / run_rmpc with plant_pvec) over
# 40 steps x 4 experiments, and between the point-mass LMPC plant and the tray plant in closed loop over 40 steps x 18
# experiments, measured on one MI355X; the tests assert ten times these
MEASURED_PMPC_DU_CMD = 0.0              # (the two PMPC loops agreed bit for bit: the test asserts equality)
MEASURED_PMPC_DX = 0.0
MEASURED_RMPC_DU_CMD = 6.120e-15
MEASURED_RMPC_DPOS_ERR = 2.776e-17
MEASURED_REDUCTION_DU_CMD = 4.721e-08


@pytest.fixture(scope="module")
def pmpc_solver(L):
    s = L.Solver(N=N, Ts=TS, B_max=70)
    yield s
    s.close()


@pytest.fixture(scope="module")
def rmpc_solver(L):
    s = L.RmpcSolver(N=N, Ts=TS, B_max=70)
    yield s
    s.close()


@pytest.fixture(scope="module")
def lmpc_solver(L):
    s = L.LmpcSolver(N=N, Ts=TS, B_max=70)
    yield s
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# Test 1: one loop-step launch of each kernel against numpy
def _pmpc_case(L, rng, B):
    x = rng.uniform(X_LO, -X_LO, (B, 8))
    state = dict(x=x, tilt=rng.uniform(-0.3, 0.3, (B, 2)), metrics=_metrics_midrun(L, B))
    target = np.zeros((B, 6)); target[:, [0, 2]] = rng.uniform(-0.15, 0.15, (B, 2)); target[:, 4] = 0.4
    near = np.arange(B) % 4 == 1            # within 1 cm: slot 1 becomes k where it was -1
    target[near, 0] = x[near, 0] + 1e-3; target[near, 2] = x[near, 2] - 2e-3
    pz_vz = np.stack([np.full(B, 0.43), rng.uniform(-0.01, 0.01, B)], axis=1)
    io = _nan_io(L, L.PMPC_LOOP_IO, B)
    io.update(u0=rng.uniform(-0.5, 0.5, (B, 2)), f=rng.uniform(0, 1, B), status=rng.integers(-2, 1, B).astype(np.int32),
              iters=rng.integers(1, 60, B).astype(np.int32))
    return state, target, rng.uniform(0.01, 1.9, (B, 34)), pz_vz, io


def _pmpc_expected(harness, state, target, pvec, pz_vz, io, logs, k, do_post, do_pre):
    from dart_mpc.pmpc import tilt_to_quat
    s = {n: v.copy() for n, v in state.items()}
    q = {n: v.copy() for n, v in io.items()}
    lg = None if logs is None else {n: v.copy() for n, v in logs.items()}
    if do_post:
        x, u = s["x"], io["u0"]
        X6 = np.concatenate([x[:, :4], pz_vz], axis=1)
        if lg is not None:
            lg["X"][k], lg["U_cmd"][k], lg["loss"][k], lg["rot"][k] = X6, u, io["f"], x[:, 4:]
            lg["quat_tray"][k] = np.stack([tilt_to_quat(v) for v in u])
            lg["status"][k], lg["iters"][k] = io["status"], io["iters"]
        s["metrics"] = harness.rollout_metrics(X6[None], target, u[None], io["status"][None], io["iters"][None],
                                               x[None, :, 4:], TS, metrics=s["metrics"], k0=k)
        s["x"], s["tilt"] = _plant_step(harness, x, s["tilt"], u, pvec)
    if do_pre:
        q["x0"] = np.concatenate([s["x"][:, :4], pz_vz], axis=1)
    return s, q, lg


@pytest.mark.parametrize("do_post,do_pre", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_pmpc_lm_loop_step_matches_numpy(L, torch, pmpc_solver, B, do_post, do_pre):
    from dart_mpc import harness
    rng = np.random.default_rng(4100 + 10 * B + 2 * do_post + do_pre)
    state, target, pvec, pz_vz, io = _pmpc_case(L, rng, B)
    rows, k = 3, 1
    logs = L.loop_logs(L.PMPC_LM_LOOP_LOGS, rows, B)
    want = _pmpc_expected(harness, state, target, pvec, pz_vz, io, logs, k, do_post, do_pre)
    ds, dio, dl = _to_dev(torch, state), _to_dev(torch, io), _to_dev(torch, logs)
    c = _to_dev(torch, dict(target=target, pvec=pvec, pz_vz=pz_vz))
    pmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, rows, c["target"].data_ptr(), c["pvec"].data_ptr(),
                                 c["pz_vz"].data_ptr(), _ptrs(ds), _ptrs(dio), _ptrs(dl))
    pmpc_solver.sync()
    worst = max(_close(_host(g), w, what) for g, w, what in zip((ds, dio, dl), want, ("state", "solve I/O", "logs")))
    print(f"pmpc_lm loop step B={B} post={do_post} pre={do_pre}: max |difference| = {worst:.3e}")
    m = _host(ds)["metrics"]
    if do_post:
        fresh_near = (np.arange(B) % 4 == 1) & (state["metrics"][:, 1] < 0)
        assert np.all(m[fresh_near, 1] == k) and np.all(m[:, 7] == state["metrics"][:, 7] + 1)
    else:
        assert _bits(m, state["metrics"])
    g = _host(dl)
    untouched = [r for r in range(rows) if not (do_post and r == k)]
    assert np.isnan(g["X"][untouched]).all() and np.isnan(g["rot"][untouched]).all()
    assert np.all(g["status"][untouched] == L.LOG_INT_FILL)


@pytest.mark.parametrize("do_post,do_pre", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_rmpc_lm_loop_step_matches_numpy(L, torch, rmpc_solver, B, do_post, do_pre):
    from dart_mpc import harness
    rng = np.random.default_rng(5200 + 10 * B + 2 * do_post + do_pre)
    state, target, prm, pvec, io = _rmpc_case(L, rng, B, N, lm=True)
    rows, k = 4, 3
    logs = L.loop_logs(L.RMPC_LM_LOOP_LOGS, rows, B)
    want = _rmpc_expected(L, harness, state, target, prm, lambda x, tilt, u: _plant_step(harness, x, tilt, u, pvec),
                          io, logs, N, k, do_post, do_pre)
    ds, dio, dl = _to_dev(torch, state), _to_dev(torch, io), _to_dev(torch, logs)
    c = _to_dev(torch, dict(target=target, prm=prm, pvec=pvec))
    rmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, rows, c["target"].data_ptr(), c["prm"].data_ptr(),
                                 c["pvec"].data_ptr(), _ptrs(ds), _ptrs(dio), _ptrs(dl))
    rmpc_solver.sync()
    worst = max(_close(_host(g), w, what) for g, w, what in zip((ds, dio, dl), want, ("state", "solve I/O", "logs")))
    print(f"rmpc_lm loop step B={B} post={do_post} pre={do_pre}: max |difference| = {worst:.3e}")
    if do_post:        # closed episodes and rows past nlog keep the prefill
        g = _host(dl)
        closed = state["done"] == 1
        assert np.isnan(g["pos_err_norm"][:, closed]).all()
        for b in np.where(~closed)[0]:
            assert np.isnan(np.delete(g["pos_err_norm"][:, b], state["nlog"][b])).all()
        near = (np.arange(B) % 4 == 1) & ~closed
        assert np.all(_host(ds)["done"][near] == 1)


@pytest.mark.parametrize("do_post,do_pre", [(1, 0), (1, 1)])
def test_loop_steps_in_metrics_only_mode(L, torch, pmpc_solver, rmpc_solver, do_post, do_pre):
    """Every log pointer null: state, metrics and the solve's inputs as in logging mode (1e-13 against numpy, bit for bit
    against the logging launch), log_rows = 0 not consulted, RMPC's done / nlog advance."""
    from dart_mpc import harness
    B, k = 5, 9
    rng = np.random.default_rng(61 + do_pre)
    state, target, pvec, pz_vz, io = _pmpc_case(L, rng, B)
    want = _pmpc_expected(harness, state, target, pvec, pz_vz, io, None, k, do_post, do_pre)
    c = _to_dev(torch, dict(target=target, pvec=pvec, pz_vz=pz_vz))
    cp = (c["target"].data_ptr(), c["pvec"].data_ptr(), c["pz_vz"].data_ptr())
    ds, dio = _to_dev(torch, state), _to_dev(torch, io)
    pmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, 0, *cp, _ptrs(ds), _ptrs(dio), None)
    ds2, dio2 = _to_dev(torch, state), _to_dev(torch, io)
    dl2 = _to_dev(torch, L.loop_logs(L.PMPC_LM_LOOP_LOGS, k + 1, B))
    pmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, k + 1, *cp, _ptrs(ds2), _ptrs(dio2), _ptrs(dl2))
    pmpc_solver.sync()
    for g, w, what in zip((ds, dio), want, ("state", "solve I/O")):
        _close(_host(g), w, what)
    for a, b in ((ds, ds2), (dio, dio2)):
        for n in a:
            assert _same(torch, a[n], b[n]), n

    state, target, prm, pvec, io = _rmpc_case(L, rng, B, N, lm=True)
    want = _rmpc_expected(L, harness, state, target, prm, lambda x, tilt, u: _plant_step(harness, x, tilt, u, pvec),
                          io, None, N, k, do_post, do_pre)
    c = _to_dev(torch, dict(target=target, prm=prm, pvec=pvec))
    cp = (c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr())
    ds, dio = _to_dev(torch, state), _to_dev(torch, io)
    rmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, 0, *cp, _ptrs(ds), _ptrs(dio), None)
    ds2, dio2 = _to_dev(torch, state), _to_dev(torch, io)
    dl2 = _to_dev(torch, L.loop_logs(L.RMPC_LM_LOOP_LOGS, k + 1, B))
    rmpc_solver.loop_step_lm_dev(B, k, do_post, do_pre, k + 1, *cp, _ptrs(ds2), _ptrs(dio2), _ptrs(dl2))
    rmpc_solver.sync()
    for g, w, what in zip((ds, dio), want, ("state", "solve I/O")):
        _close(_host(g), w, what)
    for a, b in ((ds, ds2), (dio, dio2)):
        for n in a:
            assert _same(torch, a[n], b[n]), n
    open_ = state["done"] == 0
    assert open_.any() and np.all(_host(ds)["nlog"][open_] == state["nlog"][open_] + 1)


# ------------------------------------------------------------------------------------------------------------------
# Test 2: the plant step is lmpc_loop_kernel's, bit for bit, on (x, -tilt, -u, pvec)
@pytest.mark.parametrize("B", [1, 5, 70])
def test_plant_step_is_bitwise_the_lmpc_loop_steps(L, torch, pmpc_solver, rmpc_solver, lmpc_solver, B):
    rng = np.random.default_rng(700 + B)
    ps, ptg, pvec, pz_vz, pio = _pmpc_case(L, rng, B)
    x, tilt, u = ps["x"], ps["tilt"], pio["u0"]
    c = _to_dev(torch, dict(ptg=ptg, pvec=pvec, pz_vz=pz_vz, rtg=ptg[:, :4], rprm=np.tile(RMPC_PRM, (B, 1)),
                            ltg=np.zeros((B, 8))))
    # the LMPC loop's post on the flipped tilt and command
    ls = _to_dev(torch, dict(x=x, tilt=-tilt, u_prev=np.zeros((B, 2)), model_params=pvec))
    lio = _nan_io(L, L.LMPC_LOOP_IO, B)
    lio.update(u0=-u, f=pio["f"], status=pio["status"], iters=pio["iters"])
    lio = _to_dev(torch, lio)
    ll = _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, 1, B))
    lmpc_solver.loop_step_dev(B, 0, 1, 0, 1, c["ltg"].data_ptr(), c["pvec"].data_ptr(), _ptrs(ls), _ptrs(lio), _ptrs(ll))
    lmpc_solver.sync()
    # PMPC's post
    dps, dpio = _to_dev(torch, ps), _to_dev(torch, pio)
    pmpc_solver.loop_step_lm_dev(B, 0, 1, 0, 0, c["ptg"].data_ptr(), c["pvec"].data_ptr(), c["pz_vz"].data_ptr(),
                                 _ptrs(dps), _ptrs(dpio), None)
    pmpc_solver.sync()
    # RMPC's post, same x, tilt and command
    rs, _, _, _, rio = _rmpc_case(L, rng, B, N, lm=True)
    rs.update(x=x, tilt=tilt)
    rio.update(u0=u)
    drs, drio = _to_dev(torch, rs), _to_dev(torch, rio)
    rmpc_solver.loop_step_lm_dev(B, 0, 1, 0, 0, c["rtg"].data_ptr(), c["rprm"].data_ptr(), c["pvec"].data_ptr(),
                                 _ptrs(drs), _ptrs(drio), None)
    rmpc_solver.sync()
    assert not torch.equal(ls["x"], torch.from_numpy(x).cuda())          # the plant moved
    for what, d in (("PMPC", dps), ("RMPC", drs)):
        assert _same(torch, d["x"], ls["x"]), what
        assert _same(torch, d["tilt"], -ls["tilt"]), what


def test_glue_is_the_same_on_both_plants(L, torch, pmpc_solver):
    """The two instantiations of each glue kernel, given the same x[:, :4], prev, r_v, theta, done, nlog, target, prm
    and solve outputs, write the same bits to everything that does not pass through the plant step: from a pre-only
    launch the next solve's inputs and r_v, from a post + pre launch the episode and step rows and what the post
    hands to the next step.  RMPC at B = 5 (two blocks) with N = 1 and N = 63 (the ends of the staged reference's
    lanes), PMPC at B = 5; no solve runs."""
    B, rows, k = 5, 4, 3
    for N in (1, 63):
        with L.RmpcSolver(N=N, Ts=TS, B_max=B) as s:
            for do_post, do_pre in ((0, 1), (1, 1)):
                rng = np.random.default_rng(8800 + 10 * N + do_post)
                lm_state, target, prm, pvec, io = _rmpc_case(L, rng, B, N, lm=True)
                tray_state = {n: v for n, v in lm_state.items() if n != "metrics"}
                tray_state["x"] = np.concatenate([lm_state["x"][:, :4], np.full((B, 1), 0.43), np.zeros((B, 1))], axis=1)
                c = _to_dev(torch, dict(target=target, prm=prm, pvec=pvec, mu=rng.uniform(0.05, 0.3, B)))
                ts, tio, tl = (_to_dev(torch, d) for d in (tray_state, io, L.loop_logs(L.RMPC_LOOP_LOGS, rows, B)))
                ls, lio, ll = (_to_dev(torch, d) for d in (lm_state, io, L.loop_logs(L.RMPC_LM_LOOP_LOGS, rows, B)))
                s.loop_step_dev(B, k, do_post, do_pre, rows, c["target"].data_ptr(), c["prm"].data_ptr(), c["mu"].data_ptr(),
                                _ptrs(ts), _ptrs(tio), _ptrs(tl))
                s.loop_step_lm_dev(B, k, do_post, do_pre, rows, c["target"].data_ptr(), c["prm"].data_ptr(),
                                   c["pvec"].data_ptr(), _ptrs(ls), _ptrs(lio), _ptrs(ll))
                s.sync()
                if do_post:
                    pairs = [(tl[n], ll[n], "log " + n) for n, _, _ in L.RMPC_LOOP_LOGS]
                    pairs += [(ts[n], ls[n], n) for n in ("prev", "u_prev", "done", "nlog")]
                    assert not torch.isnan(tl["x"][k]).any() and not torch.isnan(tl["u_cmd"]).all()
                    assert not torch.equal(ts["nlog"], torch.from_numpy(tray_state["nlog"]).cuda())
                else:
                    pairs = [(tio[n], lio[n], n) for n in ("x0", "Rref", "phi", "y")] + [(ts["r_v"], ls["r_v"], "r_v")]
                    assert not torch.isnan(tio["Rref"]).any() and not torch.isnan(tio["phi"]).any()
                for a, b, what in pairs:
                    assert _same(torch, a, b), (N, do_post, do_pre, what)

    rng = np.random.default_rng(8900)
    lm_state, target, pvec, pz_vz, io = _pmpc_case(L, rng, B)
    tray_state = dict(x=np.concatenate([lm_state["x"][:, :4], pz_vz], axis=1), tilt=lm_state["tilt"])
    prm = np.tile([0.4, 100.0, 0.0, 0.1, -0.5, 0.5], (B, 1))
    c = _to_dev(torch, dict(target=target, prm=prm, pvec=pvec, pz_vz=pz_vz))
    ts, tio, tl = (_to_dev(torch, d) for d in (tray_state, io, L.loop_logs(L.PMPC_LOOP_LOGS, rows, B)))
    ls, lio, ll = (_to_dev(torch, d) for d in (lm_state, io, L.loop_logs(L.PMPC_LM_LOOP_LOGS, rows, B)))
    pmpc_solver.loop_step_dev(B, k, 1, 1, rows, c["prm"].data_ptr(), _ptrs(ts), _ptrs(tio), _ptrs(tl))
    pmpc_solver.loop_step_lm_dev(B, k, 1, 1, rows, c["target"].data_ptr(), c["pvec"].data_ptr(), c["pz_vz"].data_ptr(),
                                 _ptrs(ls), _ptrs(lio), _ptrs(ll))
    pmpc_solver.sync()
    for n in ("U_cmd", "quat_tray", "loss", "status", "iters"):
        assert _same(torch, tl[n], ll[n]), n
    assert _same(torch, tl["X"][:, :, :4].contiguous(), ll["X"][:, :, :4].contiguous())
    assert not torch.isnan(tl["quat_tray"][k]).any() and not torch.isnan(tl["X"][k]).any()


# ------------------------------------------------------------------------------------------------------------------
# Test 3: the rollout is its launches; a second call continues it
def _closed_loop_inputs(B, seed0=0):
    from dart_mpc.workload import pmpc_batch
    S, T, P = (a[:B].copy() for a in pmpc_batch(1, seed0=seed0))
    S[:, 4:] = 0.0                            # pz_vz = 0
    pvec = np.random.default_rng(11).uniform(0.01, 1.9, (B, 34))
    return S, T, P, pvec


def _pmpc_fresh(L, torch, S, rows):
    B = S.shape[0]
    x8 = np.zeros((B, 8)); x8[:, :4] = S[:, :4]
    st = _to_dev(torch, dict(x=x8, tilt=np.zeros((B, 2)), metrics=L.loop_metrics(B)))
    return st, (None if rows is None else _to_dev(torch, L.loop_logs(L.PMPC_LM_LOOP_LOGS, rows, B)))


def _pmpc_rollout(L, torch, s, S, c, rows, chunks):
    B = S.shape[0]
    st, lg = _pmpc_fresh(L, torch, S, rows)
    k = 0
    for n in chunks:
        s.rollout_lm_dev(B, k, n, rows or 0, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(),
                         c["pz_vz"].data_ptr(), _ptrs(st), _ptrs(lg))
        k += n
    s.sync()
    return st, lg


def test_pmpc_lm_rollout_is_its_launches_and_continues(L, torch, pmpc_solver):
    B, K = 5, 12
    S, T, P, pvec = _closed_loop_inputs(B, seed0=2)
    s = pmpc_solver
    c = _to_dev(torch, dict(target=T, prm=P, pvec=pvec, pz_vz=S[:, 4:6]))
    st, lg = _pmpc_rollout(L, torch, s, S, c, K, [K])
    st2, lg2 = _pmpc_fresh(L, torch, S, K)
    io = _to_dev(torch, _nan_io(L, L.PMPC_LOOP_IO, B))
    p, q = _ptrs(st2), _ptrs(io)
    cp = (c["target"].data_ptr(), c["pvec"].data_ptr(), c["pz_vz"].data_ptr())
    s.loop_step_lm_dev(B, 0, 0, 1, K, *cp, p, q, _ptrs(lg2))
    for k in range(K):
        s.solve_batch_dev(B, q["x0"], c["target"].data_ptr(), c["prm"].data_ptr(), q["u0"], q["f"], q["status"], q["iters"])
        s.loop_step_lm_dev(B, k, 1, int(k + 1 < K), K, *cp, p, q, _ptrs(lg2))
    s.sync()
    st3, lg3 = _pmpc_rollout(L, torch, s, S, c, K, [7, 5])
    for other_st, other_lg in ((st2, lg2), (st3, lg3)):
        for k in st:
            assert _same(torch, st[k], other_st[k]), k
        for k in lg:
            assert _same(torch, lg[k], other_lg[k]), k
    h = _host(lg)
    assert not np.isnan(h["U_cmd"]).any() and not np.isnan(h["rot"]).any() and np.all(h["status"] != L.LOG_INT_FILL)
    m = _host(st)["metrics"]
    assert np.all(m[:, 7] == K) and np.all(m[:, 5] == h["iters"].sum(axis=0))
    assert np.all(m[:, 4] == (h["status"] != 0).sum(axis=0))


def _rmpc_fresh(L, torch, s, S, rows):
    st = _to_dev(torch, s.loop_state_lm(S[:, :4]))
    return st, (None if rows is None else _to_dev(torch, L.loop_logs(L.RMPC_LM_LOOP_LOGS, rows, S.shape[0])))


def _rmpc_rollout(L, torch, s, S, c, rows, chunks, loop=None):
    B = S.shape[0]
    st, lg = _rmpc_fresh(L, torch, s, S, rows)
    k = 0
    for n in chunks:
        s.rollout_lm_dev(B, k, n, rows or 0, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(), _ptrs(st),
                         _ptrs(lg), loop=loop)
        k += n
    s.sync()
    return st, lg


def test_rmpc_lm_rollout_is_its_launches_and_continues(L, torch, rmpc_solver):
    B, K = 5, 12
    S, T, P, pvec = _closed_loop_inputs(B, seed0=2)
    T[0, [0, 2]] = S[0, [0, 2]] + 2e-3         # one episode closes at its first step
    s = rmpc_solver
    c = _to_dev(torch, dict(target=T[:, :4], prm=np.tile(RMPC_PRM, (B, 1)), pvec=pvec))
    st, lg = _rmpc_rollout(L, torch, s, S, c, K, [K])
    st2, lg2 = _rmpc_fresh(L, torch, s, S, K)
    io = _to_dev(torch, _nan_io(L, L.RMPC_LOOP_IO, B, nref=4 * (N + 1)))
    cp = (c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr())
    p, q = _ptrs(st2), _ptrs(io)
    s.loop_step_lm_dev(B, 0, 0, 1, K, *cp, p, q, _ptrs(lg2))
    for k in range(K):
        s.solve_batch_dev(B, q["x0"], p["u_prev"], p["theta"], q["Rref"], cp[1], q["u0"], q["f"], q["status"], q["iters"],
                          w_warm=p["w"], w_out=p["w"], rls_P=p["P"], rls_phi=q["phi"], rls_y=q["y"], rls_lambda=0.995)
        s.loop_step_lm_dev(B, k, 1, int(k + 1 < K), K, *cp, p, q, _ptrs(lg2))
    s.sync()
    st3, lg3 = _rmpc_rollout(L, torch, s, S, c, K, [7, 5])
    for other_st, other_lg in ((st2, lg2), (st3, lg3)):
        for k in st:
            assert _same(torch, st[k], other_st[k]), k
        for k in lg:
            assert _same(torch, lg[k], other_lg[k]), k
    h = _host(lg)
    assert not np.isnan(h["x"]).any() and not np.isnan(h["rot"]).any() and np.all(h["status"] != L.LOG_INT_FILL)
    n = _host(st)["nlog"]
    # an episode logs one row per step up to and including the first step below the tolerance (pmpc_batch starts a
    # quarter of its experiments within 5 mm of their targets)
    e = np.linalg.norm(h["x"][:, :, [0, 2]] - T[None, :, [0, 2]], axis=2)
    below = e < 0.01
    want_n = np.where(below.any(axis=0), below.argmax(axis=0) + 1, K)
    np.testing.assert_array_equal(n, want_n)
    assert n[0] == 1 and (n == K).any()
    assert np.isnan(h["u_cmd"][1:, 0]).all() and not np.isnan(h["u_cmd"][:, n == K]).any()
    m = _host(st)["metrics"]
    assert np.all(m[:, 7] == K) and np.all(m[:, 5] == h["iters"].sum(axis=0)) and m[0, 1] == 0.0


# ------------------------------------------------------------------------------------------------------------------
# Test 4: metrics-only against logging mode; the metrics against the logs
def _check_metrics_against_logs(harness, M, X, target, U, status, iters, rot, what):
    want = harness.rollout_metrics(X, target, U, status, iters, rot, TS)
    K, B = status.shape
    exact = [1, 4, 5, 6, 7]
    assert _bits(M[:, exact], want[:, exact]), (what, M[:, exact], want[:, exact])
    rel = np.abs(M[:, [0, 2, 3]] - want[:, [0, 2, 3]]) / np.abs(want[:, [0, 2, 3]])
    worst = float(rel.max())
    t = np.arange(K) * TS
    for b in range(B):
        ref = harness.logger_metrics({"X": X[:, b], "X_target": np.tile(target[b], (K, 1)), "t": t, "U_cmd": U[:, b]}, TS)
        conv = TS * M[b, 1] if M[b, 1] >= 0 else t[-1]
        for got, key in ((M[b, 0], "steady_state_error"), (M[b, 2], "control_effort"), (conv, "convergence_time")):
            d = abs(got - ref[key]) / abs(ref[key]) if ref[key] != 0 else abs(got)
            worst = max(worst, d)
    print(f"{what}: metrics against rollout_metrics / logger_metrics of the logs, max relative difference = {worst:.3e}")
    assert worst <= 1e-12


def test_metrics_only_mode_equals_logging_mode_and_the_logs(L, torch, pmpc_solver, rmpc_solver):
    from dart_mpc import harness
    B, K = 6, 40
    S, T, P, pvec = _closed_loop_inputs(B)
    T[1, [0, 2]] = S[1, [0, 2]] + 3e-3           # below 1 cm at step 0
    c = _to_dev(torch, dict(target=T, prm=P, pvec=pvec, pz_vz=S[:, 4:6]))
    st, lg = _pmpc_rollout(L, torch, pmpc_solver, S, c, K, [K])
    st0, _ = _pmpc_rollout(L, torch, pmpc_solver, S, c, None, [25, 15])
    for k in st:
        assert _same(torch, st[k], st0[k]), k
    h, M = _host(lg), _host(st)["metrics"]
    assert M[1, 1] == 0.0
    _check_metrics_against_logs(harness, M, h["X"], T, h["U_cmd"], h["status"], h["iters"], h["rot"], "PMPC")

    c = _to_dev(torch, dict(target=T[:, :4], prm=np.tile(RMPC_PRM, (B, 1)), pvec=pvec))
    loop = L.rmpc_loop_config(pos_tol=0.0)       # no episode closes: u_cmd row k is step k's command
    st, lg = _rmpc_rollout(L, torch, rmpc_solver, S, c, K, [K], loop=loop)
    st0, _ = _rmpc_rollout(L, torch, rmpc_solver, S, c, None, [25, 15], loop=loop)
    for k in st:
        assert _same(torch, st[k], st0[k]), k
    h, hs = _host(lg), _host(st)
    assert np.all(hs["nlog"] == K) and not hs["done"].any()
    _check_metrics_against_logs(harness, hs["metrics"], h["x"], T[:, :4], h["u_cmd"], h["status"], h["iters"], h["rot"],
                                "RMPC")


def test_host_entries_in_metrics_only_mode():
    """harness.rollout_pmpc / rollout_rmpc through dart_*_lm_rollout: metrics_only returns bit for bit the metrics of
    the logging call; the chunked RMPC run continues its metrics."""
    from dart_mpc import harness
    B, K = 4, 20
    S, T, P, pvec = _closed_loop_inputs(B)
    logs, st = harness.rollout_pmpc(S, T, P, K, N=N, plant_pvec=pvec)
    M = harness.rollout_pmpc(S, T, P, K, N=N, plant_pvec=pvec, metrics_only=True)
    assert M.shape == (B, 8) and _bits(M, np.stack([lg["metrics"] for lg in logs]))
    assert st.shape == (K, B) and logs[0]["rot"].shape == (K, 4) and np.all(M[:, 7] == K)
    eps, st, done = harness.rollout_rmpc(S[:, :4], T[:, :4], K, N=N, pos_tol=0.0, plant_pvec=pvec)
    M = harness.rollout_rmpc(S[:, :4], T[:, :4], K, N=N, pos_tol=0.0, plant_pvec=pvec, metrics_only=True, check_every=7)
    assert M.shape == (B, 8) and _bits(M, np.stack([e["metrics"] for e in eps]))
    assert st.shape == (K, B) and eps[0]["rot"].shape == (K, 4) and np.all(M[:, 7] == K)


# ------------------------------------------------------------------------------------------------------------------
# Tests 5, 6: resident against host loop
def test_pmpc_resident_against_host_loop():
    """B = 4, N = 10, 40 steps.  Measured on one MI355X over the 40 x 4 steps: max |dU_cmd| = 0, max |dX| = 0 (the
    logged states and commands of the two loops are bit for bit equal; the rotation states differ by 4.3e-19 and the
    metrics by 4.2e-22, numpy against device transcendentals).  The test asserts ten times the measured values, which
    here is equality, far below the 1e-6 closed-loop bar."""
    from dart_mpc import harness
    B, K = 4, 40
    S, T, P, pvec = _closed_loop_inputs(B)
    host, st_h = harness.run_pmpc(S, T, P, K, N=N, plant_pvec=pvec)
    dev, st_d = harness.rollout_pmpc(S, T, P, K, N=N, plant_pvec=pvec)
    du = max(float(np.max(np.abs(h["U_cmd"] - d["U_cmd"]))) for h, d in zip(host, dev))
    dx = max(float(np.max(np.abs(h["X"] - d["X"]))) for h, d in zip(host, dev))
    dr = max(float(np.max(np.abs(h["rot"] - d["rot"]))) for h, d in zip(host, dev))
    dm = float(np.max(np.abs(np.stack([h["metrics"] for h in host]) - np.stack([d["metrics"] for d in dev]))))
    print(f"rollout_pmpc vs run_pmpc on the LMPC plant: max|dU_cmd| = {du:.3e}, max|dX| = {dx:.3e}, max|drot| = {dr:.3e}, "
          f"max|dmetrics| = {dm:.3e}, statuses host {np.unique(st_h).tolist()} device {np.unique(st_d).tolist()}")
    np.testing.assert_array_equal(st_h, st_d)
    assert np.all(st_d == 0)
    assert 10 * MEASURED_PMPC_DU_CMD <= 1e-6 and 10 * MEASURED_PMPC_DX <= 1e-6
    assert du <= 10 * MEASURED_PMPC_DU_CMD and dx <= 10 * MEASURED_PMPC_DX


def test_rmpc_resident_against_host_loop():
    """The same shape for RMPC (pos_tol 0: every step is an episode row in both loops).  Which statuses RMPC reaches on
    this plant is not checked (the velocity cap can bind: status 2); the two loops must agree on them.  Measured on one
    MI355X over the 40 x 4 episode rows: max |du_cmd| = 6.120e-15, max |dpos_err| = 2.776e-17, every status 0 in both
    loops; the test asserts ten times these."""
    from dart_mpc import harness
    B, K = 4, 40
    S, T, P, pvec = _closed_loop_inputs(B)
    host = harness.run_rmpc(S[:, :4], T[:, :4], K, N=N, pos_tol=0.0, plant_pvec=pvec)
    dev = harness.rollout_rmpc(S[:, :4], T[:, :4], K, N=N, pos_tol=0.0, plant_pvec=pvec)
    du = dp = 0.0
    for b in range(B):
        h, g = host[0][b]["ep1"], dev[0][b]["ep1"]
        assert len(h["timestep"]) == len(g["timestep"]) == K, (b, len(h["timestep"]), len(g["timestep"]))
        du = max(du, float(np.max(np.abs(np.asarray(h["u_cmd"]) - np.asarray(g["u_cmd"])))))
        dp = max(dp, float(np.max(np.abs(np.asarray(h["pos_err"]) - np.asarray(g["pos_err"])))))
    print(f"rollout_rmpc vs run_rmpc on the LMPC plant: max|du_cmd| = {du:.3e}, max|dpos_err| = {dp:.3e}, statuses host "
          f"{np.unique(host[1], return_counts=True)} device {np.unique(dev[1], return_counts=True)}")
    np.testing.assert_array_equal(host[1], dev[1])
    assert 10 * MEASURED_RMPC_DU_CMD <= 1e-6 and 10 * MEASURED_RMPC_DPOS_ERR <= 1e-6
    assert du <= 10 * MEASURED_RMPC_DU_CMD and dp <= 10 * MEASURED_RMPC_DPOS_ERR


# ------------------------------------------------------------------------------------------------------------------
# Test 7: the point-mass reduction end to end
def test_point_mass_reduction_end_to_end():
    """rollout_pmpc on LmpcPlant(point_mass_pvec(mu)) against the tray-plant rollout without Coulomb friction, the 18
    experiments of pmpc_batch(1), 40 steps.  Measured on one MI355X: max |dU_cmd| = 4.721e-08 (max |dX| = 9.0e-09),
    equal statuses; the test asserts ten times the measured |dU_cmd|."""
    from dart_mpc import harness
    from dart_mpc.workload import pmpc_batch, point_mass_pvec
    S, T, P = pmpc_batch(1)
    K = 40
    lm, st_lm = harness.rollout_pmpc(S, T, P, K, N=N, plant_pvec=point_mass_pvec(P[:, 0]))
    tray, st_tr = harness.rollout_pmpc(S, T, P, K, N=N, plant_kw={"mu_c": 0})
    du = max(float(np.max(np.abs(a["U_cmd"] - b["U_cmd"]))) for a, b in zip(lm, tray))
    dx = max(float(np.max(np.abs(a["X"] - b["X"]))) for a, b in zip(lm, tray))
    print(f"point-mass LMPC plant vs tray plant (mu_c = 0) in closed loop: max|dU_cmd| = {du:.3e}, max|dX| = {dx:.3e}")
    np.testing.assert_array_equal(st_lm, st_tr)
    assert all(np.all(a["rot"] == 0.0) for a in lm)
    assert 10 * MEASURED_REDUCTION_DU_CMD <= 1e-4
    assert du <= 10 * MEASURED_REDUCTION_DU_CMD


# ------------------------------------------------------------------------------------------------------------------
# Test 8: errors
def test_cross_plant_errors_launch_nothing(L, torch, pmpc_solver, rmpc_solver):
    B, K = 3, 4
    S, T, P, pvec = _closed_loop_inputs(B)
    c = _to_dev(torch, dict(target=T, prm=P, pvec=pvec, pz_vz=S[:, 4:6], rtarget=T[:, :4], rprm=np.tile(RMPC_PRM, (B, 1))))
    pst, plg = _pmpc_fresh(L, torch, S, K)
    rst, rlg = _rmpc_fresh(L, torch, rmpc_solver, S, K)
    before = [{k: v.clone() for k, v in d.items()} for d in (pst, plg, rst, rlg)]
    pc = [c[n].data_ptr() for n in ("target", "prm", "pvec", "pz_vz")]
    rc = [c[n].data_ptr() for n in ("rtarget", "rprm", "pvec")]
    p, r = pmpc_solver, rmpc_solver
    E = L.DartMPCError
    for run, cc, st, lg in ((p.rollout_lm_dev, pc, pst, plg), (r.rollout_lm_dev, rc, rst, rlg)):
        with pytest.raises(E, match="B_max"):
            run(71, 0, K, K, *cc, _ptrs(st), _ptrs(lg))
        with pytest.raises(E, match="log_rows"):
            run(B, 2, K - 1, K, *cc, _ptrs(st), _ptrs(lg))
        with pytest.raises(E, match="negative"):
            run(B, 0, -1, K, *cc, _ptrs(st), _ptrs(lg))
        with pytest.raises(E, match="null pointer"):               # a required input
            run(B, 0, K, K, cc[0], cc[1], 0, *cc[3:], _ptrs(st), _ptrs(lg))
        with pytest.raises(E, match="null pointer"):               # the metrics
            run(B, 0, K, K, *cc, {**_ptrs(st), "metrics": 0}, _ptrs(lg))
        with pytest.raises(E, match="null and non-null log"):      # some logs given, others not
            run(B, 0, K, K, *cc, _ptrs(st), {**_ptrs(lg), "rot": 0})
        with pytest.raises(E, match="null and non-null log"):
            run(B, 0, K, K, *cc, _ptrs(st), {**{n: 0 for n in lg}, "status": lg["status"].data_ptr()})
        run(B, 0, 0, K, *cc, _ptrs(st), _ptrs(lg))                 # steps = 0: OK, touches nothing
        run(B, 0, 0, 0, *cc, _ptrs(st), None)
    with pytest.raises(E, match="null and non-null log"):          # the loop-step entries check the same way
        p.loop_step_lm_dev(B, 0, 1, 1, K, pc[0], pc[2], pc[3], _ptrs(pst),
                           {n: plg["X"].data_ptr() for n, _, _ in L.PMPC_LOOP_IO}, {**_ptrs(plg), "loss": 0})
    with pytest.raises(E, match="log_rows"):
        r.loop_step_lm_dev(B, K, 1, 1, K, *rc, _ptrs(rst), {n: rlg["x"].data_ptr() for n, _, _ in L.RMPC_LOOP_IO},
                           _ptrs(rlg))
    with pytest.raises(E, match="not an RMPC handle"):             # a PMPC handle given to the RMPC entry
        L.RmpcSolver.rollout_lm_dev(p, B, 0, K, K, *rc, _ptrs(rst), _ptrs(rlg))
    with pytest.raises(E, match="not a PMPC handle"):
        L.Solver.rollout_lm_dev(r, B, 0, K, K, *pc, _ptrs(pst), _ptrs(plg))
    p.sync(); r.sync()
    torch.cuda.synchronize()
    for a, b in zip((pst, plg, rst, rlg), before):
        for k in a:
            assert _same(torch, a[k], b[k]), k
