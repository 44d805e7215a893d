"""The RMPC closed loop through the dual-arm layer on the device (csrc/rmpc_stack_step.hip, dart_rmpc_stack_*), on the
fixtures of test_gpu_stack.py: the xArm7 pair at its grasp pose (n = 7) and one random chain with n = 2.

Bars.  One launch against numpy (tests/rmpc_stack_refs.py): 1e-13 absolute on every field.  Coupling, command and plant
fields by test_gpu_stack.py's header (quantities at most 1 in magnitude, a few dozen fp64 operations and two
transcendentals, libm against the device's math library).  The RMPC glue fields (Rref, phi, y, r_v) carry the bar that
test_gpu_rollout.py applies to them under rmpc_loop_kernel, on loop_harness._rmpc_case's inputs: prev lies within 1e-3 of
x, so y = (v - v_prev) / Ts is at most 0.5 in magnitude and 1e-13 is ~1e3 ulp of it.  Everything that compares the device
with itself is bit for bit.

Measured on an MI355X (printed by the tests): max |device - numpy| over all fields of one command + one couple launch,
E in {1, 5}, the three (post, pre) pairs, n = 7 and 2 alike: tray plant 1.11e-16 in ride mode and 4.44e-16 in achieved
mode, LMPC plant 1.11e-16 in both modes; at N = 63 (tray plant, achieved mode, E = 5) 1.67e-16.
"""
import functools

import numpy as np
import pytest

import rmpc_stack_refs as RS
import stack_refs as S
from loop_harness import (RMPC_PRM, L, torch, _bits, _close, _host, _metrics_midrun, _nan_io, _ptrs, _rmpc_case,  # noqa: F401
                          _to_dev)
from test_gpu_stack import E_LOOP, K_LOOP, TS, _arms, _poses, _pvec

pytestmark = pytest.mark.gpu

N_HORIZON = 20
R_DACTL_GRASP = RS.DACTL_GRASP


@functools.lru_cache(maxsize=None)
def _solver(N=N_HORIZON, B_max=E_LOOP):
    import dart_mpc
    return dart_mpc.RmpcSolver(N=N, Ts=TS, B_max=B_max, device=0)


# ---- 1. one launch against numpy ----------------------------------------------------------------------------------------
ROWS_STEP, K_STEP = 4, 2


def _step_case(L, lm, E, n, N, seed):
    """Inputs of one command + one couple launch: loop_harness._rmpc_case's RMPC state and solve I/O (prev near x, one
    experiment in four crossing pos_tol), metrics under way, test_gpu_stack._poses' EE poses in the snapshot rows.  E = 5
    holds a non-finite ee_quat row (2), an experiment already done (3), one that crosses pos_tol in this launch (1) and
    one with nlog == log_rows (4)."""
    rng = np.random.default_rng(seed)
    SL = L.lib().dart_arm_snapshot_len(n)
    state, target, prm, plant, io = _rmpc_case(L, rng, E, N, lm)
    state["metrics"] = _metrics_midrun(L, E)
    sm = np.zeros((E, 8)); sm[1::2] = [0.01, 0.02, 1e-4, 0.5, 1e-3, 0.7, 1.0, 7.0]
    state["stack_metrics"] = sm
    _, pos, ee_pos, ee_quat = _poses(E, seed + 1)
    if E > 2:
        ee_quat[2, 0, 1] = np.nan                   # a non-finite row: its tilt is held
    if E == 5:
        state["done"][:] = [0, 0, 0, 1, 0]
        state["nlog"][4] = ROWS_STEP
    else:
        state["done"][:] = 0
    snap = rng.uniform(-1, 1, (2 * E, SL))
    snap[:, 3 * n + 3:3 * n + 6] = ee_pos.reshape(2 * E, 3)
    fixed = dict(target=target, prm=prm, tray_pos=pos, grasp=R_DACTL_GRASP.copy(), snap=snap,
                 ee_quat=ee_quat.reshape(2 * E, 4), tray_cmd=np.full((E, 7), np.nan))
    fixed["plant_pvec" if lm else "mu"] = plant
    return state, io, fixed, plant, ee_pos, ee_quat


def _one_launch(L, torch, lm, couple, n, E, N, do_post, do_pre):
    solver = _solver(N, 8)
    scfg, cfg = L.stack_config(couple), L.rmpc_loop_config()
    spec = L.RMPC_LM_LOOP_LOGS if lm else L.RMPC_LOOP_LOGS
    state, io, fixed, plant, ee_pos, ee_quat = _step_case(L, lm, E, n, N, 40 + E + N)
    logs, slogs = L.loop_logs(spec, ROWS_STEP, E), L.loop_logs(L.RMPC_STACK_LOGS, ROWS_STEP, E)
    d = _to_dev(torch, {**fixed, **state, **io})
    lg, sl = _to_dev(torch, logs), _to_dev(torch, slogs)
    solver.rmpc_stack_loop_step(E, n, K_STEP, L.STACK_COMMAND, 0, 0, ROWS_STEP, _ptrs(d), scfg=scfg, lm=lm)
    solver.rmpc_stack_loop_step(E, n, K_STEP, L.STACK_COUPLE, do_post, do_pre, ROWS_STEP, _ptrs(d), _ptrs(lg), _ptrs(sl),
                                scfg=scfg, lm=lm)
    solver.sync()
    got, glg, gsl = _host(d), _host(lg), _host(sl)
    ws, wio, wl, wsl = RS.rmpc_stack_step(lm, couple, N, K_STEP, do_post, do_pre, TS, cfg, state, fixed["target"],
                                          fixed["prm"], plant, io, logs, slogs, fixed["tray_pos"], ee_pos, ee_quat)
    what = f"lm={lm} couple={couple} n={n} E={E} N={N} post={do_post} pre={do_pre}"
    worst = max(_close(got, ws, what + " state"), _close(got, wio, what + " solve I/O"), _close(glg, wl, what + " logs"),
                _close(gsl, wsl, what + " stack logs"),
                _close(got, {"tray_cmd": S.command_pose(io["u0"], fixed["tray_pos"])}, what + " command"))
    assert _bits(got["tray_cmd"][:, :3], fixed["tray_pos"]), what
    if do_post:
        # log_quat is the command launch's pose, bit for bit
        assert _bits(gsl["quat_tray"][K_STEP], got["tray_cmd"][:, 3:]), what
        assert _bits(gsl["U_cmd"][K_STEP], io["u0"]), what
        assert _bits(got["u_prev"], io["u0"]), what          # the command in both modes
        if E > 2:       # the non-finite row: tilt held (achieved mode), counted
            assert got["stack_metrics"][2, 6] == state["stack_metrics"][2, 6] + 1.0
            assert np.isnan(gsl["tilt"][K_STEP, 2]).all()
            if couple == S.ACHIEVED:
                assert _bits(got["tilt"][2], state["tilt"][2]), what
            assert np.array_equal(np.delete(got["stack_metrics"][:, 6], 2), np.delete(state["stack_metrics"][:, 6], 2))
        if E == 5:
            assert got["done"].tolist() == [0, 1, 0, 1, 0], what              # 1 crossed, 3 was closed
            assert np.isnan(glg["pos_err_norm"][:, 3]).all() and got["nlog"][3] == state["nlog"][3]
            assert np.isnan(glg["pos_err_norm"][:, 4]).all() and got["nlog"][4] == ROWS_STEP + 1
            assert np.isfinite(glg["pos_err_norm"][state["nlog"][1], 1])
    else:
        assert np.array_equal(got["done"], state["done"]) and np.array_equal(got["nlog"], state["nlog"])
    # what the launch does not write is untouched
    for name in ("target", "prm", "plant_pvec" if lm else "mu", "tray_pos", "grasp", "snap", "ee_quat", "u0", "f", "status",
                 "iters", "theta"):
        assert _bits(got[name], {**fixed, **state, **io}[name]), (what, name)
    return worst


@pytest.mark.parametrize("n", [7, 2])
@pytest.mark.parametrize("couple", [S.RIDE, S.ACHIEVED])
@pytest.mark.parametrize("lm", [False, True])
def test_loop_step_launch_against_numpy(L, torch, lm, couple, n):
    worst = 0.0
    for E in (1, 5):
        for do_post, do_pre in ((0, 1), (1, 1), (1, 0)):
            worst = max(worst, _one_launch(L, torch, lm, couple, n, E, N_HORIZON, do_post, do_pre))
    print(f"rmpc stack loop step lm={lm} couple={couple} n={n}: max |device - numpy| = {worst:.2e} (bar 1e-13)")


def test_loop_step_launch_at_the_last_lane(L, torch):
    """N = 63: lane 63 writes the last reference node."""
    worst = _one_launch(L, torch, False, S.ACHIEVED, 7, 5, 63, 1, 1)
    print(f"rmpc stack loop step N=63: max |device - numpy| = {worst:.2e} (bar 1e-13)")


# ---- 2 / 3. the rollout ---------------------------------------------------------------------------------------------------
def _objects(E=E_LOOP, seed=5):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((E, 4)); x0[:, [0, 2]] = rng.uniform(-0.05, 0.05, (E, 2)); x0[:, [1, 3]] = rng.uniform(-0.1, 0.1, (E, 2))
    tg = np.zeros((E, 4)); tg[:, [0, 2]] = rng.uniform(-0.08, 0.08, (E, 2))
    tg[0, [0, 2]] = x0[0, [0, 2]] + 2e-3        # one episode closes at its first step
    return x0, tg, np.tile(RMPC_PRM, (E, 1)), rng.uniform(0.05, 0.3, E)


def _fresh(lm, n):
    from dart_mpc.harness import rmpc_stack_arrays
    rows, q0, qd0, tray_pos, prm = _arms(n)
    x0, tg, rprm, mu = _objects()
    arrays, E, n_, lm_ = rmpc_stack_arrays(x0, tg, q0, qd0, rows, prm, tray_pos, mu=mu, prm=rprm,
                                           plant_pvec=_pvec() if lm else None, N=N_HORIZON, Ts=TS)
    assert (E, n_, lm_) == (E_LOOP, n, lm)
    return arrays


def _run_host(L, lm, n, couple, k0, steps, rows, arrays, logs=True):
    from dart_mpc.harness import rmpc_stack_logs
    lg, sl, al = rmpc_stack_logs(rows, E_LOOP, n, lm) if logs is True else (logs if logs else (None, None, None))
    _solver().rmpc_stack_rollout(E_LOOP, n, k0, steps, rows, arrays["arm_prm"].shape[1], arrays, lg, sl, al,
                                 scfg=L.stack_config(couple), lm=lm)
    return arrays, (lg, sl, al)


@functools.lru_cache(maxsize=None)
def _full_run(lm, n, couple):
    from dart_mpc import _lib
    return _run_host(_lib, lm, n, couple, 0, K_LOOP, K_LOOP, _fresh(lm, n))


LOOP_STATE = ("x", "tilt", "prev", "u_prev", "r_v", "theta", "P", "w", "done", "nlog")
STATE = LOOP_STATE + ("metrics", "q", "qd", "qdd_prev", "arm_metrics", "stack_metrics")


@pytest.mark.parametrize("n", [7, 2])
@pytest.mark.parametrize("lm", [False, True])
def test_ride_mode_is_the_two_existing_loops(L, lm, n):
    from dart_mpc.harness import rollout_dual_arm, rollout_rmpc
    arrays, (lg, sl, al) = _full_run(lm, n, S.RIDE)
    rows, q0, qd0, tray_pos, prm = _arms(n)
    x0, tg, rprm, mu = _objects()
    # the object side: dart_rmpc[_lm]_rollout
    eps, status, done, extra = rollout_rmpc(x0, tg, K_LOOP, N=N_HORIZON, Ts=TS, prm=rprm, mu=mu,
                                            plant_pvec=_pvec() if lm else None, return_logs=True)
    for name in ("x", "theta", "r_v", "f", "status", "iters"):
        assert _bits(lg[name], extra[name]), name
    for name, rows_ in extra["episode_rows"].items():
        assert _bits(lg[name], rows_), name
    assert np.array_equal(arrays["done"].astype(bool), done)
    for name in LOOP_STATE + (("metrics",) if lm else ()):
        assert _bits(arrays[name], extra["state"][name]), name
    if lm:
        for b in range(E_LOOP):
            assert _bits(lg["rot"][:, b], eps[b]["rot"]), b
    assert arrays["nlog"][0] == 1 and np.all(arrays["nlog"][1:] == K_LOOP)
    # the arm side: dart_dual_arm_rollout fed tray_pos and this run's log_quat
    tray = np.concatenate([np.broadcast_to(tray_pos, (K_LOOP, E_LOOP, 3)), sl["quat_tray"]], axis=2)
    ar = rollout_dual_arm(q0, qd0, tray, rows, prm, K_LOOP)
    for name, key in (("q", "q"), ("qd", "qd"), ("qdd_prev", "qdd_prev"), ("arm_metrics", "metrics")):
        assert _bits(arrays[name].reshape(ar[key].shape), ar[key]), name
    for name in L.ARM_LOOP_LOGS:
        assert _bits(al[name], ar["logs"][name]), name
    assert np.all(arrays["stack_metrics"][:, 7] == K_LOOP)


@pytest.mark.parametrize("n", [7, 2])
@pytest.mark.parametrize("lm", [False, True])
def test_rollout_is_its_launches(L, torch, lm, n):
    from dart_mpc.arm import ArmDynamics, arm_config, arm_dyn_config
    from dart_mpc.harness import rmpc_stack_logs
    full, (lg, sl, al) = _full_run(lm, n, S.ACHIEVED)
    E, B, K, N = E_LOOP, 2 * E_LOOP, K_LOOP, N_HORIZON
    scfg = L.stack_config(S.ACHIEVED)

    def same(got, want, host=False):
        arrays, logs = got
        for name in STATE:
            assert _bits(arrays[name] if host else arrays[name].cpu().numpy(), full[name]), name
        for g, w in zip(logs, want):
            for name in w:
                assert _bits(g[name] if host else g[name].cpu().numpy(), w[name]), name

    # (a) the device form equals the host form
    d = _to_dev(torch, _fresh(lm, n))
    d["work"] = torch.zeros(L.lib().dart_stack_work_len(E, n), dtype=torch.float64, device="cuda")
    dl, ds, da = (_to_dev(torch, g) for g in rmpc_stack_logs(K, E, n, lm))
    _solver().rmpc_stack_rollout_dev(E, n, 0, K, K, full["arm_prm"].shape[1], _ptrs(d), _ptrs(dl), _ptrs(ds), _ptrs(da),
                                     scfg=scfg, lm=lm)
    _solver().sync()
    same((d, (dl, ds, da)), (lg, sl, al))

    # (b) 4 + 2 steps continued through k0, the state and the in/out metrics
    part, pl = _run_host(L, lm, n, S.ACHIEVED, 0, 4, K, _fresh(lm, n))
    part, _ = _run_host(L, lm, n, S.ACHIEVED, 4, 2, K, part, logs=pl)
    same((part, pl), (lg, sl, al), host=True)

    # (c) metrics-only
    mo, _ = _run_host(L, lm, n, S.ACHIEVED, 0, K, 0, _fresh(lm, n), logs=None)
    same((mo, ()), (), host=True)

    # (d) the same entries issued one by one from the host
    h = _to_dev(torch, _fresh(lm, n))
    SL = L.lib().dart_arm_snapshot_len(n)
    h["work"] = torch.zeros(L.lib().dart_dual_arm_work_len(E, n), dtype=torch.float64, device="cuda")
    h["snap"] = h["work"]
    h["ee_quat"] = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
    h["tray_cmd"] = torch.zeros((E, 7), dtype=torch.float64, device="cuda")
    h.update(_to_dev(torch, _nan_io(L, L.RMPC_LOOP_IO, E, nref=4 * (N + 1))))
    hl, hs, ha = (_to_dev(torch, g) for g in rmpc_stack_logs(K, E, n, lm))
    models_b = h["models"].repeat(E, 1).contiguous()
    scratch_snap = torch.zeros((B, SL), dtype=torch.float64, device="cuda")
    ident = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda").repeat(B, 1)
    dyn = ArmDynamics(_arms(n)[0][0], n)
    dcfg, qcfg = arm_dyn_config(), arm_config()
    vp = L.ctypes.c_void_p
    sv = _solver()
    p = _ptrs(h)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()            # every launch of the sequence, torch's included, on this one stream
    st = stream.cuda_stream
    sv.rmpc_stack_loop_step(E, n, 0, L.STACK_COUPLE, 0, 1, K, p, _ptrs(hl), _ptrs(hs), scfg=scfg, lm=lm, stream=st)
    for k in range(K):
        sv.solve_batch_dev(E, p["x0"], p["u_prev"], p["theta"], p["Rref"], p["prm"], p["u0"], p["f"], p["status"], p["iters"],
                           w_warm=p["w"], w_out=p["w"], rls_P=p["P"], rls_phi=p["phi"], rls_y=p["y"],
                           rls_lambda=L.rmpc_loop_config().rls_lambda, stream=st)
        sv.rmpc_stack_loop_step(E, n, k, L.STACK_COMMAND, 0, 0, K, p, scfg=scfg, lm=lm, stream=st)
        # the EE orientations of q_k (the rollout keeps them from its own dynamics launch)
        with torch.cuda.stream(stream):
            state_rows = torch.cat([h["q"], h["qd"], h["qdd_prev"], ident], dim=1).contiguous()
        dyn.dynamics_batch_dev(B, models_b.data_ptr(), False, state_rows.data_ptr(), scratch_snap.data_ptr(),
                               h["ee_quat"].data_ptr(), stream=st)
        # dynamics + QP + plant of one arm step: the arm rollout's device entry, this step's log rows
        rows_k = [ha[a][k].data_ptr() for a in L.ARM_LOOP_LOGS]
        rc = L.lib().dart_dual_arm_rollout_dev(L.ctypes.byref(dcfg), L.ctypes.byref(qcfg), E, n, 1, 1,
                                               *(vp(p[a]) for a in ("tray_cmd", "grasp", "models", "plant_models", "arm_prm")),
                                               full["arm_prm"].shape[1],
                                               *(vp(p[a]) for a in ("q", "qd", "qdd_prev", "arm_metrics", "work")),
                                               *(vp(q) for q in rows_k), vp(st))
        assert rc == 0
        sv.rmpc_stack_loop_step(E, n, k, L.STACK_COUPLE, 1, int(k + 1 < K), K, p, _ptrs(hl), _ptrs(hs), scfg=scfg, lm=lm,
                                stream=st)
    stream.synchronize()
    same((h, (hl, hs, ha)), (lg, sl, al))


# ---- 4. the coupling acts -------------------------------------------------------------------------------------------------
def test_the_coupling_acts():
    from dart_mpc._lib import LOG_INT_FILL
    from dart_mpc.harness import rollout_stack_rmpc
    rows, q0, qd0, tray_pos, prm = _arms(7)
    x0, tg, rprm, mu = _objects()
    K = K_LOOP
    kw = dict(mu=mu, prm=rprm, N=N_HORIZON, Ts=TS)
    a = rollout_stack_rmpc(x0, tg, q0, qd0, rows, prm, K, tray_pos, couple="achieved", **kw)
    r = rollout_stack_rmpc(x0, tg, q0, qd0, rows, prm, K, tray_pos, couple="ride", **kw)
    xa, xr = a["extra"]["state"]["x"], r["extra"]["state"]["x"]
    assert not np.array_equal(xa, xr)
    print("achieved vs ride after", K, "steps: max |x difference|", float(np.max(np.abs(xa - xr))),
          "stack metrics (achieved)", a["stack_metrics"].tolist())
    for res in (a, r):
        assert res["steps"] == K and np.all(res["stack_metrics"][:, 7] == K)
        assert np.isfinite(res["metrics"]).all() and np.isfinite(res["stack_metrics"]).all()
        assert np.all(res["status"] != LOG_INT_FILL) and res["U_log"].shape == (K, E_LOOP, 2)
        tau = res["arm"]["logs"]["tau"]
        for b, ep in enumerate(res["episodes"]):
            tq = np.asarray(ep["ep1"]["torque"])
            nl = len(ep["ep1"]["timestep"])
            assert nl == int(res["extra"]["state"]["nlog"][b]) >= 1 and tq.shape == (nl, 14)
            assert np.isfinite(tq).all() and np.all(np.any(tq != 0.0, axis=1))
            for j in range(nl):         # [L | R] of that step from the arm log
                assert _bits(tq[j], np.concatenate([tau[j, 2 * b], tau[j, 2 * b + 1]]))
    # the chunked run (check_every) is the bits of one call, and stops once every episode has closed
    c = rollout_stack_rmpc(x0, tg, q0, qd0, rows, prm, K, tray_pos, couple="achieved", check_every=4, **kw)
    for name in ("x", "theta", "w", "nlog"):
        assert _bits(c["extra"]["state"][name], a["extra"]["state"][name]), name
    assert _bits(c["stack_metrics"], a["stack_metrics"]) and _bits(c["arm"]["logs"]["tau"], a["arm"]["logs"]["tau"])
