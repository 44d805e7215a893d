"""The PMPC closed loop through the dual-arm layer on the device (csrc/stack_step.hip, dart_pmpc_stack_*), on the xArm7
fixture (n = 7) and on one random model with n = 2, so that a stride in n cannot hide.

Bars.  Against numpy (tests/stack_refs.py): 1e-13 absolute, the argument of test_gpu_rollout.py's header -- the
quantities are at most 1 in magnitude, a coupling is a few dozen fp64 operations and two transcendentals (atan2, asin;
the command: sin, cos), libm against the device's math library, a few ulp of 1.1e-16 each.  Everything that compares the
device with itself is bit for bit.

Measured on an MI355X (printed by the tests): coupling against numpy, max |difference| 2.2e-16 at E = 5 and E = 67
(2.0e-19 at E = 1); one command + one couple + object launch against numpy 1.1e-16 on both plants, both modes, n = 7, 2.
"""
import functools
import os

import numpy as np
import pytest

import arm_dyn_refs as R
import arm_qp
import stack_refs as S
from loop_harness import L, torch, _bits, _close, _host, _ptrs, _to_dev  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BAR = 1e-13
TS, N_HORIZON = 0.002, 20
E_LOOP, K_LOOP = 3, 6


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def _params(n):
    if n == 7:
        return arm_qp.default_params()
    return {"Wimp": np.diag([10.0, 10.0, 10.0, 1.0, 1.0, 1.0]), "Wpos": np.eye(n) * 0.1, "Wsmooth": np.zeros((n, n)),
            "Qmin": -3.0 * np.ones(n), "Qmax": 3.0 * np.ones(n), "Qdotmin": -20.0 * np.ones(n), "Qdotmax": 20.0 * np.ones(n),
            "taumin": -50.0 * np.ones(n), "taumax": 50.0 * np.ones(n), "K": np.diag([500.0] * 3 + [5.0] * 3),
            "K_null": np.eye(n), "dt": TS}


@functools.lru_cache(maxsize=None)
def _arms(n):
    """(model rows [2, .], q0 [E, 2, n], qd0, tray_pos [E, 3], parameter dict): the xArm7 pair at the grasp pose of a level
    tray (tests/golden/xarm7_grasp_q.npz: inverse kinematics of arm_dyn_refs for the tray at (0, 0, 0.4)), slightly
    perturbed; or one random two-joint chain for both arms."""
    rng = np.random.default_rng(300 + n)
    if n == 7:
        rows = np.load(os.path.join(GOLD, "xarm7_arm_models.npz"))["rows"]
        g = np.load(os.path.join(GOLD, "xarm7_grasp_q.npz"))
        q0 = g["q"][None] + rng.uniform(-2e-3, 2e-3, (E_LOOP, 2, 7))
        tray_pos = np.tile(g["tray_pos"], (E_LOOP, 1))
    else:
        rows = np.stack([R.random_model(rng, n)] * 2)
        q0 = rng.uniform(-1.0, 1.0, (E_LOOP, 2, n))
        tray_pos = rng.uniform(-0.2, 0.2, (E_LOOP, 3))
    return rows, q0, rng.uniform(-1e-2, 1e-2, (E_LOOP, 2, n)), tray_pos, _params(n)


def _objects(E=E_LOOP):
    from dart_mpc.workload import pmpc_batch
    S0, T, P = pmpc_batch(1)
    return S0[:E].copy(), T[:E].copy(), P[:E].copy()


def _pvec(E=E_LOOP):
    from dart_mpc.workload import lmpc_batch
    return np.ascontiguousarray(lmpc_batch(1)["pvec"][:E])


def _poses(E, seed):
    """E experiments' EE poses: exact grasps of random tilted trays, every other one perturbed (position by up to a
    centimetre, orientation by up to 0.05 rad, independently per arm)."""
    from dart_mpc.pmpc import tilt_to_quat
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.5, 0.5, (E, 2))
    pos = rng.uniform(-0.5, 0.5, (E, 3))
    ee_pos, ee_quat = np.zeros((E, 2, 3)), np.zeros((E, 2, 4))
    for e in range(E):
        for a, (p, q) in enumerate(R.resolve_ee_targets(pos[e], tilt_to_quat(u[e]))):
            if e % 2:
                p = p + rng.uniform(-0.01, 0.01, 3)
                w = rng.uniform(-0.05, 0.05, 3)
                q = R.qmul(np.concatenate([[np.cos(np.linalg.norm(w) / 2)], np.sin(np.linalg.norm(w) / 2) * w / np.linalg.norm(w)]), q)
            ee_pos[e, a], ee_quat[e, a] = p, q * rng.choice([-1.0, 1.0])
    return u, pos, ee_pos, ee_quat


def _max_diff(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    return float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0


# ---- 1. the coupling alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 5, 67])
def test_tray_from_arms_against_numpy(E):
    from dart_mpc.arm import tray_from_arms
    _, _, ee_pos, ee_quat = _poses(E, 10 + E)
    cases = [(ee_pos, ee_quat)]
    bad = ee_quat.copy()
    bad[E // 2, 1, 2] = np.nan                      # one non-finite row
    cases.append((ee_pos, bad))
    worst = 0.0
    for p, q in cases:
        got, ref = tray_from_arms(p, q), S.tray_from_arms_batch(p, q)
        for k in ("tray", "tilt", "yaw", "gap", "angle"):
            worst = max(worst, _max_diff(got[k], ref[k]))
    assert not np.isfinite(got["tilt"][E // 2]).any()
    assert np.isfinite(np.delete(got["tilt"], E // 2, axis=0)).all()
    print(f"dart_tray_from_arms E = {E}: max |device - numpy| = {worst:.2e} (bar {BAR:.0e})")
    assert worst <= BAR
    if E == 1:      # the unbatched form
        one = tray_from_arms(ee_pos[0], ee_quat[0])
        assert one["tray"].shape == (7,) and np.array_equal(one["tilt"], tray_from_arms(ee_pos, ee_quat)["tilt"][0])


# ---- 2. one command launch, one couple + object launch ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solver(B_max=8):
    import dart_mpc
    return dart_mpc.Solver(N=N_HORIZON, Ts=TS, tol=1e-8, B_max=B_max, device=0)


def _step_case(L, lm, E, n, seed):
    rng = np.random.default_rng(seed)
    SL = L.lib().dart_arm_snapshot_len(n)
    u, pos, ee_pos, ee_quat = _poses(E, seed + 1)
    if E > 2:
        ee_quat[2, 0, 1] = np.nan                   # a non-finite row: its tilt is held
    snap = rng.uniform(-1, 1, (2 * E, SL))
    snap[:, 3 * n + 3:3 * n + 6] = ee_pos.reshape(2 * E, 3)
    x = np.zeros((E, 8 if lm else 6))
    x[:, :4] = rng.uniform(-0.15, 0.15, (E, 4))
    if lm:
        x[:, 4:] = rng.uniform(-0.05, 0.05, (E, 4))
    else:
        x[:, 4], x[:, 5] = 0.43, rng.uniform(-0.01, 0.01, E)
    target = np.zeros((E, 6)); target[:, [0, 2]] = rng.uniform(-0.1, 0.1, (E, 2)); target[:, 4] = 0.43
    target[0, 0], target[0, 2] = x[0, 0] + 1e-3, x[0, 2]          # within the metric's 1 cm: slot 1 is set
    m = L.loop_metrics(E); m[1::2] = [0.03, -1.0, 0.2, 0.09, 2.0, 55.0, 0.02, 7.0]
    sm = np.zeros((E, 8)); sm[1::2] = [0.01, 0.02, 1e-4, 0.5, 1e-3, 0.7, 1.0, 7.0]
    arrays = dict(target=target, prm=np.tile([0.1, 600.0, 5.0, 0.1, -0.6, 0.6], (E, 1)) * rng.uniform(0.9, 1.1, (E, 1)),
                  plant_pvec=rng.uniform(0.01, 1.9, (E, 34)), pz_vz=rng.uniform(-0.01, 0.01, (E, 2)), tray_pos=pos,
                  grasp=R.DACTL_GRASP.copy(), snap=snap, ee_quat=ee_quat.reshape(2 * E, 4), x=x,
                  tilt=rng.uniform(-0.3, 0.3, (E, 2)), metrics=m, stack_metrics=sm, x0=np.full((E, 6), np.nan),
                  tray_cmd=np.full((E, 7), np.nan), u0=rng.uniform(-0.5, 0.5, (E, 2)), f=rng.uniform(0, 1, E),
                  status=rng.integers(-2, 3, E).astype(np.int32), iters=rng.integers(1, 60, E).astype(np.int32))
    return arrays, ee_pos, ee_quat


@pytest.mark.parametrize("n", [7, 2])
@pytest.mark.parametrize("couple", [S.RIDE, S.ACHIEVED])
@pytest.mark.parametrize("lm", [False, True])
def test_loop_step_launches_against_numpy(L, torch, lm, couple, n):
    solver, rows, k = _solver(), 4, 2
    scfg = L.stack_config(couple)
    worst = 0.0
    for E in (1, 5):
        arrays, ee_pos, ee_quat = _step_case(L, lm, E, n, 40 + E)
        for do_post, do_pre in ((0, 1), (1, 1), (1, 0)):
            d = _to_dev(torch, arrays)
            lg = _to_dev(torch, L.loop_logs(L.PMPC_LM_LOOP_LOGS if lm else L.PMPC_LOOP_LOGS, rows, E))
            sl = _to_dev(torch, L.loop_logs(L.STACK_LOGS, rows, E))
            solver.stack_loop_step_dev(E, n, k, L.STACK_COMMAND, 0, 0, rows, _ptrs(d), scfg=scfg, lm=lm)
            solver.stack_loop_step_dev(E, n, k, L.STACK_COUPLE, do_post, do_pre, rows, _ptrs(d), _ptrs(lg), _ptrs(sl),
                                       scfg=scfg, lm=lm)
            solver.sync()
            got, glg, gsl = _host(d), _host(lg), _host(sl)
            ref = S.stack_step(lm, couple, k, do_post, do_pre, TS, arrays["target"], arrays["prm"], arrays["tray_pos"],
                               ee_pos, ee_quat, arrays["x"], arrays["tilt"], arrays["metrics"], arrays["stack_metrics"],
                               arrays["u0"], arrays["f"], arrays["status"], arrays["iters"],
                               plant_pvec=arrays["plant_pvec"], pz_vz=arrays["pz_vz"])
            what = f"lm={lm} couple={couple} n={n} E={E} post={do_post} pre={do_pre}"
            want = {k_: ref[k_] for k_ in ("x", "tilt", "metrics", "stack_metrics")}
            want["x0"] = ref["x0"] if do_pre else arrays["x0"]
            want["tray_cmd"] = S.command_pose(arrays["u0"], arrays["tray_pos"])
            worst = max(worst, _close(got, want, what))
            wl = L.loop_logs(L.PMPC_LM_LOOP_LOGS if lm else L.PMPC_LOOP_LOGS, rows, E)
            ws = L.loop_logs(L.STACK_LOGS, rows, E)
            if do_post:
                for name in wl:
                    wl[name][k] = ref[name]
                ws["tilt"][k], ws["tray"][k] = ref["tilt_log"], ref["tray_log"]
                # the command pose is log_quat's expressions, bit for bit
                assert _bits(got["tray_cmd"][:, 3:], glg["quat_tray"][k]), what
                assert _bits(got["tray_cmd"][:, :3], arrays["tray_pos"]), what
                if E > 2:       # the non-finite row: tilt held (achieved mode), counted
                    assert got["stack_metrics"][2, 6] == arrays["stack_metrics"][2, 6] + 1.0
                    assert np.isnan(gsl["tilt"][k, 2]).all()
                    if couple == S.ACHIEVED:
                        assert _bits(got["tilt"][2], arrays["tilt"][2]), what
                    assert np.array_equal(np.delete(got["stack_metrics"][:, 6], 2),
                                          np.delete(arrays["stack_metrics"][:, 6], 2))
            worst = max(worst, _close(glg, wl, what + " logs"), _close(gsl, ws, what + " stack logs"))
            # what the launch does not write is untouched
            for name in ("target", "prm", "plant_pvec", "pz_vz", "tray_pos", "grasp", "snap", "ee_quat", "u0", "f",
                         "status", "iters"):
                assert _bits(got[name], arrays[name]), (what, name)
    print(f"stack loop step lm={lm} couple={couple} n={n}: max |device - numpy| = {worst:.2e} (bar {BAR:.0e})")


def test_command_quaternion_is_the_pmpc_loops_log_quat(L, torch):
    """The same u0 through dart_pmpc_loop_step_dev (pmpc_loop_kernel's log_quat) and through the command launch."""
    solver, E, rows = _solver(), 5, 2
    arrays, _, _ = _step_case(L, False, E, 7, 77)
    d = _to_dev(torch, arrays)
    lg = _to_dev(torch, L.loop_logs(L.PMPC_LOOP_LOGS, rows, E))
    solver.stack_loop_step_dev(E, 7, 0, L.STACK_COMMAND, 0, 0, rows, _ptrs(d))
    solver.loop_step_dev(E, 1, 1, 0, rows, d["prm"].data_ptr(), _ptrs({"x": d["x"], "tilt": d["tilt"]}),
                         _ptrs({k: d[k] for k in ("x0", "u0", "f", "status", "iters")}), _ptrs(lg))
    solver.sync()
    assert _bits(d["tray_cmd"].cpu().numpy()[:, 3:], lg["quat_tray"].cpu().numpy()[1])


# ---- 3 / 4. the rollout ---------------------------------------------------------------------------------------------------
def _fresh(lm, n):
    from dart_mpc.harness import stack_arrays
    rows, q0, qd0, tray_pos, prm = _arms(n)
    S0, T, P = _objects()
    arrays, E, n_, lm_ = stack_arrays(S0, T, P, q0, qd0, rows, prm, tray_pos, plant_pvec=_pvec() if lm else None, Ts=TS)
    assert (E, n_, lm_) == (E_LOOP, n, lm)
    return arrays


def _run_host(L, lm, n, couple, k0, steps, rows, arrays, logs=True):
    from dart_mpc.harness import stack_logs
    lg, sl, al = stack_logs(rows, E_LOOP, n, lm) if logs is True else (logs if logs else (None, None, None))
    _solver().stack_rollout(E_LOOP, n, k0, steps, rows, arrays["arm_prm"].shape[1], arrays, lg, sl, al,
                            scfg=L.stack_config(couple), lm=lm)
    return arrays, (lg, sl, al)


@functools.lru_cache(maxsize=None)
def _full_run(lm, n, couple):
    from dart_mpc import _lib
    return _run_host(_lib, lm, n, couple, 0, K_LOOP, K_LOOP, _fresh(lm, n))


STATE = ("x", "tilt", "metrics", "q", "qd", "qdd_prev", "arm_metrics", "stack_metrics")


@pytest.mark.parametrize("n", [7, 2])
@pytest.mark.parametrize("lm", [False, True])
def test_ride_mode_is_the_two_existing_loops(L, lm, n):
    from dart_mpc.harness import rollout_dual_arm
    arrays, (lg, sl, al) = _full_run(lm, n, S.RIDE)
    rows, q0, qd0, tray_pos, prm = _arms(n)
    S0, T, P = _objects()
    fresh = _fresh(lm, n)
    # the object side: dart_pmpc[_lm]_rollout
    spec = L.PMPC_LM_LOOP_LOGS if lm else L.PMPC_LOOP_LOGS
    ol = L.loop_logs(spec, K_LOOP, E_LOOP)
    if lm:
        state = {"x": fresh["x"].copy(), "tilt": np.zeros((E_LOOP, 2)), "metrics": L.loop_metrics(E_LOOP)}
        _solver().rollout_lm(0, K_LOOP, T, P, fresh["plant_pvec"], fresh["pz_vz"], state, ol)
        assert _bits(arrays["metrics"], state["metrics"])
    else:
        state = {"x": S0.copy(), "tilt": np.zeros((E_LOOP, 2))}
        _solver().rollout(0, K_LOOP, T, P, state, ol)
    for name, _, _ in spec:
        assert _bits(lg[name], ol[name]), name
    assert _bits(arrays["x"], state["x"]) and _bits(arrays["tilt"], state["tilt"])
    # the arm side: dart_dual_arm_rollout fed tray_pos and that run's log_quat
    tray = np.concatenate([np.broadcast_to(tray_pos, (K_LOOP, E_LOOP, 3)), ol["quat_tray"]], axis=2)
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
    from dart_mpc.harness import stack_logs
    full, (lg, sl, al) = _full_run(lm, n, S.ACHIEVED)
    E, B, K = E_LOOP, 2 * E_LOOP, K_LOOP
    scfg = L.stack_config(S.ACHIEVED)

    # (a) the device form equals the host form
    d = _to_dev(torch, _fresh(lm, n))
    d["work"] = torch.zeros(L.lib().dart_stack_work_len(E, n), dtype=torch.float64, device="cuda")
    dl, ds, da = (_to_dev(torch, g) for g in stack_logs(K, E, n, lm))
    _solver().stack_rollout_dev(E, n, 0, K, K, full["arm_prm"].shape[1], _ptrs(d), _ptrs(dl), _ptrs(ds), _ptrs(da),
                                scfg=scfg, lm=lm)
    _solver().sync()
    for name in STATE:
        assert _bits(d[name].cpu().numpy(), full[name]), name
    for got, want in ((dl, lg), (ds, sl), (da, al)):
        for name in want:
            assert _bits(got[name].cpu().numpy(), want[name]), name

    # (b) 4 + 2 steps continued through k0, the state and the in/out metrics
    part, (pl, ps, pa) = _run_host(L, lm, n, S.ACHIEVED, 0, 4, K, _fresh(lm, n))
    part, _ = _run_host(L, lm, n, S.ACHIEVED, 4, 2, K, part, logs=(pl, ps, pa))
    for name in STATE:
        assert _bits(part[name], full[name]), name
    for got, want in ((pl, lg), (ps, sl), (pa, al)):
        for name in want:
            assert _bits(got[name], want[name]), name

    # (c) metrics-only
    mo, _ = _run_host(L, lm, n, S.ACHIEVED, 0, K, 0, _fresh(lm, n), logs=None)
    for name in STATE:
        assert _bits(mo[name], full[name]), name

    # (d) the same entries issued one by one from the host
    h = _to_dev(torch, _fresh(lm, n))
    SL, ML = L.lib().dart_arm_snapshot_len(n), L.lib().dart_arm_model_len(n)
    h["work"] = torch.zeros(L.lib().dart_dual_arm_work_len(E, n), dtype=torch.float64, device="cuda")
    h["snap"] = h["work"]
    h["ee_quat"] = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
    h["tray_cmd"] = torch.zeros((E, 7), dtype=torch.float64, device="cuda")
    io = _to_dev(torch, {"x0": np.zeros((E, 6)), "u0": np.zeros((E, 2)), "f": np.zeros(E), "status": np.zeros(E, np.int32),
                         "iters": np.zeros(E, np.int32)})
    h.update(io)
    hl, hs, ha = (_to_dev(torch, g) for g in stack_logs(K, E, n, lm))
    models_b = h["models"].repeat(E, 1).contiguous()
    scratch_snap = torch.zeros((B, SL), dtype=torch.float64, device="cuda")
    ident = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda").repeat(B, 1)
    dyn = ArmDynamics(_arms(n)[0][0], n)
    dcfg, qcfg = arm_dyn_config(), arm_config()
    vp = L.ctypes.c_void_p
    sv = _solver()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()            # every launch of the sequence, torch's included, on this one stream
    st = stream.cuda_stream
    sv.stack_loop_step_dev(E, n, 0, L.STACK_COUPLE, 0, 1, K, _ptrs(h), _ptrs(hl), _ptrs(hs), scfg=scfg, lm=lm, stream=st)
    for k in range(K):
        sv.solve_batch_dev(E, *(h[a].data_ptr() for a in ("x0", "target", "prm", "u0", "f", "status", "iters")), stream=st)
        sv.stack_loop_step_dev(E, n, k, L.STACK_COMMAND, 0, 0, K, _ptrs(h), scfg=scfg, lm=lm, stream=st)
        # the EE orientations of q_k (the rollout keeps them from its own dynamics launch)
        with torch.cuda.stream(stream):
            state_rows = torch.cat([h["q"], h["qd"], h["qdd_prev"], ident], dim=1).contiguous()
        dyn.dynamics_batch_dev(B, models_b.data_ptr(), False, state_rows.data_ptr(), scratch_snap.data_ptr(),
                               h["ee_quat"].data_ptr(), stream=st)
        # dynamics + QP + plant of one arm step: the arm rollout's device entry, this step's log rows
        rows_k = [ha[a][k].data_ptr() for a in L.ARM_LOOP_LOGS]
        rc = L.lib().dart_dual_arm_rollout_dev(L.ctypes.byref(dcfg), L.ctypes.byref(qcfg), E, n, 1, 1,
                                               *(vp(h[a].data_ptr()) for a in ("tray_cmd", "grasp", "models", "plant_models",
                                                                                "arm_prm")),
                                               full["arm_prm"].shape[1],
                                               *(vp(h[a].data_ptr()) for a in ("q", "qd", "qdd_prev", "arm_metrics", "work")),
                                               *(vp(p) for p in rows_k), vp(st))
        assert rc == 0
        sv.stack_loop_step_dev(E, n, k, L.STACK_COUPLE, 1, int(k + 1 < K), K, _ptrs(h), _ptrs(hl), _ptrs(hs), scfg=scfg,
                               lm=lm, stream=st)
    stream.synchronize()
    for name in STATE:
        assert _bits(h[name].cpu().numpy(), full[name]), name
    for got, want in ((hl, lg), (hs, sl), (ha, al)):
        for name in want:
            assert _bits(got[name].cpu().numpy(), want[name]), name


# ---- 5. the coupling acts -------------------------------------------------------------------------------------------------
def test_the_coupling_acts():
    from dart_mpc._lib import LOG_INT_FILL
    from dart_mpc.harness import rollout_stack
    rows, q0, qd0, tray_pos, prm = _arms(7)
    S0, T, P = _objects()
    K = 30
    kw = dict(N=N_HORIZON, Ts=TS, settle_steps=10)
    a = rollout_stack(S0, T, P, q0, qd0, rows, prm, K, tray_pos, couple="achieved", **kw)
    r = rollout_stack(S0, T, P, q0, qd0, rows, prm, K, tray_pos, couple="ride", **kw)
    Xa, Xr = (np.stack([d["X"] for d in res["logs"]]) for res in (a, r))
    assert not np.array_equal(Xa, Xr)
    print("achieved vs ride: max |X difference|", float(np.max(np.abs(Xa - Xr))),
          "stack metrics (achieved)", a["stack_metrics"].tolist())
    for res in (a, r):
        assert np.isfinite(res["metrics"]).all() and np.isfinite(res["stack_metrics"]).all()
        assert np.isfinite(res["arm"]["metrics"]).all() and np.isfinite(np.stack([d["loss"] for d in res["logs"]])).all()
        assert np.all(res["status"] != LOG_INT_FILL) and np.all(res["stack_metrics"][:, 7] == K)
        assert np.all(res["stack_metrics"][:, 6] == 0)
    # the target at the start position, the plant the controller's models: the achieved tilt stays within the tilt box
    T0 = S0.copy(); T0[:, [1, 3, 5]] = 0.0
    h = rollout_stack(S0, T0, P, q0, qd0, rows, prm, K, tray_pos, couple="achieved", plant_models=rows, **kw)
    assert np.all(h["tilt_log"] >= P[None, :, 4:5]) and np.all(h["tilt_log"] <= P[None, :, 5:6])
    print("held target: max |achieved tilt|", float(np.max(np.abs(h["tilt_log"]))))

