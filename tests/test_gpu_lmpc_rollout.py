"""Device-resident LMPC closed loop (lmpc_loop_kernel in csrc/loop_step.hip, dart_lmpc_loop_step_dev /
dart_lmpc_rollout_dev / dart_lmpc_rollout, harness.run_lmpc / rollout_lmpc).

Bars:
  * one loop step against the numpy code it restates (harness.LmpcPlant.step): absolute 1e-13.  Values are below 1 in
    magnitude; the worst amplification is 1 / I <= 100 on a few-ulp transcendental, times Ts, so the sum is a few
    1e-16 and 1e-13 leaves about 2000x over the 5.6e-17 by which the numpy and C restatements of the model differ on
    the CPU.  The kernel keeps numpy's operation order (no fma contraction), so only sin / tanh / exp can differ;
  * rollout against the same launches issued one by one, and a rollout continued by a second call: bit for bit;
  * per-step parity with the oracle chain: pvec within 1e-6 of the restated policy (the bar of test_gpu_policy.py),
    same status, |du0| <= 1e-6, the plant step within 1e-13 of oracle_lib.lmpc_rk4;
  * host loop against resident loop: |dU_cmd| <= 1e-9, |dX| <= 1e-10 (the oracle chain moves by 5.3e-12 / 1.2e-12
    when its plant is jittered by 1e-13 per step, the largest difference the first bar allows).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import lmpc_policy as lp
import oracle_lib

from loop_harness import _host, _ptrs, _same, _to_dev

pytestmark = pytest.mark.gpu

TS = 0.002
X_LO = np.array([-0.18, -0.15, -0.13, -0.15, -0.05, -0.05, -0.05, -0.05])       # workload.lmpc_batch's state ranges


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def solvers(L):
    """One LMPC handle per horizon (B_max 67), shared by the tests of this module."""
    made = {}

    def get(N):
        if N not in made:
            made[N] = L.LmpcSolver(N=N, Ts=TS, B_max=67)
        return made[N]
    yield get
    for s in made.values():
        s.close()


def _nan_io(L, B):
    return {n: (np.full((B, w) if w else (B,), np.nan) if dt is np.float64 else np.full(B, L.LOG_INT_FILL, np.int32))
            for n, w, dt in L.LMPC_LOOP_IO}


# ------------------------------------------------------------------------------------------------------------------
# Test 1: one loop-step launch against numpy
@pytest.mark.parametrize("do_post,do_pre", [(0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_lmpc_loop_step_matches_numpy(L, torch, solvers, B, do_post, do_pre):
    """Measured on one MI355X over the nine cases: max |difference| = 1.388e-17 (B = 67, post only; six of the nine
    cases agree bit for bit)."""
    from dart_mpc import harness
    rng = np.random.default_rng(500 + 10 * B + 2 * do_post + do_pre)
    state = dict(x=rng.uniform(X_LO, -X_LO, (B, 8)), tilt=rng.uniform(-0.3, 0.3, (B, 2)),
                 u_prev=rng.uniform(-0.4, 0.4, (B, 2)), model_params=rng.uniform(0.01, 1.9, (B, 34)))
    target = np.zeros((B, 8)); target[:, [0, 2]] = rng.uniform(-0.15, 0.15, (B, 2))
    pvec = rng.uniform(0.01, 1.9, (B, 34))
    io = _nan_io(L, B)
    io.update(u0=rng.uniform(-0.4, 0.4, (B, 2)), f=rng.uniform(0, 1, B), status=rng.integers(-4, 3, B).astype(np.int32),
              iters=rng.integers(1, 50, B).astype(np.int32))
    rows, k = 3, 1
    logs = L.loop_logs(L.LMPC_LOOP_LOGS, rows, B)
    ws, wio, wl = ({n: v.copy() for n, v in d.items()} for d in (state, io, logs))
    if do_post:
        wl["X"][k], wl["U_cmd"][k], wl["loss"][k] = state["x"], io["u0"], io["f"]
        wl["pvec"][k], wl["status"][k], wl["iters"][k] = state["model_params"], io["status"], io["iters"]
        ws["u_prev"] = io["u0"].copy()
        plant = harness.LmpcPlant(state["x"], pvec, dt=TS)          # tau 0.03, as dart_plant_config's default
        plant.tilt = state["tilt"].copy()
        ws["x"] = plant.step(io["u0"])
        ws["tilt"] = plant.tilt
        dx, dy = ws["x"][:, 0] - target[:, 0], ws["x"][:, 2] - target[:, 2]
        wl["pos_error"][k] = np.sqrt(dx * dx + dy * dy)
    if do_pre:
        wio["state"] = ws["x"].copy()
    ds, dio, dl = _to_dev(torch, state), _to_dev(torch, io), _to_dev(torch, logs)
    c = _to_dev(torch, dict(target=target, pvec=pvec))
    s = solvers(20)
    s.loop_step_dev(B, k, do_post, do_pre, rows, c["target"].data_ptr(), c["pvec"].data_ptr(), _ptrs(ds), _ptrs(dio),
                    _ptrs(dl))
    s.sync()
    worst = 0.0
    for got, exp, what in zip((ds, dio, dl), (ws, wio, wl), ("state", "solve I/O", "logs")):
        got = _host(got)
        for n in exp:
            if exp[n].dtype == np.float64:
                assert np.array_equal(np.isnan(got[n]), np.isnan(exp[n])), f"{what}: {n} (prefill)"
                if np.isfinite(exp[n]).any():
                    worst = max(worst, float(np.nanmax(np.abs(got[n] - exp[n]))))
                np.testing.assert_allclose(got[n], exp[n], rtol=0, atol=1e-13, equal_nan=True, err_msg=f"{what}: {n}")
            else:
                np.testing.assert_array_equal(got[n], exp[n], err_msg=f"{what}: {n}")
    print(f"lmpc loop step B={B} post={do_post} pre={do_pre}: max |difference| = {worst:.3e}")
    g = _host(dl)
    untouched = [r for r in range(rows) if not (do_post and r == k)]
    assert np.isnan(g["X"][untouched]).all() and np.all(g["status"][untouched] == L.LOG_INT_FILL)


# ------------------------------------------------------------------------------------------------------------------
# Tests 2, 3: the rollout is its launches; a second call continues it
SHAPES = [(5, 20), (40, 20), (3, 40)]       # one fused launch; the <false> + <true> pair; the two-wave build


def _inputs(B, K, seed=5):
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(3)
    pol = LmpcPolicy(B, seed=0)
    noise = np.random.default_rng(seed).standard_normal((K, B, 34)).astype(np.float32)
    return dict(x0=D["state"][:B], target=D["target"][:B], pvec=D["pvec"][:B], policy=pol, noise=noise)


def _consts(L, torch, I, B):
    return _to_dev(torch, dict(target=I["target"], prm=np.tile(L.LMPC_PRM_DEFAULT, (B, 1)), pvec=I["pvec"],
                               current_k=I["policy"].current_k, weights=I["policy"].weights, noise=I["noise"]))


def _fresh(L, torch, s, I, rows):
    B = I["x0"].shape[0]
    return _to_dev(torch, s.loop_state(I["x0"], policy=I["policy"])), _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, rows, B))


def _rollout(L, torch, s, I, rows, chunks):
    B = I["x0"].shape[0]
    st, lg = _fresh(L, torch, s, I, rows)
    c = _consts(L, torch, I, B)
    k = 0
    for n in chunks:
        s.rollout_dev(B, k, n, rows, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(), _ptrs(st),
                      _ptrs(lg), pcfg=I["policy"].cfg, weights=c["weights"].data_ptr(),
                      current_k=c["current_k"].data_ptr(), noise=c["noise"].data_ptr())
        k += n
    s.sync()
    return st, lg


def _hand_sequenced(L, torch, s, I, K):
    """The launches of a K-step rollout issued one by one, the solves alternating between w and a second buffer."""
    B = I["x0"].shape[0]
    st2, lg2 = _fresh(L, torch, s, I, K)
    io = _to_dev(torch, _nan_io(L, B))
    c = _consts(L, torch, I, B)
    other = torch.full_like(st2["w"], float("nan"))
    p, q = _ptrs(st2), _ptrs(io)
    w_in, w_out = p["w"], other.data_ptr()
    tg, pv = c["target"].data_ptr(), c["pvec"].data_ptr()
    s.loop_step_dev(B, 0, 0, 1, K, tg, pv, p, q, _ptrs(lg2))
    for k in range(K):
        s.policy_solve_batch_dev(I["policy"].cfg, B, c["weights"].data_ptr(), q["state"], p["u_prev"], tg,
                                 c["current_k"].data_ptr(), p["obs_mean"], p["obs_M2"], p["obs_count"], p["history"],
                                 p["timestep"], c["noise"].data_ptr() + 4 * 34 * B * k, p["model_params"],
                                 c["prm"].data_ptr(), q["u0"], q["f"], q["status"], q["iters"], w_warm=w_in, w_out=w_out)
        w_in, w_out = w_out, w_in
        s.loop_step_dev(B, k, 1, int(k + 1 < K), K, tg, pv, p, q, _ptrs(lg2))
    s.sync()
    if w_in != p["w"]:
        st2["w"] = other
    return st2, lg2


def _assert_same_rollout(torch, got, want):
    for a, b in zip(got, want):
        for k in a:
            assert _same(torch, a[k], b[k]), k


@pytest.mark.parametrize("B,N", SHAPES)
def test_lmpc_rollout_equals_hand_sequenced_launches(L, torch, solvers, B, N):
    K = 12
    s = solvers(N)
    I = _inputs(B, K)
    st, lg = _rollout(L, torch, s, I, K, [K])
    _assert_same_rollout(torch, (st, lg), _hand_sequenced(L, torch, s, I, K))
    h = _host(lg)
    assert not np.isnan(h["X"]).any() and not np.isnan(h["pos_error"]).any() and np.all(h["status"] != L.LOG_INT_FILL)
    assert np.all(_host(st)["timestep"] == K) and np.abs(_host(st)["w"]).max() > 0


@pytest.mark.parametrize("K", [1, 6])
def test_lmpc_rollout_warm_start_paths(L, torch, solvers, K):
    """The rollout's two ways of handing w from solve to solve give what separate buffers give: with the restoration
    phases off it rewrites w in place, with them on it alternates two buffers (K = 1: through a copy back into w)."""
    I = _inputs(5, K)
    want = None
    s_off = L.LmpcSolver(N=20, Ts=TS, B_max=8, restoration=False)
    try:
        got = _rollout(L, torch, s_off, I, K, [K])
        want = _hand_sequenced(L, torch, s_off, I, K)
        _assert_same_rollout(torch, got, want)
    finally:
        s_off.close()
    s = solvers(20)
    _assert_same_rollout(torch, _rollout(L, torch, s, I, K, [K]), _hand_sequenced(L, torch, s, I, K))
    assert np.abs(_host(got[0])["w"]).max() > 0


@pytest.mark.parametrize("B,N", SHAPES)
def test_lmpc_rollout_continues_bit_for_bit(L, torch, solvers, B, N):
    """7 steps then 5 (k0 = 7) equal 12 steps, with noise: every state array (the policy's and w included) and log."""
    s = solvers(N)
    I = _inputs(B, 12, seed=6)
    one = _rollout(L, torch, s, I, 12, [12])
    two = _rollout(L, torch, s, I, 12, [7, 5])
    for a, b in zip(one, two):
        for k in a:
            assert _same(torch, a[k], b[k]), k
    assert not np.isnan(_host(one[1])["X"]).any()


# ------------------------------------------------------------------------------------------------------------------
# Test 4: per-step parity with the oracle chain
def test_lmpc_rollout_matches_oracle_chain_per_step():
    """Measured on one MI355X: max |dpvec| = 2.168e-07, max |du0| = 1.137e-08, max |dx_next| = 1.388e-17; every solve
    ends at status 0 in at most 7 iterations, as the oracle chain does."""
    from dart_mpc import harness
    from dart_mpc.lmpc import LmpcPolicy, init_policy_weights
    from dart_mpc.workload import lmpc_batch
    B, N, K = 3, 20, 25            # the policy update fires at steps 0, 8, 16 and 24
    D = lmpc_batch(1)
    x0, tg, pvec = D["state"][:B], D["target"][:B], D["pvec"][:B]
    logs, st, X = harness.rollout_lmpc(x0, tg, pvec, K, N=N, policy_seed=0, noise_seed=7, plant_kw=dict(tau=0.0),
                                       return_logs=True)
    assert st.shape == (K, B)
    noise = np.random.default_rng(7).standard_normal((K, B, 34)).astype(np.float32)
    weights, cur_k = init_policy_weights(0), LmpcPolicy(B, seed=0).current_k
    U = np.stack([lg["u_cmd"] for lg in logs], axis=1)                  # [K, B, 2]
    Xs = np.concatenate([X["X"], X["state"]["x"][None]], axis=0)        # [K + 1, B, 8]
    np.testing.assert_array_equal(Xs[0], x0)
    dp = du = dxn = 0.0
    for b in range(B):
        ps = lp.PolicyState(cur_k[b])
        w0, up = np.zeros(8 * (N + 1) + 2 * N), np.zeros(2)
        for k in range(K):
            x = Xs[k, b]
            lp.policy_step(ps, weights, x, tg[b], up, noise[k, b])
            dp = max(dp, float(np.max(np.abs(X["pvec"][k, b] - ps.model_params))))
            assert np.max(np.abs(X["pvec"][k, b] - ps.model_params)) <= 1e-6, (b, k)
            o = oracle_lib.lmpc_solve_batch(x[None], up[None], X["pvec"][k, b][None], tg[b][None], N=N, w_init=w0[None])
            w0 = o["w"][0]
            assert int(st[k, b]) == int(o["status"][0]), (b, k, st[k, b], o["status"][0])
            du = max(du, float(np.max(np.abs(U[k, b] - o["u0"][0]))))
            assert np.max(np.abs(U[k, b] - o["u0"][0])) <= 1e-6, (b, k, U[k, b], o["u0"][0])
            xn = oracle_lib.lmpc_rk4(x[None], U[k, b][None], pvec[b][None], TS)[0]
            dxn = max(dxn, float(np.max(np.abs(Xs[k + 1, b] - xn))))
            assert np.max(np.abs(Xs[k + 1, b] - xn)) <= 1e-13, (b, k)
            np.testing.assert_array_equal(logs[b]["state"][k], Xs[k + 1, b])
            up = U[k, b]
    print(f"rollout_lmpc vs oracle chain: max|dpvec| = {dp:.3e}, max|du0| = {du:.3e}, max|dx_next| = {dxn:.3e}, "
          f"max iters = {int(X['iters'].max())}")
    # the parameters moved at the policy's update steps only
    moved = np.any(X["pvec"][1:] != X["pvec"][:-1], axis=(1, 2))
    assert set(np.where(moved)[0] + 1) == {8, 16, 24}


# ------------------------------------------------------------------------------------------------------------------
# Test 5: host loop against resident loop
def test_lmpc_host_loop_matches_resident_loop():
    """B = 4, N = 20, 50 steps, tau = 0.03, noise on.  Measured on one MI355X: max |dU_cmd| = 1.388e-17,
    max |dX| = 2.776e-17, statuses and iterations equal (all status 0, at most 7 iterations)."""
    from dart_mpc import harness
    from dart_mpc.workload import lmpc_batch
    B, N, K = 4, 20, 50
    D = lmpc_batch(1, seed0=1)
    args = (D["state"][:B], D["target"][:B], D["pvec"][:B], K)
    kw = dict(N=N, policy_seed=0, noise_seed=3, plant_kw=dict(tau=0.03), return_logs=True)
    hl, hs, hx = harness.run_lmpc(*args, **kw)
    dl, ds, dx = harness.rollout_lmpc(*args, **kw)
    du = max(float(np.max(np.abs(a["u_cmd"] - b["u_cmd"]))) for a, b in zip(hl, dl))
    dX = max(float(np.max(np.abs(hx["X"] - dx["X"]))), float(np.max(np.abs(hx["state"]["x"] - dx["state"]["x"]))))
    print(f"run_lmpc vs rollout_lmpc: max|dU_cmd| = {du:.3e}, max|dX| = {dX:.3e}, statuses {np.unique(ds).tolist()}, "
          f"max iters = {int(dx['iters'].max())}")
    assert hs.shape == ds.shape == (K, B)
    assert du <= 1e-9 and dX <= 1e-10
    np.testing.assert_array_equal(hs, ds)
    np.testing.assert_array_equal(hx["iters"], dx["iters"])
    for a, b in zip(hl, dl):
        assert set(a) == set(b) == {"pos_error", "u_cmd", "timestep", "state", "loss"}
        assert np.max(np.abs(a["pos_error"] - b["pos_error"])) <= 1e-10
        np.testing.assert_array_equal(a["timestep"], np.arange(K) * TS)


# ------------------------------------------------------------------------------------------------------------------
# Test 6: no-policy mode
def test_lmpc_rollout_without_policy(L, solvers):
    from dart_mpc.workload import lmpc_batch
    B, N, K = 2, 20, 5
    D = lmpc_batch(1, seed0=2)
    x0, tg, pvec = D["state"][:B], D["target"][:B], D["pvec"][:B]
    s = solvers(N)
    state = s.loop_state(x0, model_params=pvec)
    lg = L.loop_logs(L.LMPC_LOOP_LOGS, K, B)
    s.rollout(0, K, tg, pvec, state, lg, policy=None, plant=L.plant_config(tau=0.0))
    np.testing.assert_array_equal(state["model_params"], pvec)
    np.testing.assert_array_equal(lg["pvec"], np.broadcast_to(pvec, (K, B, 34)))
    assert np.all(state["timestep"] == 0) and np.all(state["obs_count"] == 0)        # the policy state is not touched
    np.testing.assert_array_equal(lg["X"][0], x0)
    for b in range(B):
        w0, up = np.zeros(8 * (N + 1) + 2 * N), np.zeros(2)
        for k in range(K):
            o = oracle_lib.lmpc_solve_batch(lg["X"][k, b][None], up[None], pvec[b][None], tg[b][None], N=N, w_init=w0[None])
            w0 = o["w"][0]
            assert int(lg["status"][k, b]) == int(o["status"][0]), (b, k)
            assert np.max(np.abs(lg["U_cmd"][k, b] - o["u0"][0])) <= 1e-6, (b, k, lg["U_cmd"][k, b], o["u0"][0])
            up = lg["U_cmd"][k, b]
    np.testing.assert_array_equal(state["u_prev"], lg["U_cmd"][K - 1])


# ------------------------------------------------------------------------------------------------------------------
# Test 7: errors
def test_lmpc_rollout_errors_launch_nothing(L, torch, solvers):
    s = solvers(20)
    B, K = 3, 4
    I = _inputs(B, K)
    st, lg = _fresh(L, torch, s, I, K)
    c = _consts(L, torch, I, B)
    io = _to_dev(torch, _nan_io(L, B))
    before = [{k: v.clone() for k, v in d.items()} for d in (st, lg, io)]
    cp = (c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr())
    pol = dict(pcfg=I["policy"].cfg, weights=c["weights"].data_ptr(), current_k=c["current_k"].data_ptr(),
               noise=c["noise"].data_ptr())

    def raises(match, *a, fn=s.rollout_dev, **kw):
        with pytest.raises(L.DartMPCError, match=match) as e:
            fn(*a, **kw)
        # DART_MPC_EINVAL, then dart_mpc_last_error's text (the part `match` looked for)
        assert "failed (-1): " in str(e.value) and str(e.value).split("failed (-1): ")[1].strip()

    raises("B_max", 68, 0, K, K, *cp, _ptrs(st), _ptrs(lg), **pol)
    raises("log_rows", B, 2, K - 1, K, *cp, _ptrs(st), _ptrs(lg), **pol)
    raises("negative", B, 0, -1, K, *cp, _ptrs(st), _ptrs(lg), **pol)
    raises("null", B, 0, K, K, cp[0], 0, cp[2], _ptrs(st), _ptrs(lg), **pol)
    raises("null", B, 0, K, K, *cp, {**_ptrs(st), "obs_mean": 0}, _ptrs(lg), **pol)
    raises("null", B, 0, K, K, *cp, {**_ptrs(st), "model_params": 0}, _ptrs(lg))           # required without a policy too
    raises("policy config", B, 0, K, K, *cp, _ptrs(st), _ptrs(lg), **{**pol, "pcfg": None})
    raises("log_rows", B, K, 1, 0, K, cp[0], cp[2], _ptrs(st), _ptrs(io), _ptrs(lg), fn=s.loop_step_dev)
    pm = L.Solver(N=20, Ts=TS, B_max=4)         # a PMPC handle given to the LMPC entries
    try:
        raises("not an LMPC handle", pm, B, 0, K, K, *cp, _ptrs(st), _ptrs(lg), fn=L.LmpcSolver.rollout_dev, **pol)
        raises("not an LMPC handle", pm, B, 0, 1, 1, K, cp[0], cp[2], _ptrs(st), _ptrs(io), _ptrs(lg),
               fn=L.LmpcSolver.loop_step_dev)
    finally:
        pm.close()
    with pytest.raises(L.DartMPCError, match="not a PMPC handle"):      # and an LMPC handle to the PMPC entry
        L.Solver.rollout_dev(s, B, 0, K, K, cp[0], cp[1], {"x": st["x"].data_ptr(), "tilt": st["tilt"].data_ptr()},
                             {n: lg["X"].data_ptr() for n, _, _ in L.PMPC_LOOP_LOGS})
    s.rollout_dev(B, 0, 0, K, *cp, _ptrs(st), _ptrs(lg), **pol)        # steps = 0: OK, touches nothing
    s.sync()
    torch.cuda.synchronize()
    for a, b in zip((st, lg, io), before):
        for k in a:
            assert _same(torch, a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------
# Test 8: a process that exits with the solver open (the atexit path of dart_mpc/_lib.py)
_CHILD = """
import numpy as np
from dart_mpc import _lib
from dart_mpc.lmpc import LmpcPolicy
from dart_mpc.workload import lmpc_batch
D = lmpc_batch(1)
s = _lib.LmpcSolver(N=20, B_max=4)
pol = LmpcPolicy(2, seed=0)
st = s.loop_state(D["state"][:2], policy=pol); lg = _lib.loop_logs(_lib.LMPC_LOOP_LOGS, 3, 2)
s.rollout(0, 3, D["target"][:2], D["pvec"][:2], st, lg, policy=pol)
assert not np.isnan(lg["X"]).any() and (st["timestep"] == 3).all()
print("rolled", int(lg["iters"].sum()))
"""


def test_child_exits_cleanly_with_an_open_lmpc_solver():
    from dart_mpc import _lib
    pkg_root = os.path.dirname(_lib.PKG_DIR)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg_root, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "rolled" in r.stdout
