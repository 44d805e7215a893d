"""The cross-plant loops (PMPC / RMPC on harness.LmpcPlant) without a GPU: the sign of the tilt and the point-mass
reduction of the LMPC plant, the numpy statement of the streaming metrics against AsyncLogger's, and the six new
symbols (added within ABI 8).

Bars:
  * LmpcPlant(point_mass_pvec(mu, m)) driven by -u against TrayPlant(mu, mu_c=0) driven by u: |dx[:, :4]| <= 1e-6
    over 200 steps.  The two differ by the model's 1e-6 parameter squashing (a residual spring and radius), measured
    1.34e-7 over the 200 steps; with the same sign on both sides the difference is 9.4e-4 after ONE step, so the bar
    separates right from wrong;
  * rollout_metrics against logger_metrics: relative 1e-12 (numpy sums pairwise, the accumulator sequentially; a sum
    of K <= 200 non-negative terms differs by at most K ulp ~ 4e-14 relative).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dart_pmpc_lm_loop_step_dev", "dart_pmpc_lm_rollout_dev", "dart_pmpc_lm_rollout",
       "dart_rmpc_lm_loop_step_dev", "dart_rmpc_lm_rollout_dev", "dart_rmpc_lm_rollout")


def _plants(seed=0, B=16):
    from dart_mpc import harness
    from dart_mpc.workload import point_mass_pvec
    rng = np.random.default_rng(seed)
    mu, m = rng.uniform(0.05, 0.6, B), rng.uniform(0.2, 1.5, B)
    x4 = np.stack([rng.uniform(-0.15, 0.15, B), rng.uniform(-0.1, 0.1, B), rng.uniform(-0.12, 0.12, B),
                   rng.uniform(-0.1, 0.1, B)], axis=1)
    x6 = np.zeros((B, 6)); x6[:, :4] = x4; x6[:, 4] = 0.43
    x8 = np.zeros((B, 8)); x8[:, :4] = x4
    tray = harness.TrayPlant(x6, mu, tau=0.03, mu_c=0.0)
    lm = harness.LmpcPlant(x8, point_mass_pvec(mu, m), tau=0.03)
    return rng, tray, lm


def test_point_mass_pvec_layout():
    from dart_mpc.workload import point_mass_pvec
    p = point_mass_pvec([0.1, 0.3], m=[0.5, 2.0])
    assert p.shape == (2, 34)
    want = np.zeros((2, 34))
    want[:, 0] = want[:, 1] = [0.5, 2.0]
    want[:, 2] = want[:, 3] = [0.05, 0.6]
    want[:, 16:18] = 1.0
    np.testing.assert_array_equal(p, want)
    assert point_mass_pvec(0.2).shape == (1, 34) and point_mass_pvec(0.2)[0, 0] == 1.0


def test_lmpc_plant_with_flipped_command_reduces_to_the_tray_plant():
    rng, tray, lm = _plants()
    B, worst = tray.x.shape[0], 0.0
    for _ in range(200):
        u = rng.uniform(-0.4, 0.4, (B, 2))
        tray.step(u)
        lm.step(-u)
        worst = max(worst, float(np.max(np.abs(lm.x[:, :4] - tray.x[:, :4]))))
        np.testing.assert_array_equal(lm.tilt, -tray.tilt)
    print(f"LmpcPlant(point mass, -u) vs TrayPlant(mu_c = 0, u): max |dx[:4]| over 200 steps = {worst:.3e}")
    assert worst <= 1e-6
    assert np.all(lm.x[:, 4:] == 0.0)                      # no rotation is excited


def test_the_same_sign_on_both_sides_is_far_outside_the_bar():
    rng, tray, lm = _plants()
    u = rng.uniform(-0.4, 0.4, (tray.x.shape[0], 2))
    tray.step(u)
    lm.step(u)
    assert float(np.max(np.abs(lm.x[:, :4] - tray.x[:, :4]))) > 1e-4


def _synthetic(rng, K, start, never=False, at0=False):
    """One experiment's logs: the error decays from `start`; never: it stays above 1 cm; at0: below it from step 0."""
    target = np.array([0.05, 0.0, -0.03, 0.0, 0.4, 0.0])
    decay = np.exp(-np.arange(K) / (K / 6.0))
    e = start * decay + (0.02 if never else 0.0)
    if at0:
        e = 0.005 * decay
    ang = rng.uniform(0, 2 * np.pi, K)
    X = np.zeros((K, 6))
    X[:, 0] = target[0] + e * np.cos(ang); X[:, 2] = target[2] + e * np.sin(ang)
    X[:, [1, 3]] = rng.uniform(-0.1, 0.1, (K, 2)); X[:, 4] = 0.4
    U = rng.uniform(-0.5, 0.5, (K, 2))
    st = (rng.uniform(size=K) < 0.2).astype(np.int32) * rng.choice([-2, 1, 2], K).astype(np.int32)
    it = rng.integers(3, 40, K).astype(np.int32)
    rot = rng.uniform(-0.2, 0.2, (K, 4))
    return X, target, U, st, it, rot


def test_rollout_metrics_against_logger_metrics():
    from dart_mpc import harness
    rng = np.random.default_rng(2)
    Ts = 0.002
    for K, kw in ((200, {}), (57, dict(never=True)), (33, dict(at0=True)), (1, {})):
        X, target, U, st, it, rot = _synthetic(rng, K, 0.08, **kw)
        m = harness.rollout_metrics(X, target, U, st, it, rot, Ts)
        assert m.shape == (8,)
        t = np.arange(K) * Ts
        ref = harness.logger_metrics({"X": X, "X_target": np.tile(target, (K, 1)), "t": t, "U_cmd": U}, Ts)
        rel = lambda a, b: abs(a - b) <= 1e-12 * abs(b)
        assert rel(m[0], ref["steady_state_error"]) and rel(m[2], ref["control_effort"])
        conv = Ts * m[1] if m[1] >= 0 else t[-1]
        assert rel(conv, ref["convergence_time"]) or conv == ref["convergence_time"] == 0.0
        e = np.linalg.norm(X[:, [0, 2]] - target[[0, 2]], axis=1)
        if kw.get("never"):
            assert m[1] == -1.0 and ref["convergence_time"] == t[-1] and e.min() >= 0.01
        if kw.get("at0"):
            assert m[1] == 0.0 and ref["convergence_time"] == 0.0
        if not kw and K > 1:
            assert 0 < m[1] < K - 1                              # the threshold is crossed inside the run
        assert rel(m[3], e.max()) and m[4] == np.sum(st != 0) and m[5] == it.sum() and m[7] == K
        assert m[6] == np.abs(rot[:, [0, 2]]).max()


def test_rollout_metrics_batched_and_continued():
    """[K, B] logs give the per-experiment rows, and K1 + K2 steps continued from the first call's metrics give bit for
    bit one call of K1 + K2."""
    from dart_mpc import harness
    rng = np.random.default_rng(3)
    runs = [_synthetic(rng, 40, s) for s in (0.08, 0.03, 0.2)]
    X, U, st, it, rot = (np.stack([r[i] for r in runs], axis=1) for i in (0, 2, 3, 4, 5))
    target = np.stack([r[1] for r in runs])
    M = harness.rollout_metrics(X, target, U, st, it, rot, 0.002)
    assert M.shape == (3, 8)
    for b, r in enumerate(runs):
        np.testing.assert_array_equal(M[b], harness.rollout_metrics(r[0], r[1], r[2], r[3], r[4], r[5], 0.002))
    M1 = harness.rollout_metrics(X[:17], target, U[:17], st[:17], it[:17], rot[:17], 0.002)
    M2 = harness.rollout_metrics(X[17:], target, U[17:], st[17:], it[17:], rot[17:], 0.002, metrics=M1, k0=17)
    np.testing.assert_array_equal(M2, M)
    fresh = harness.rollout_metrics(X[:0], target, U[:0], st[:0], it[:0], rot[:0], 0.002)
    from dart_mpc import _lib
    np.testing.assert_array_equal(fresh, _lib.loop_metrics(3))


def test_new_symbols_declared_and_exported_within_abi_8():
    from dart_mpc import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "dart_mpc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint %s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS
    assert L.dart_mpc_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_null_handle_is_einval():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in NEW:
        fn = getattr(L, n)
        args = [None if t is _lib.ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -1, n


def test_layout_tables_and_signatures():
    import inspect
    from dart_mpc import _lib, harness
    assert [n for n, _, _ in _lib.PMPC_LM_LOOP_STATE] == ["x", "tilt", "metrics"]
    assert [n for n, _, _ in _lib.RMPC_LM_LOOP_STATE] == ["x", "tilt", "prev", "u_prev", "r_v", "theta", "P", "w", "done",
                                                         "nlog", "metrics"]
    assert dict((n, w) for n, w, _ in _lib.RMPC_LM_LOOP_STATE)["x"] == 8
    assert _lib.PMPC_LM_LOOP_LOGS[-1][:2] == _lib.RMPC_LM_LOOP_LOGS[-1][:2] == ("rot", 4)
    assert len(_lib.METRIC_SLOTS) == 8
    for fn in (harness.run_pmpc, harness.run_rmpc, harness.rollout_pmpc, harness.rollout_rmpc):
        sig = inspect.signature(fn).parameters
        assert sig["plant_pvec"].default is None and sig["x_rot0"].default is None
    for fn in (harness.rollout_pmpc, harness.rollout_rmpc):
        assert inspect.signature(fn).parameters["metrics_only"].default is False
