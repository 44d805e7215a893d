"""The LMPC evaluation (dart_lmpc_eval*, harness.population_scores / evaluate_lmpc) without a GPU: the numpy statement
of the score reduction against rows worked out by hand, the Python tables against the header's widths, and
evaluate_lmpc's promise that a policy passed in is not advanced (the library call replaced by a stand-in).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dart_lmpc_eval_loop_step_dev", "dart_lmpc_eval_dev", "dart_lmpc_eval", "dart_lmpc_eval_scores_dev",
       "dart_lmpc_eval_scores")


def test_population_scores_hand_computed_rows():
    from dart_mpc.harness import population_scores
    # slots: e, convergence step, effort, max e, bad steps, iters, rotation, steps
    M = np.array([
        [[0.25, 4.0, 1.0, 0.5, 0.0, 30.0, 0.125, 10.0],       # learner 0: two of three converged
         [0.5, -1.0, 2.0, 0.75, 2.0, 50.0, 0.5, 10.0],
         [0.75, 8.0, 3.0, 0.25, 1.0, 40.0, 0.25, 10.0]],
        [[0.5, -1.0, 0.5, 0.5, 0.0, 8.0, 0.0, 4.0],           # learner 1: nobody converged
         [1.5, -1.0, 0.25, 1.5, 4.0, 8.0, 0.0, 4.0],
         [1.0, -1.0, 0.75, 1.0, 0.0, 8.0, 0.0, 4.0]],
        [[0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],           # learner 2: a fresh run, no step taken
         [0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
         [0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]])
    want = np.array([[0.5, 2.0 / 3.0, 6.0, 2.0, 0.75, 3.0, 4.0, 0.5],
                     [1.0, 0.0, -1.0, 0.5, 1.5, 4.0, 2.0, 0.0],
                     [0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    got = population_scores(M)
    assert got.shape == (3, 8) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)


def test_population_scores_one_instance_and_step_zero():
    from dart_mpc.harness import population_scores
    # B = 1; converged at step 0 counts as converged (slot 1 = 0 is not "none")
    M = np.array([[[0.004, 0.0, 0.3, 0.2, 1.0, 21.0, 0.01, 3.0]]])
    np.testing.assert_array_equal(population_scores(M), [[0.004, 1.0, 0.0, 0.3, 0.2, 1.0, 7.0, 0.01]])


def test_population_scores_sums_in_instance_order():
    """The mean is the sequential sum over b = 0, 1, 2 divided by B: 1 + 1e-16 + 1e-16 stays 1 from the left (numpy's
    own sum of these three gives the same here; summed from the right it would be 1 + 2e-16)."""
    from dart_mpc.harness import population_scores
    M = np.zeros((1, 3, 8)); M[0, :, 1] = -1.0
    M[0, :, 0] = [1.0, 1e-16, 1e-16]
    assert population_scores(M)[0, 0] == ((1.0 + 1e-16) + 1e-16) / 3.0 == 1.0 / 3.0


def test_eval_tables_agree_with_the_header():
    from dart_mpc import _lib
    assert _lib.LMPC_EVAL_STATE == _lib.LMPC_LOOP_STATE + (("metrics", 8, np.float64),)
    assert len(_lib.SCORE_SLOTS) == 8 == len(set(_lib.SCORE_SLOTS)) == len(_lib.METRIC_SLOTS)
    assert _lib.SCORE_SLOTS[0] == "mean_steady_state_error" and _lib.SCORE_SLOTS[7] == "max_rotation"
    src = open(os.path.join(ROOT, "include", "dart_mpc.h")).read()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert n in _lib.EXPORTS
    # the widths the header states for the evaluation's own arrays
    assert "metrics [.][8]" in src and "scores [P][8]" in src and "[P][39748]; learner l's" in src
    assert _lib.ACTOR_NWEIGHTS == 39748
    # one pointer per entry of the tables, in the header's order
    decl = re.search(r"int dart_lmpc_eval_dev\((.*?)\);", src, re.S).group(1)
    names = [a.split("*")[-1].strip() for a in decl.split(",") if "*" in a]
    state = [n for n, _, _ in _lib.LMPC_EVAL_STATE]
    logs = ["log_" + {"U_cmd": "U"}.get(n, n) for n, _, _ in _lib.LMPC_LOOP_LOGS]
    assert names == (["h", "plant", "pcfg", "target", "prm", "plant_pvec", "current_k", "weights", "noise"] + state
                     + ["scores"] + logs + ["hip_stream"])
    assert decl.count("int ") == 5
    lib = _lib.lib()
    assert len(lib.dart_lmpc_eval_dev.argtypes) == len(names) + 5 == len(lib.dart_lmpc_eval.argtypes)
    assert len(lib.dart_lmpc_eval_loop_step_dev.argtypes) == 27


class _FakeSolver:
    """Stands in for _lib.LmpcSolver: ``evaluate`` advances every state array it is handed, as the device would."""
    made = []

    def __init__(self, N=20, Ts=0.002, B_max=1, device=0):
        self.nw = 8 * (N + 1) + 2 * N
        self.B_max, self.calls, self.closed = B_max, [], False
        _FakeSolver.made.append(self)

    def loop_state(self, x0, policy=None, model_params=None):
        return _FakeSolver.real.loop_state(self, x0, policy=policy, model_params=model_params)

    def evaluate(self, P, k0, steps, target, plant_pvec, state, logs, **kw):
        self.calls.append(dict(P=P, k0=k0, steps=steps, target=target, plant_pvec=plant_pvec, logs=logs, kw=kw,
                               shapes={n: v.shape for n, v in state.items()}))
        for v in state.values():
            v += 1
        kw["scores"][:] = np.arange(8 * P).reshape(P, 8)
        if logs is not None:
            for v in logs.values():
                v[...] = 0

    def close(self):
        self.closed = True


def test_evaluate_lmpc_copies_the_policies_state(monkeypatch):
    from dart_mpc import _lib, harness
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    _FakeSolver.real = _lib.LmpcSolver
    monkeypatch.setattr(_lib, "LmpcSolver", _FakeSolver)
    _FakeSolver.made.clear()
    B, P, K = 3, 2, 5
    D = lmpc_batch(1)
    pols = [LmpcPolicy(B, seed=s) for s in range(P)]
    rng = np.random.default_rng(0)
    for p in pols:      # a training state under way
        p.obs_mean[:] = rng.uniform(-1, 1, p.obs_mean.shape); p.obs_M2[:] = rng.uniform(0, 1, p.obs_M2.shape)
        p.obs_count[:] = 40; p.timestep[:] = 40
        p.history[:] = rng.uniform(-1, 1, p.history.shape).astype(np.float32)
        p.model_params[:] = rng.uniform(0.1, 1.0, p.model_params.shape)
    names = ("weights", "current_k", "model_params", "obs_mean", "obs_M2", "obs_count", "timestep", "history")
    before = [{n: getattr(p, n).copy() for n in names} for p in pols]
    x0, tg, pv = D["state"][:B].copy(), D["target"][:B].copy(), D["pvec"][:B].copy()
    keep = [a.copy() for a in (x0, tg, pv)]
    out = harness.evaluate_lmpc(x0, tg, pv, K, pols, N=10, noise_seed=3)
    for p, was in zip(pols, before):
        for n in names:
            np.testing.assert_array_equal(getattr(p, n), was[n], err_msg=n)
    for a, was in zip((x0, tg, pv), keep):
        np.testing.assert_array_equal(a, was)
    s, = _FakeSolver.made
    c, = s.calls
    assert s.closed and s.B_max == P * B and c["P"] == P and c["k0"] == 0 and c["steps"] == K and c["logs"] is None
    assert c["shapes"]["x"] == (P * B, 8) and c["shapes"]["metrics"] == (P * B, 8) and c["shapes"]["history"] == (P * B, 520)
    # every learner sees the same experiments and the same draws, its own weights and current_k
    np.testing.assert_array_equal(c["target"], np.tile(tg, (P, 1)))
    np.testing.assert_array_equal(c["plant_pvec"], np.tile(pv, (P, 1)))
    nz = c["kw"]["noise"]
    assert nz.shape == (K, P * B, 34) and nz.dtype == np.float32
    np.testing.assert_array_equal(nz[:, :B], harness.lmpc_noise(3, K, B))
    np.testing.assert_array_equal(nz[:, B:], nz[:, :B])
    np.testing.assert_array_equal(c["kw"]["weights"], np.stack([p.weights for p in pols]))
    np.testing.assert_array_equal(c["kw"]["current_k"], np.concatenate([p.current_k for p in pols]))
    # a fresh run's metrics went in (zeros, slot 1 = -1; the stand-in added one), [P, B, 8] comes out
    assert out["metrics"].shape == (P, B, 8) and np.all(out["metrics"][..., 1] == 0.0) and np.all(out["metrics"][..., 0] == 1.0)
    np.testing.assert_array_equal(out["scores"], np.arange(8 * P).reshape(P, 8))
    assert set(out) == {"metrics", "scores"}


def test_evaluate_lmpc_default_is_zero_noise_and_logs_on_request(monkeypatch):
    from dart_mpc import _lib, harness
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    _FakeSolver.real = _lib.LmpcSolver
    monkeypatch.setattr(_lib, "LmpcSolver", _FakeSolver)
    _FakeSolver.made.clear()
    B, K = 2, 4
    D = lmpc_batch(1)
    out = harness.evaluate_lmpc(D["state"][:B], D["target"][:B], D["pvec"][:B], K, LmpcPolicy(B), N=10,
                                metrics_only=False)
    c, = _FakeSolver.made[0].calls
    assert c["P"] == 1 and c["kw"]["noise"] is None
    assert c["logs"] is not None and c["logs"]["X"].shape == (K, B, 8) and c["logs"]["pvec"].shape == (K, B, 34)
    assert len(out["logs"]) == 1 and len(out["logs"][0]) == B and out["status"][0].shape == (K, B)
    assert set(out["logs"][0][0]) == {"pos_error", "u_cmd", "timestep", "state", "loss"}
    # no policy: one "learner", the plant's parameters as the model
    out = harness.evaluate_lmpc(D["state"][:B], D["target"][:B], D["pvec"][:B], K, None, N=10)
    c, = _FakeSolver.made[1].calls
    assert c["P"] == 1 and c["kw"]["weights"] is None and c["kw"]["pcfg"] is None and out["metrics"].shape == (1, B, 8)
