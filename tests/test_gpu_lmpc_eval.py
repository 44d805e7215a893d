"""Evaluation of a population of LMPC policies in one device-resident rollout (lmpc_eval_loop_kernel and
lmpc_eval_scores_kernel in csrc/loop_step.hip; dart_lmpc_eval_loop_step_dev / dart_lmpc_eval_dev / dart_lmpc_eval /
dart_lmpc_eval_scores*; harness.population_scores).

Bars:
  * next x, tilt, u_prev, state and the log rows against dart_lmpc_loop_step_dev / dart_lmpc_rollout_dev on the same
    inputs: bit for bit (the evaluation's kernel restates that kernel's expressions in their order);
  * metrics against harness.rollout_metrics: bit for bit in slots 1, 4, 5, 6, 7 (comparisons, counts, sums of small
    integers, a maximum of inputs), relative 1e-12 in slots 0, 2, 3, which pass through a square root (the bars of
    tests/test_gpu_cross_plant.py: the device's sqrt and numpy's may differ by an ulp, 1.1e-16 relative, and slot 2
    sums at most 12 such terms here);
  * a population against its members' single runs, chunked against whole calls, metrics-only against logging, the host
    entry against the device entry: bit for bit;
  * scores against harness.population_scores: bit for bit in all eight slots (sequential fp64 sums in instance order
    and IEEE division on both sides).
The closed-loop cases compare two device paths with each other; a solve that leaves status 0 is not a failure here.
"""
import numpy as np
import pytest

from loop_harness import L, TS, X_LO, _bits, _host, _metrics_midrun, _ptrs, _to_dev, torch  # noqa: F401

pytestmark = pytest.mark.gpu

N, B_MAX = 10, 33
EXACT, ROOTED = [1, 4, 5, 6, 7], [0, 2, 3]


@pytest.fixture(scope="module")
def solver(L):
    s = L.LmpcSolver(N=N, Ts=TS, B_max=B_MAX)
    yield s
    s.close()


def _assert_metrics(got, want, what):
    """The bars of the metrics against the numpy statement; returns the largest relative difference of the rooted
    slots."""
    got, want = got.reshape(-1, 8), want.reshape(-1, 8)
    assert _bits(got[:, EXACT], want[:, EXACT]), f"{what}: slots 1, 4, 5, 6, 7"
    rel = np.abs(got[:, ROOTED] - want[:, ROOTED]) / np.maximum(np.abs(want[:, ROOTED]), 1e-300)
    rel = np.where(got[:, ROOTED] == want[:, ROOTED], 0.0, rel)
    print(f"{what}: metrics slots 0, 2, 3 max relative difference = {rel.max():.3e}")
    np.testing.assert_allclose(got[:, ROOTED], want[:, ROOTED], rtol=1e-12, atol=0, err_msg=f"{what}: slots 0, 2, 3")
    return float(rel.max())


# ------------------------------------------------------------------------------------------------------------------
# Test 1: one loop step against numpy and against the rollout's loop step
@pytest.mark.parametrize("do_post,do_pre", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("B", [33, 3])       # a full block of 32 groups plus a block that holds one; one partial block
def test_eval_loop_step(L, torch, solver, B, do_post, do_pre):
    from dart_mpc import harness
    rng = np.random.default_rng(900 + 10 * B + 2 * do_post + do_pre)
    state = dict(x=rng.uniform(X_LO, -X_LO, (B, 8)), tilt=rng.uniform(-0.3, 0.3, (B, 2)),
                 u_prev=rng.uniform(-0.4, 0.4, (B, 2)), model_params=rng.uniform(0.01, 1.9, (B, 34)))
    target = np.zeros((B, 8)); target[:, [0, 2]] = rng.uniform(-0.15, 0.15, (B, 2))
    target[1, 0], target[1, 2] = state["x"][1, 0] + 1e-3, state["x"][1, 2] - 2e-3        # within 1 cm: converges at k
    pvec = rng.uniform(0.01, 1.9, (B, 34))
    io = {n: (np.full((B, w) if w else (B,), np.nan) if dt is np.float64 else np.full(B, L.LOG_INT_FILL, np.int32))
          for n, w, dt in L.LMPC_LOOP_IO}
    io.update(u0=rng.uniform(-0.4, 0.4, (B, 2)), f=rng.uniform(0, 1, B), status=rng.integers(-4, 3, B).astype(np.int32),
              iters=rng.integers(1, 50, B).astype(np.int32))
    io["status"][0], io["status"][-1] = 0, -2           # (both kinds of status, whatever was drawn)
    metrics = _metrics_midrun(L, B)
    rows, k = 3, 2
    c = _to_dev(torch, dict(target=target, pvec=pvec))
    tg, pv = c["target"].data_ptr(), c["pvec"].data_ptr()

    def run(entry, with_metrics, with_logs):
        st = dict(state, metrics=metrics) if with_metrics else state
        ds, dio, dl = _to_dev(torch, st), _to_dev(torch, io), _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, rows, B))
        entry(B, k, do_post, do_pre, rows, tg, pv, _ptrs(ds), _ptrs(dio), _ptrs(dl) if with_logs else None)
        solver.sync()
        return _host(ds), _host(dio), _host(dl)

    ref = run(solver.loop_step_dev, False, True)
    got = run(solver.eval_loop_step_dev, True, True)
    quiet = run(solver.eval_loop_step_dev, True, False)
    for what, (s, q, lg) in (("logging", got), ("metrics-only", quiet)):
        for n in ("x", "tilt", "u_prev", "model_params"):
            assert _bits(s[n], ref[0][n]), f"{what}: {n}"
        for n in q:
            assert _bits(q[n], ref[1][n]), f"{what}: {n}"
    for n in ref[2]:
        assert _bits(got[2][n], ref[2][n]), f"log {n}"
        fill = L.loop_logs(L.LMPC_LOOP_LOGS, rows, B)[n]
        assert _bits(quiet[2][n], fill), f"metrics-only wrote log {n}"
    assert _bits(quiet[0]["metrics"], got[0]["metrics"])
    if do_post:
        want = harness.rollout_metrics(state["x"][None], target, io["u0"][None], io["status"][None], io["iters"][None],
                                       state["x"][None, :, 4:], TS, metrics=metrics, k0=k)
        assert metrics[1, 1] == -1.0 and want[1, 1] == float(k)            # the near instance converges at this step
        _assert_metrics(got[0]["metrics"], want, f"eval loop step B={B} post={do_post} pre={do_pre}")
        assert not _bits(got[0]["metrics"], metrics)
    else:
        assert _bits(got[0]["metrics"], metrics)


# ------------------------------------------------------------------------------------------------------------------
# Tests 2 .. 6: the closed loop.  One case (N = 10, B = 3, P = 3, 12 steps, noise on) and its reference runs, computed
# once per module and left unchanged.
P, B, K = 3, 3, 12


def _case(L, seeds=(0, 1, 0), with_policy=True, learners=P, rows=(0, 3, 6)):
    """``learners`` learners of B instances: learner l has the policy of seed ``seeds[l]`` and the experiments of the
    workload's rows ``rows[l]`` .. + B (learner 2: learner 0's policy on other experiments)."""
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    pick = np.concatenate([np.arange(r, r + B) for r in rows[:learners]])
    pols = [LmpcPolicy(B, seed=s) for s in seeds[:learners]] if with_policy else None
    noise = np.random.default_rng(11).standard_normal((K, learners * B, 34)).astype(np.float32)
    C = dict(P=learners, x0=D["state"][pick], target=D["target"][pick], pvec=D["pvec"][pick], policies=pols, noise=noise,
             prm=np.tile(L.LMPC_PRM_DEFAULT, (learners * B, 1)))
    if with_policy:
        C["weights"] = np.stack([p.weights for p in pols])
        C["current_k"] = np.concatenate([p.current_k for p in pols])
    return C


def _member(C, l):
    """Learner l's own arrays, for the single-policy entries."""
    sl = slice(l * B, (l + 1) * B)
    return dict(P=1, x0=C["x0"][sl], target=C["target"][sl], pvec=C["pvec"][sl], policies=[C["policies"][l]],
                noise=np.ascontiguousarray(C["noise"][:, sl]), prm=C["prm"][sl], weights=C["weights"][l:l + 1],
                current_k=C["current_k"][sl])


def _fresh_state(L, s, C, metrics=True):
    if C["policies"] is None:
        st = s.loop_state(C["x0"], model_params=C["pvec"])
    else:
        parts = [s.loop_state(C["x0"][l * B:(l + 1) * B], policy=p) for l, p in enumerate(C["policies"])]
        st = {n: np.concatenate([q[n] for q in parts]) for n in parts[0]}
    if metrics:
        st["metrics"] = L.loop_metrics(st["x"].shape[0])
    return st


def _policy_args(torch, C):
    if C["policies"] is None:
        return {}, None
    d = _to_dev(torch, dict(weights=C["weights"], current_k=C["current_k"], noise=C["noise"]))
    return dict(pcfg=C["policies"][0].cfg, weights=d["weights"].data_ptr(), current_k=d["current_k"].data_ptr(),
                noise=d["noise"].data_ptr()), d


def _evaluate(L, torch, s, C, chunks=(K,), logs=True, scores=True, host=False):
    """(state, logs or None, scores or None) as host arrays after evaluate_dev (or the host entry) over ``chunks``."""
    NI = C["x0"].shape[0]
    st = _fresh_state(L, s, C)
    lg = L.loop_logs(L.LMPC_LOOP_LOGS, K, NI) if logs else None
    sc = np.full((C["P"], 8), np.nan) if scores else None
    k = 0
    if host:
        pol = {} if C["policies"] is None else dict(pcfg=C["policies"][0].cfg, weights=C["weights"],
                                                    current_k=C["current_k"], noise=C["noise"])
        for n in chunks:
            s.evaluate(C["P"], k, n, C["target"], C["pvec"], st, lg, prm=C["prm"], scores=sc, rows=K, **pol)
            k += n
        return st, lg, sc
    c = _to_dev(torch, dict(target=C["target"], prm=C["prm"], pvec=C["pvec"]))
    pol, keep = _policy_args(torch, C)
    ds, dl = _to_dev(torch, st), (_to_dev(torch, lg) if logs else None)
    dsc = _to_dev(torch, dict(s=sc))["s"] if scores else None
    for n in chunks:
        s.evaluate_dev(C["P"], NI // C["P"], k, n, K, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(),
                       _ptrs(ds), _ptrs(dl), scores=dsc.data_ptr() if scores else 0, **pol)
        k += n
    s.sync()
    return _host(ds), (_host(dl) if logs else None), (dsc.cpu().numpy() if scores else None)


def _rollout(L, torch, s, C):
    """dart_lmpc_rollout_dev on the same arrays (one policy, or none, for all instances)."""
    NI = C["x0"].shape[0]
    c = _to_dev(torch, dict(target=C["target"], prm=C["prm"], pvec=C["pvec"]))
    pol, keep = _policy_args(torch, C)
    ds, dl = _to_dev(torch, _fresh_state(L, s, C, metrics=False)), _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, K, NI))
    s.rollout_dev(NI, 0, K, K, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(), _ptrs(ds), _ptrs(dl), **pol)
    s.sync()
    return _host(ds), _host(dl)


@pytest.fixture(scope="module")
def runs(L, torch, solver):
    """The population's logging run in one call, and every member's rollout alone."""
    C = _case(L)
    return dict(C=C, pop=_evaluate(L, torch, solver, C), single=[_rollout(L, torch, solver, _member(C, l)) for l in range(P)])


def _same_run(got, want, what, sl=slice(None)):
    for n in want[0]:
        assert _bits(got[0][n][sl], want[0][n]), f"{what}: state {n}"
    if want[1] is not None:
        for n in want[1]:
            assert _bits(got[1][n][:, sl], want[1][n]), f"{what}: log {n}"


def test_population_equals_single_rollouts(L, torch, solver, runs):
    from dart_mpc import harness
    st, lg, sc = runs["pop"]
    assert not np.isnan(lg["X"]).any() and np.all(lg["status"] != L.LOG_INT_FILL) and np.all(st["timestep"] == K)
    for l in range(P):
        _same_run((st, lg), runs["single"][l], f"learner {l}", slice(l * B, (l + 1) * B))
    # learners 0 and 1 differ in their weights, 0 and 2 in their experiments: nobody is compared with a twin
    assert not _bits(lg["pvec"][:, 0:B], lg["pvec"][:, B:2 * B]) and not _bits(lg["X"][:, 0:B], lg["X"][:, 2 * B:])
    want = harness.rollout_metrics(lg["X"], runs["C"]["target"], lg["U_cmd"], lg["status"], lg["iters"], lg["X"][:, :, 4:], TS)
    _assert_metrics(st["metrics"], want, "population, 12 steps")
    assert np.all(st["metrics"][:, 7] == K)
    # a population of one is the rollout, bit for bit
    one = _evaluate(L, torch, solver, _member(runs["C"], 1))
    _same_run(one, runs["single"][1], "P = 1")
    assert _bits(one[0]["metrics"], st["metrics"][B:2 * B])


def test_learners_are_isolated(L, torch, solver, runs):
    C = dict(runs["C"])
    C["weights"] = C["weights"].copy()
    C["weights"][1] += np.float32(1e-3)
    st, lg, sc = _evaluate(L, torch, solver, C)
    ref = runs["pop"]
    for l in (0, 2):
        sl = slice(l * B, (l + 1) * B)
        for n in st:
            assert _bits(st[n][sl], ref[0][n][sl]), f"learner {l}: state {n}"
        for n in lg:
            assert _bits(lg[n][:, sl], ref[1][n][:, sl]), f"learner {l}: log {n}"
        assert _bits(sc[l], ref[2][l])
    assert not _bits(lg["pvec"][:, B:2 * B], ref[1]["pvec"][:, B:2 * B])        # (the perturbation acts)


def test_chaining_and_modes(L, torch, solver, runs):
    ref = runs["pop"]

    def same(got, what, logs=True):
        for n in ref[0]:
            assert _bits(got[0][n], ref[0][n]), f"{what}: state {n}"
        if logs:
            for n in ref[1]:
                assert _bits(got[1][n], ref[1][n]), f"{what}: log {n}"
        assert _bits(got[2], ref[2]), f"{what}: scores"

    same(_evaluate(L, torch, solver, runs["C"], chunks=(7, 5)), "chunks 7 + 5")
    same(_evaluate(L, torch, solver, runs["C"], logs=False), "metrics-only", logs=False)
    same(_evaluate(L, torch, solver, runs["C"], chunks=(7, 5), logs=False), "metrics-only, chunks 7 + 5", logs=False)
    same(_evaluate(L, torch, solver, runs["C"], host=True), "host entry")
    same(_evaluate(L, torch, solver, runs["C"], chunks=(7, 5), logs=False, host=True), "host entry, metrics-only, 7 + 5",
         logs=False)
    # scores == NULL: the same run, no score launch
    got = _evaluate(L, torch, solver, runs["C"], scores=False)
    assert got[2] is None and _bits(got[0]["metrics"], ref[0]["metrics"])


def test_scores(L, torch, solver, runs):
    from dart_mpc import harness
    st, _, sc = runs["pop"]
    want = harness.population_scores(st["metrics"].reshape(P, B, 8))
    assert not np.isnan(sc).any() and _bits(sc, want), (sc, want)
    assert np.all(sc[:, 6] > 0)                 # iterations per solve
    rng = np.random.default_rng(5)
    M = rng.uniform(0.0, 1.0, (3, 5, 8))
    M[:, :, 1] = np.where(rng.uniform(size=(3, 5)) < 0.5, -1.0, rng.integers(0, 50, (3, 5)))
    M[1, :, 1] = -1.0                           # a learner with no converged instance
    M[:, :, 4:6] = rng.integers(0, 40, (3, 5, 2)); M[:, :, 7] = rng.integers(1, 20, (3, 5))
    M[2, :, 7] = 0.0                            # ... and one with no step taken
    got = L.LmpcSolver.eval_scores(M)
    want = harness.population_scores(M)
    assert want[1, 2] == -1.0 and want[2, 6] == 0.0
    assert _bits(got, want), (got, want)
    # device pointers
    d = _to_dev(torch, dict(m=M, s=np.full((3, 8), np.nan)))
    assert L.lib().dart_lmpc_eval_scores_dev(3, 5, d["m"].data_ptr(), d["s"].data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert _bits(d["s"].cpu().numpy(), want)


def test_no_policy(L, torch, solver):
    C = _case(L, with_policy=False, learners=2)
    st, lg, sc = _evaluate(L, torch, solver, C)
    _same_run((st, lg), _rollout(L, torch, solver, C), "no policy, P = 2")
    from dart_mpc import harness
    assert _bits(sc, harness.population_scores(st["metrics"].reshape(2, B, 8)))


def test_evaluate_population_front_end(L, torch, solver):
    """ppo.evaluate_population on a population_stack dict: the latest weights and the best-policy snapshots (here the
    other member's weights), against evaluate_dev on the same arrays; the population is not advanced."""
    from dart_mpc import ppo
    C = _case(L, seeds=(0, 1), learners=2, rows=(0, 0))
    members = []
    for l, p in enumerate(C["policies"]):
        snap = np.concatenate([C["weights"][1 - l], np.zeros(L.CRITIC_NWEIGHTS, np.float32)])
        members.append(dict(target=C["target"][:B], plant_pvec=C["pvec"][:B], state=solver.loop_state(C["x0"][:B], policy=p),
                            cstate={}, adam=np.zeros((2, L.PPO_NPARAMS), np.float32), adam_step=np.zeros(1, np.int32),
                            best=dict(best_return=np.array([1.0]), best_weights=snap, best_iter=np.array([0], np.int32)),
                            current_k=p.current_k, weights=p.weights))
    pop = ppo.population_stack(members)
    before = {n: v.copy() for n, v in pop["state"].items()}
    for which, weights in (("latest", C["weights"]), ("best", C["weights"][::-1].copy())):
        ref = _evaluate(L, torch, solver, dict(C, weights=weights), logs=False)
        res = ppo.evaluate_population(solver, pop, C["x0"][:B], C["target"][:B], C["pvec"][:B], K, which=which,
                                      pcfg=C["policies"][0].cfg, noise=C["noise"])
        assert _bits(res["scores"], ref[2]) and _bits(res["metrics"], ref[0]["metrics"].reshape(2, B, 8)), which
        assert res["best"] == int(np.argmin(ref[2][:, 0]))
    assert all(_bits(pop["state"][n], before[n]) for n in before)
    pop["best"]["best_iter"][1] = -1
    with pytest.raises(L.DartMPCError):
        ppo.evaluate_population(solver, pop, C["x0"][:B], C["target"][:B], C["pvec"][:B], K, which="best")


def test_evaluate_lmpc_front_end(L):
    """harness.evaluate_lmpc (its own handle, the host entry): the metrics of learner 1 are those that
    compare_controllers' LMPC leg forms in Python from rollout_lmpc's logs, and the logging mode changes nothing."""
    from dart_mpc import harness
    from dart_mpc.lmpc import LmpcPolicy
    C = _case(L, learners=1)
    a = (C["x0"], C["target"], C["pvec"], K)
    pols = [LmpcPolicy(B, seed=s) for s in (0, 1)]
    out = harness.evaluate_lmpc(*a, pols, N=N)
    full = harness.evaluate_lmpc(*a, pols, N=N, metrics_only=False)
    assert _bits(out["metrics"], full["metrics"]) and _bits(out["scores"], full["scores"])
    assert _bits(out["scores"], harness.population_scores(out["metrics"]))
    logs, st, X = harness.rollout_lmpc(*a, N=N, policy_seed=1, return_logs=True)
    U = np.stack([lg["u_cmd"] for lg in logs], axis=1)
    _assert_metrics(out["metrics"][1], harness.rollout_metrics(X["X"], C["target"], U, st, X["iters"], X["X"][:, :, 4:], TS),
                    "evaluate_lmpc against the LMPC leg of compare_controllers")
    for b in range(B):
        assert _bits(full["logs"][1][b]["pos_error"], logs[b]["pos_error"]) and _bits(full["logs"][1][b]["state"], logs[b]["state"])
    assert _bits(full["status"][1], st)
    assert all(np.all(p.timestep == 0) for p in pols)


# ------------------------------------------------------------------------------------------------------------------
# Test 7: refusals
def test_refusals_leave_everything_untouched(L, torch, solver):
    C = _case(L)
    NI = P * B
    c = _to_dev(torch, dict(target=C["target"], prm=C["prm"], pvec=C["pvec"]))
    pol, keep = _policy_args(torch, C)
    st = {n: (np.full_like(v, np.nan) if v.dtype.kind == "f" else np.full_like(v, L.LOG_INT_FILL))
          for n, v in _fresh_state(L, solver, C).items()}
    lg = L.loop_logs(L.LMPC_LOOP_LOGS, K, NI)
    ds, dl, dsc = _to_dev(torch, st), _to_dev(torch, lg), _to_dev(torch, dict(s=np.full((P, 8), np.nan)))["s"]

    def refused(message, P_=P, B_=B, k0=0, steps=K, rows=K, state=None, logs="all", **over):
        sp = dict(_ptrs(ds), **(state or {}))
        lp = _ptrs(dl) if logs == "all" else logs
        kw = dict(pol, **over)
        with pytest.raises(L.DartMPCError) as e:
            solver.evaluate_dev(P_, B_, k0, steps, rows, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(),
                                sp, lp, scores=dsc.data_ptr(), **kw)
        assert "(-1)" in str(e.value) and message in str(e.value), str(e.value)

    refused("1 <= P <= DART_LMPC_POP_MAX", P_=0)
    refused("1 <= P <= DART_LMPC_POP_MAX", P_=L.POP_MAX + 1, B_=1)
    refused("P * B larger than B_max", B_=12)
    refused("negative batch, step or row count", B_=-1)
    refused("negative batch, step or row count", steps=-1)
    refused("negative batch, step or row count", k0=-1)
    refused("k0 + steps exceeds log_rows", k0=1)
    refused("k0 + steps exceeds log_rows", logs=None, rows=K - 1)           # metrics-only: log_rows bounds the noise rows
    refused("null and non-null log pointers", logs=dict(_ptrs(dl), pvec=0))
    refused("null metrics", state=dict(metrics=0))
    refused("null pointer", state=dict(tilt=0))
    refused("null pointer (policy state)", state=dict(history=0))
    torch.cuda.synchronize()
    for got, want in ((ds, st), (dl, lg)):
        h = _host(got)
        for n in want:
            assert _bits(h[n], want[n]), n
    assert np.isnan(dsc.cpu().numpy()).all()
    # the loop step's own
    io = _to_dev(torch, {n: (np.full((NI, w) if w else (NI,), np.nan) if dt is np.float64 else np.full(NI, L.LOG_INT_FILL, np.int32))
                         for n, w, dt in L.LMPC_LOOP_IO})
    for message, sp, lp in (("null metrics", dict(_ptrs(ds), metrics=0), _ptrs(dl)),
                            ("null and non-null log pointers", _ptrs(ds), dict(_ptrs(dl), X=0)),
                            ("null pointer", dict(_ptrs(ds), x=0), None)):
        with pytest.raises(L.DartMPCError) as e:
            solver.eval_loop_step_dev(NI, 0, 1, 1, K, c["target"].data_ptr(), c["pvec"].data_ptr(), sp, _ptrs(io), lp)
        assert "(-1)" in str(e.value) and message in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert all(_bits(_host(ds)[n], st[n]) for n in st)
    # the score entries
    assert L.lib().dart_lmpc_eval_scores_dev(0, 3, ds["metrics"].data_ptr(), dsc.data_ptr(), None) == -1
    assert L.lib().dart_lmpc_eval_scores_dev(2, 0, ds["metrics"].data_ptr(), dsc.data_ptr(), None) == -1
    assert L.lib().dart_lmpc_eval_scores_dev(2, 3, None, dsc.data_ptr(), None) == -1
    assert np.isnan(dsc.cpu().numpy()).all()
