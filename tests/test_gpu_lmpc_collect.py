"""LMPC experience collection on the device (lmpc_experience_kernel / lmpc_gae_kernel in csrc/lmpc_experience.hip,
dart_lmpc_experience_step_dev / dart_lmpc_collect(_dev) / dart_lmpc_gae(_dev), harness.run_lmpc_collect / collect_lmpc).

Bars:
  * the recomputed actor mean against the policy kernel's action under zero noise: bit for bit (same accumulation order);
  * value and log-probability against the numpy nets: np.allclose(rtol = atol = 1e-5), the bar tests/test_gpu_policy.py
    holds the fp32 actor to;
  * reward against harness.lmpc_reward_step: 1e-9 relative on the fp64 terms plus w_change x 1e-5 x change_cost for
    the fp32 term (the wave sum and numpy's dot add 34 squares in different orders); done bits and counters equal;
  * collect against the same launches issued one by one, and a collection continued by a second call: bit for bit;
  * host loop against resident loop: ten times the bars of test_lmpc_host_loop_matches_resident_loop
    (|dU_cmd| <= 1e-8, |dX| <= 1e-9; a reset copies values, it adds no arithmetic), rewards / values /
    log-probabilities within the bars above;
  * GAE against the numpy recursion: 1e-12 relative.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from loop_harness import _host, _ptrs, _same, _to_dev

pytestmark = pytest.mark.gpu

TS = 0.002
X_LO = np.array([-0.18, -0.15, -0.13, -0.15, -0.05, -0.05, -0.05, -0.05])


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
    """One LMPC handle per (horizon, restoration) (B_max 67), shared by the tests of this module."""
    made = {}

    def get(N, restoration=True):
        if (N, restoration) not in made:
            made[(N, restoration)] = L.LmpcSolver(N=N, Ts=TS, B_max=67, restoration=restoration)
        return made[(N, restoration)]
    yield get
    for s in made.values():
        s.close()


def _biased(w, sl, rng, scale=0.1):
    w = w.copy()
    for s in sl:
        w[s] = rng.normal(0, scale, w[s].shape)
    return w


def _nets(seed):
    """Actor and critic with non-zero biases (a fresh Policy has zero ones)."""
    from dart_mpc.lmpc import init_critic_weights, init_policy_weights
    rng = np.random.default_rng(seed)
    o1, o2 = 520 * 64, 520 * 64 + 64 + 64 * 64
    actor = _biased(init_policy_weights(0), (slice(o1, o1 + 64), slice(o2, o2 + 64), slice(39680, 39714)), rng)
    critic = _biased(init_critic_weights(1), (slice(o1, o1 + 64), slice(o2, o2 + 64), slice(37568, 37569)), rng)
    return actor, critic


# ------------------------------------------------------------------------------------------------------------------
# Test 1: one experience launch against numpy
CASES = {"norec": dict(timestep=4, rec_rows=4, reset_rows=2, full=False),
         "record": dict(timestep=9, rec_rows=4, reset_rows=2, full=False),
         "full": dict(timestep=17, rec_rows=3, reset_rows=2, full=True),
         "reset0": dict(timestep=9, rec_rows=4, reset_rows=0, full=False)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("B", [1, 5, 67])
def test_experience_step_matches_numpy(L, torch, solvers, B, case):
    """Measured on one MI355X over the twelve cases: mean_out equal bit for bit in all of them; max |dvalue| = 2.4e-07,
    max |dlogp| = 9.8e-04 (on log-probabilities of magnitude 1e3: the odd instances draw raw with sigma 2), max
    |dreward| = 1.5e-11 (the fp32 change_cost term; the fp64 terms agree to the last bits at B = 1)."""
    from dart_mpc import harness
    from dart_mpc.lmpc import LmpcPolicy
    C = CASES[case]
    rng = np.random.default_rng(900 + 7 * B + len(case))
    actor, critic = _nets(3)
    PADB, rows, k = B + 2, 3, 1                 # two instances past the batch, one log row either side of k
    rcfg = L.reward_config(max_episode_steps=6, max_per_dim_rms=0.02)
    # obs_k: the history three policy steps leave behind; under zero noise their action is the mean
    pol = LmpcPolicy(B, weights=actor)
    target = np.zeros((PADB, 8)); target[:, [0, 2]] = rng.uniform(-0.15, 0.15, (PADB, 2))
    for _ in range(3):
        act0 = pol.step(rng.uniform(X_LO, -X_LO, (B, 8)), target[:B], rng.uniform(-0.4, 0.4, (B, 2)),
                        noise=np.zeros((B, 34), np.float32))
    obs = pol.history.reshape(B, 520).copy()
    xk = rng.uniform(X_LO, -X_LO, (B, 8))
    xk[0::3, 0] = 0.21                                                         # out of bounds
    ok = np.arange(B) % 3 == 1
    xk[ok] = target[:B][ok]; xk[ok, 1] = 1e-3                                  # success bonus
    scale = np.where(np.arange(B) % 2 == 0, 0.5, 2.0)[:, None]                 # rms of delta_z 0.01 / 0.04: damping on odd b
    raw = (rng.standard_normal((B, 34)) * scale).astype(np.float32)
    nan = lambda *s: np.full(s, np.nan)
    state = dict(history=np.full((PADB, 520), np.nan, np.float32), timestep=np.full(PADB, C["timestep"], np.int32),
                 u_prev=rng.uniform(-0.4, 0.4, (PADB, 2)), x=rng.uniform(X_LO, -X_LO, (PADB, 8)),
                 tilt=rng.uniform(-0.3, 0.3, (PADB, 2)))
    state["history"][:B] = obs
    action = np.full((PADB, 34), np.nan, np.float32); action[:B] = raw
    log_X = nan(rows, B, 8); log_X[k] = xk
    pvec = rng.uniform(0.01, 1.9, (PADB, 34))
    solve_state = rng.uniform(X_LO, -X_LO, (PADB, 8))
    cs = L.LmpcSolver.collect_state(rng.uniform(-0.4, 0.4, (PADB, 2)))
    cs["control_seen"][:] = rng.uniform(-0.4, 0.4, (PADB, 2))
    cs["ep_step"][:] = rng.integers(0, 6, PADB); cs["ep_step"][:B][1::3] = 5   # step 6 >= max_episode_steps
    cs["ep_return"][:] = rng.normal(0, 30, PADB); cs["time_penalty"][:] = rng.uniform(0, 1e-3, PADB)
    cs["episodes"][:] = rng.integers(0, 4, PADB)
    cs["last_return"][:] = rng.normal(0, 30, PADB); cs["last_steps"][:] = rng.integers(0, 9, PADB)
    cs["nrec"][:] = C["rec_rows"] if C["full"] else rng.integers(0, C["rec_rows"], PADB)
    cs["sticky"][:] = rng.integers(0, 2, PADB)
    R = max(C["reset_rows"], 1)
    pool = dict(reset_x=rng.uniform(X_LO, -X_LO, (R, B, 8)), reset_target=rng.uniform(-0.1, 0.1, (R, B, 8)),
                reset_pvec=rng.uniform(0.01, 1.9, (R, B, 34)))
    logs = L.loop_logs(L.LMPC_COLLECT_LOGS, rows, B)
    rec = L.loop_logs(L.LMPC_COLLECT_REC, C["rec_rows"] + 1, B)                # one row past rec_rows
    mean_out = np.full((PADB, 34), np.nan, np.float32)

    d_state, d_cs, d_logs, d_rec, d_pool = (_to_dev(torch, d) for d in (state, cs, logs, rec, pool))
    d = _to_dev(torch, dict(actor=actor, critic=critic, action=action, log_X=log_X, target=target, pvec=pvec,
                            solve_state=solve_state, mean_out=mean_out))
    s = solvers(20)
    s.experience_step_dev(B, k, rows, C["rec_rows"], C["reset_rows"], pol.cfg, rcfg, d["actor"].data_ptr(),
                          d["critic"].data_ptr(), d["action"].data_ptr(), d["log_X"].data_ptr(), d["target"].data_ptr(),
                          d["pvec"].data_ptr(), _ptrs(d_state), _ptrs(d_cs), _ptrs(d_logs), _ptrs(d_rec),
                          pool=_ptrs(d_pool) if C["reset_rows"] else None, solve_state=d["solve_state"].data_ptr(),
                          mean_out=d["mean_out"].data_ptr())
    s.sync()
    g_state, g_cs, g_logs, g_rec, g = _host(d_state), _host(d_cs), _host(d_logs), _host(d_rec), _host(d)

    # the same-order claim
    assert np.array_equal(g["mean_out"][:B].view(np.int32), act0.view(np.int32))
    assert np.isnan(g["mean_out"][B:]).all()
    # numpy: nets, log-probability, reward
    mean, log_std = harness.lmpc_actor_mean(actor, obs)
    value = harness.lmpc_critic_value(critic, obs)
    logp = harness.lmpc_log_prob(mean, log_std, raw, pol.cfg.log_std_min, pol.cfg.log_std_max)
    ecs = {n: v[:B].copy() for n, v in cs.items()}
    control = ecs["control_seen"].copy()
    reward, done = harness.lmpc_reward_step(rcfg, ecs, xk, target[:B], control, raw, pol.cfg.max_delta, pol.cfg.action_scale)
    change = harness.lmpc_change_cost(raw, pol.cfg.max_delta, pol.cfg.action_scale, rcfg.max_per_dim_rms)
    ecs["control_seen"] = state["u_prev"][:B].copy()
    assert (done & 1).any() and ((done & 2).any() or B == 1) and (change > 0.9 * 0.02 * np.sqrt(34)).any() == (B > 1)
    assert np.allclose(g_logs["value"][k], value, rtol=1e-5, atol=1e-5)
    assert np.allclose(g_logs["logp"][k], logp, rtol=1e-5, atol=1e-5)
    tol = 1e-9 * np.maximum(1.0, np.abs(reward)) + rcfg.w_change * 1e-5 * change
    assert np.all(np.abs(g_logs["reward"][k] - reward) <= tol), np.max(np.abs(g_logs["reward"][k] - reward))
    np.testing.assert_array_equal(g_logs["done"][k], done)
    print(f"experience step B={B} {case}: max|dvalue| = {np.max(np.abs(g_logs['value'][k] - value)):.3e}, "
          f"max|dlogp| = {np.max(np.abs(g_logs['logp'][k] - logp)):.3e}, "
          f"max|dreward| = {np.max(np.abs(g_logs['reward'][k] - reward)):.3e}")
    for r in (0, 2):
        assert np.isnan(g_logs["reward"][r]).all() and np.all(g_logs["done"][r] == L.LOG_INT_FILL)
        assert np.isnan(g_logs["value"][r]).all() and np.isnan(g_logs["logp"][r]).all()
    # collection state
    rec_step = (C["timestep"] - 1) % 8 == 0
    for n in ("ep_step", "episodes", "last_steps"):
        np.testing.assert_array_equal(g_cs[n][:B], ecs[n], err_msg=n)
    for n in ("prev_cmd", "control_seen"):
        np.testing.assert_array_equal(g_cs[n][:B], ecs[n], err_msg=n)
    for n in ("ep_return", "last_return", "time_penalty"):
        assert np.all(np.abs(g_cs[n][:B] - ecs[n]) <= tol + 1e-9 * np.abs(ecs[n])), n
    np.testing.assert_array_equal(g_cs["sticky"][:B], 0 if rec_step else (cs["sticky"][:B] | done))
    for n in cs:                                                               # the instances past the batch
        np.testing.assert_array_equal(g_cs[n][B:], cs[n][B:], err_msg=n)
    # records
    wrote = rec_step and not C["full"]
    np.testing.assert_array_equal(g_cs["nrec"][:B], cs["nrec"][:B] + (1 if wrote else 0))
    touched = np.zeros((C["rec_rows"] + 1, B), bool)
    if wrote:
        touched[cs["nrec"][:B], np.arange(B)] = True
        for b in range(B):
            n = int(cs["nrec"][b])
            assert np.array_equal(g_rec["rec_obs"][n, b].view(np.int32), obs[b].view(np.int32))
            assert np.array_equal(g_rec["rec_action"][n, b].view(np.int32), raw[b].view(np.int32))
            assert g_rec["rec_logp"][n, b] == g_logs["logp"][k, b] and g_rec["rec_value"][n, b] == g_logs["value"][k, b]
            assert g_rec["rec_reward"][n, b] == g_logs["reward"][k, b]
            assert g_rec["rec_done"][n, b] == float(done[b] != 0)
    for n in g_rec:
        a = g_rec[n].reshape(C["rec_rows"] + 1, B, -1)
        assert np.isnan(a[~touched]).all() and not np.isnan(a[touched]).any(), n
    # reset
    end = done != 0
    ex, et, ep, es, etilt = state["x"].copy(), target.copy(), pvec.copy(), solve_state.copy(), state["tilt"].copy()
    if C["reset_rows"]:
        for b in np.where(end)[0]:
            e = (int(ecs["episodes"][b]) - 1) % C["reset_rows"]
            ex[b] = es[b] = pool["reset_x"][e, b]
            et[b], ep[b], etilt[b] = pool["reset_target"][e, b], pool["reset_pvec"][e, b], 0.0
    np.testing.assert_array_equal(g_state["x"], ex); np.testing.assert_array_equal(g_state["tilt"], etilt)
    np.testing.assert_array_equal(g["target"], et); np.testing.assert_array_equal(g["pvec"], ep)
    np.testing.assert_array_equal(g["solve_state"], es)


# ------------------------------------------------------------------------------------------------------------------
# Tests 2, 3: collect is its launches; a second call continues it
SHAPES = [(5, 20), (67, 20), (3, 40)]       # one fused launch; the <false> + <true> pair; the two-wave build
K_STEPS, REC_ROWS = 20, 4


def _inputs(L, B, K, seed=5, **rc):
    """Instance 0 starts out of bounds (done at step 0 whatever the solver does); max_episode_steps = 6: every
    instance resets at least three times in 20 steps.  Records every 4th step: five per instance, the buffer
    (REC_ROWS = 4) fills and drops the last."""
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(5)
    actor, critic = _nets(4)
    pol = LmpcPolicy(B, weights=actor, critic_weights=critic)
    noise = np.random.default_rng(seed).standard_normal((K, B, 34)).astype(np.float32)
    x0 = D["state"][:B].copy(); x0[0, 0] = 0.21
    n = D["state"].shape[0]
    idx = (np.arange(2)[:, None] * 37 + np.arange(B)[None] + B) % n
    pool = dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx])
    rcfg = L.reward_config(**{**dict(max_episode_steps=6, record_every=4), **rc})
    return dict(x0=x0, target=D["target"][:B], pvec=D["pvec"][:B], policy=pol, noise=noise, pool=pool, rcfg=rcfg)


def _fresh(L, torch, s, I, rows):
    B = I["x0"].shape[0]
    c = _to_dev(torch, dict(target=I["target"], prm=np.tile(L.LMPC_PRM_DEFAULT, (B, 1)), pvec=I["pvec"],
                            current_k=I["policy"].current_k, weights=I["policy"].weights,
                            critic=I["policy"].critic_weights, noise=I["noise"]))
    return dict(c=c, st=_to_dev(torch, s.loop_state(I["x0"], policy=I["policy"])),
                cs=_to_dev(torch, L.LmpcSolver.collect_state(np.zeros((B, 2)))),
                lg=_to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, rows, B)),
                clg=_to_dev(torch, L.loop_logs(L.LMPC_COLLECT_LOGS, rows, B)),
                rec=_to_dev(torch, L.loop_logs(L.LMPC_COLLECT_REC, REC_ROWS, B)), pool=_to_dev(torch, I["pool"]))


def _collect(L, torch, s, I, rows, chunks):
    B = I["x0"].shape[0]
    F = _fresh(L, torch, s, I, rows)
    c, k = F["c"], 0
    for n in chunks:
        s.collect_dev(B, k, n, rows, REC_ROWS, 2, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(),
                      _ptrs(F["st"]), _ptrs(F["cs"]), _ptrs(F["lg"]), _ptrs(F["clg"]), _ptrs(F["rec"]), I["policy"].cfg,
                      I["rcfg"], c["weights"].data_ptr(), c["critic"].data_ptr(), c["current_k"].data_ptr(),
                      noise=c["noise"].data_ptr(), pool=_ptrs(F["pool"]))
        k += n
    s.sync()
    return F


def _hand_sequenced(L, torch, s, I, K):
    """The launches of a K-step collection issued one by one, the solves alternating between w and a second buffer."""
    B = I["x0"].shape[0]
    F = _fresh(L, torch, s, I, K)
    io = _to_dev(torch, {n: (np.full((B, w) if w else (B,), np.nan) if dt is np.float64
                             else np.full(B, L.LOG_INT_FILL, np.int32)) for n, w, dt in L.LMPC_LOOP_IO})
    c = F["c"]
    action = torch.full((B, 34), float("nan"), dtype=torch.float32, device="cuda")
    other = torch.full_like(F["st"]["w"], float("nan"))
    p, q = _ptrs(F["st"]), _ptrs(io)
    w_in, w_out = p["w"], other.data_ptr()
    tg, pv = c["target"].data_ptr(), c["pvec"].data_ptr()
    s.loop_step_dev(B, 0, 0, 1, K, tg, pv, p, q, _ptrs(F["lg"]))
    for k in range(K):
        s.policy_solve_batch_dev(I["policy"].cfg, B, c["weights"].data_ptr(), q["state"], p["u_prev"], tg,
                                 c["current_k"].data_ptr(), p["obs_mean"], p["obs_M2"], p["obs_count"], p["history"],
                                 p["timestep"], c["noise"].data_ptr() + 4 * 34 * B * k, p["model_params"],
                                 c["prm"].data_ptr(), q["u0"], q["f"], q["status"], q["iters"],
                                 action_out=action.data_ptr(), w_warm=w_in, w_out=w_out)
        w_in, w_out = w_out, w_in
        pre = int(k + 1 < K)
        s.loop_step_dev(B, k, 1, pre, K, tg, pv, p, q, _ptrs(F["lg"]))
        s.experience_step_dev(B, k, K, REC_ROWS, 2, I["policy"].cfg, I["rcfg"], c["weights"].data_ptr(),
                              c["critic"].data_ptr(), action.data_ptr(), F["lg"]["X"].data_ptr(), tg, pv, p, _ptrs(F["cs"]),
                              _ptrs(F["clg"]), _ptrs(F["rec"]), pool=_ptrs(F["pool"]),
                              solve_state=q["state"] if pre else 0)
    s.sync()
    if w_in != p["w"]:
        F["st"]["w"] = other
    return F


def _assert_same_collection(torch, a, b):
    for part in ("st", "cs", "lg", "clg", "rec"):
        for n in a[part]:
            assert _same(torch, a[part][n], b[part][n]), (part, n)
    for n in ("target", "pvec"):
        assert _same(torch, a["c"][n], b["c"][n]), n


def _check_collection(L, F, K, B):
    cs, clg, lg = _host(F["cs"]), _host(F["clg"]), _host(F["lg"])
    assert clg["done"][0, 0] & 1, "instance 0 starts out of bounds"
    assert np.all(cs["episodes"] >= 3) and np.all(cs["nrec"] == REC_ROWS)
    assert not np.isnan(clg["reward"]).any() and not np.isnan(lg["X"]).any() and np.all(clg["done"] != L.LOG_INT_FILL)
    assert not np.isnan(_host(F["rec"])["rec_obs"]).any()
    # a reset shows in the next logged state: it is the pool row, not the plant's successor
    pool = _host(F["pool"])
    for b in range(B):
        ends = np.where(clg["done"][:K - 1, b] != 0)[0]
        for j, k in enumerate(ends):
            np.testing.assert_array_equal(lg["X"][k + 1, b], pool["reset_x"][j % 2, b])


@pytest.mark.parametrize("B,N", SHAPES)
def test_collect_equals_hand_sequenced_launches(L, torch, solvers, B, N):
    s = solvers(N)
    I = _inputs(L, B, K_STEPS)
    F = _collect(L, torch, s, I, K_STEPS, [K_STEPS])
    _assert_same_collection(torch, F, _hand_sequenced(L, torch, s, I, K_STEPS))
    _check_collection(L, F, K_STEPS, B)


@pytest.mark.parametrize("restoration", [True, False])
@pytest.mark.parametrize("B,N", SHAPES)
def test_collect_continues_bit_for_bit(L, torch, solvers, B, N, restoration):
    """7 steps then 13 (k0 = 7) equal 20 steps: records, nrec, logs, every state array, target and plant_pvec."""
    s = solvers(N, restoration)
    I = _inputs(L, B, K_STEPS, seed=6)
    one = _collect(L, torch, s, I, K_STEPS, [K_STEPS])
    two = _collect(L, torch, s, I, K_STEPS, [7, 13])
    _assert_same_collection(torch, one, two)
    _check_collection(L, one, K_STEPS, B)


# ------------------------------------------------------------------------------------------------------------------
# Test 4: host loop against resident loop
def test_host_collect_loop_matches_resident_loop():
    """B = 4, N = 20, 50 steps, tau = 0.03, noise on, max_episode_steps = 13 (three resets per instance) and
    instance 0 starting out of bounds.  Measured on one MI355X: max |dU_cmd| = 5.551e-17, max |dX| = 1.735e-18, max
    relative |dreward| = 7.451e-12, max |dvalue| = 8.047e-07, max |dlogp| = 5.722e-05; statuses, iterations, done bits,
    nrec = 7 and the episode counters (4, 3, 3, 3) equal."""
    from dart_mpc import _lib, harness
    from dart_mpc.workload import lmpc_batch
    B, N, K = 4, 20, 50
    D = lmpc_batch(1, seed0=1)
    x0 = D["state"][:B].copy(); x0[0, 0] = 0.21
    idx = (np.arange(3)[:, None] * 11 + np.arange(B)[None] + B) % D["state"].shape[0]
    pool = dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx])
    kw = dict(N=N, policy_seed=0, critic_seed=1, noise_seed=3, plant_kw=dict(tau=0.03), reset_pool=pool,
              rcfg=_lib.reward_config(max_episode_steps=13))
    hl, hs, hx, he = harness.run_lmpc_collect(x0, D["target"][:B], D["pvec"][:B], K, **kw)
    dl, ds, dx, de = harness.collect_lmpc(x0, D["target"][:B], D["pvec"][:B], K, **kw)
    du = max(float(np.max(np.abs(a["u_cmd"] - b["u_cmd"]))) for a, b in zip(hl, dl))
    dX = max(float(np.max(np.abs(hx["X"] - dx["X"]))), float(np.max(np.abs(hx["state"]["x"] - dx["state"]["x"]))))
    dr = float(np.max(np.abs(he["reward"] - de["reward"]) / np.maximum(1.0, np.abs(he["reward"]))))
    dv, dp = float(np.max(np.abs(he["value"] - de["value"]))), float(np.max(np.abs(he["logp"] - de["logp"])))
    print(f"run_lmpc_collect vs collect_lmpc: max|dU_cmd| = {du:.3e}, max|dX| = {dX:.3e}, max rel |dreward| = {dr:.3e}, "
          f"max|dvalue| = {dv:.3e}, max|dlogp| = {dp:.3e}, episodes {de['episodes'].tolist()}, nrec {de['nrec'].tolist()}")
    assert du <= 1e-8 and dX <= 1e-9
    np.testing.assert_array_equal(hs, ds)
    np.testing.assert_array_equal(hx["iters"], dx["iters"])
    for n in ("done", "nrec", "episodes", "last_steps", "ep_step", "sticky"):
        np.testing.assert_array_equal(he[n], de[n], err_msg=n)
    assert np.all(de["episodes"] >= 3) and de["done"][0, 0] & 1 and np.all(de["nrec"] == 7)
    change_bound = 1e-3 * 1e-5 * 0.5 * np.sqrt(34)          # w_change x 1e-5 x the largest undamped change_cost
    assert np.all(np.abs(he["reward"] - de["reward"]) <= 1e-9 * np.maximum(1.0, np.abs(he["reward"])) + change_bound)
    assert np.allclose(de["value"], he["value"], rtol=1e-5, atol=1e-5)
    assert np.allclose(de["logp"], he["logp"], rtol=1e-5, atol=1e-5)
    for n in ("rec_logp", "rec_value"):
        assert np.allclose(de[n], he[n], rtol=1e-5, atol=1e-5, equal_nan=True), n
    np.testing.assert_array_equal(de["rec_done"], he["rec_done"])
    np.testing.assert_array_equal(de["target"], he["target"]); np.testing.assert_array_equal(de["plant_pvec"], he["plant_pvec"])
    assert np.max(np.abs(de["rec_obs"] - he["rec_obs"])) <= 1e-4          # fp32 normalised observations of states 1e-9 apart


# ------------------------------------------------------------------------------------------------------------------
# Test 5: done_sticky
@pytest.mark.parametrize("sticky", [0, 1])
def test_done_sticky_marks_the_record_after_an_episode_end(L, solvers, sticky):
    """max_episode_steps = 5: episodes end at steps 4, 9, 14, 19; records at steps 0, 8, 16.  No record step is an
    episode end, so the reference's records (sticky = 0) never see one; sticky = 1 marks records 1 and 2."""
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    B, K = 2, 20
    D = lmpc_batch(2)
    actor, critic = _nets(5)
    pol = LmpcPolicy(B, weights=actor, critic_weights=critic)
    s = solvers(20)
    st = s.loop_state(D["state"][:B], policy=pol)
    cs = L.LmpcSolver.collect_state(np.zeros((B, 2)))
    lg, clg = L.loop_logs(L.LMPC_LOOP_LOGS, K, B), L.loop_logs(L.LMPC_COLLECT_LOGS, K, B)
    rec = L.loop_logs(L.LMPC_COLLECT_REC, 3, B)
    tg, pv = D["target"][:B].copy(), D["pvec"][:B].copy()
    s.collect(0, K, tg, pv, st, cs, lg, clg, rec, pol, rcfg=L.reward_config(max_episode_steps=5, done_sticky=sticky))
    np.testing.assert_array_equal(np.where(clg["done"][:, 0] != 0)[0], [4, 9, 14, 19])
    np.testing.assert_array_equal(cs["nrec"], 3)
    np.testing.assert_array_equal(rec["rec_done"], np.array([[0, 0], [1, 1], [1, 1]], np.float32) * sticky)
    np.testing.assert_array_equal(rec["rec_reward"], clg["reward"][[0, 8, 16]])
    np.testing.assert_array_equal(tg, D["target"][:B])                       # reset_rows = 0: only the counters reset
    np.testing.assert_array_equal(cs["episodes"], 4)


# ------------------------------------------------------------------------------------------------------------------
# Test 6: GAE
def test_gae_matches_numpy_recursion(L, torch):
    from dart_mpc import harness
    rng = np.random.default_rng(8)
    rows, B = 6, 67
    nrec = rng.integers(0, rows + 1, B).astype(np.int32); nrec[:3] = [0, 1, rows]
    rw = rng.normal(0, 20, (rows, B))
    rv = rng.normal(0, 10, (rows, B)).astype(np.float32)
    rd = (rng.uniform(size=(rows, B)) < 0.3).astype(np.float32)
    lv = rng.normal(0, 10, B).astype(np.float32)
    assert rd.any()
    want_adv, want_ret = harness.gae_numpy(nrec, rw, rv, rd, lv, 0.99, 0.95)
    adv, ret = L.gae(nrec, rw, rv, rd, lv, 0.99, 0.95)
    d = _to_dev(torch, dict(nrec=nrec, rw=rw, rv=rv, rd=rd, lv=lv, adv=np.full((rows, B), np.nan),
                            ret=np.full((rows, B), np.nan)))
    p = _ptrs(d)
    L.set_device(0)
    rc = L.lib().dart_lmpc_gae_dev(B, rows, 0.99, 0.95, p["nrec"], p["rw"], p["rv"], p["rd"], p["lv"], p["adv"], p["ret"],
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for got_a, got_r in ((adv, ret), (d["adv"].cpu().numpy(), d["ret"].cpu().numpy())):
        for got, want in ((got_a, want_adv), (got_r, want_ret)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            m = ~np.isnan(want)
            assert np.all(np.abs(got[m] - want[m]) <= 1e-12 * np.maximum(1.0, np.abs(want[m])))
    assert np.isnan(want_adv[:, 0]).all() and not np.isnan(want_adv[:, 2]).any()


# ------------------------------------------------------------------------------------------------------------------
# Test 7: errors
def test_collect_errors_launch_nothing(L, torch, solvers):
    s = solvers(20)
    B, K = 3, 4
    I = _inputs(L, B, K)
    F = _fresh(L, torch, s, I, K)
    c = F["c"]
    parts = ("st", "cs", "lg", "clg", "rec")
    before = {p: {k: v.clone() for k, v in F[p].items()} for p in parts}
    before["c"] = {k: c[k].clone() for k in ("target", "pvec")}

    def call(solver=s, B_=B, k0=0, steps=K, rows=K, rec_rows=REC_ROWS, reset_rows=2, weights=c["weights"].data_ptr(),
             critic=c["critic"].data_ptr(), pool=_ptrs(F["pool"])):
        L.LmpcSolver.collect_dev(solver, B_, k0, steps, rows, rec_rows, reset_rows, c["target"].data_ptr(),
                                 c["prm"].data_ptr(), c["pvec"].data_ptr(), _ptrs(F["st"]), _ptrs(F["cs"]), _ptrs(F["lg"]),
                                 _ptrs(F["clg"]), _ptrs(F["rec"]), I["policy"].cfg, I["rcfg"], weights, critic,
                                 c["current_k"].data_ptr(), noise=c["noise"].data_ptr(), pool=pool)

    def raises(match, **kw):
        with pytest.raises(L.DartMPCError, match=match) as e:
            call(**kw)
        assert "failed (-1): " in str(e.value) and str(e.value).split("failed (-1): ")[1].strip()

    raises("policy", weights=0)
    raises("critic", critic=0)
    raises("16-byte aligned", weights=c["weights"].data_ptr() + 4)
    raises("negative", rec_rows=-1)
    raises("reset pool", pool=None)
    raises("log_rows", k0=2, steps=K - 1)
    pm = L.Solver(N=20, Ts=TS, B_max=4)
    try:
        raises("not an LMPC handle", solver=pm)
    finally:
        pm.close()
    call(steps=0)                               # steps = 0: OK, touches nothing
    s.sync()
    torch.cuda.synchronize()
    for p in parts:
        for k in F[p]:
            assert _same(torch, F[p][k], before[p][k]), (p, k)
    for k in before["c"]:
        assert _same(torch, c[k], before["c"][k]), k


# ------------------------------------------------------------------------------------------------------------------
# Test 8: a process that exits with the solver open (the handle-owned action buffer on the atexit path)
_CHILD = """
import numpy as np
from dart_mpc import _lib
from dart_mpc.lmpc import LmpcPolicy, init_critic_weights
from dart_mpc.workload import lmpc_batch
D = lmpc_batch(1)
s = _lib.LmpcSolver(N=20, B_max=4)
pol = LmpcPolicy(2, seed=0, critic_weights=init_critic_weights(1))
st = s.loop_state(D["state"][:2], policy=pol); cs = s.collect_state(np.zeros((2, 2)))
lg, clg = _lib.loop_logs(_lib.LMPC_LOOP_LOGS, 3, 2), _lib.loop_logs(_lib.LMPC_COLLECT_LOGS, 3, 2)
rec = _lib.loop_logs(_lib.LMPC_COLLECT_REC, 2, 2)
s.collect(0, 3, D["target"][:2].copy(), D["pvec"][:2].copy(), st, cs, lg, clg, rec, pol)
assert not np.isnan(clg["reward"]).any() and (st["timestep"] == 3).all() and (cs["nrec"] == 1).all()
print("collected", float(clg["reward"].sum()))
"""


def test_child_exits_cleanly_after_a_collect():
    from dart_mpc import _lib
    pkg_root = os.path.dirname(_lib.PKG_DIR)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg_root, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "collected" in r.stdout
