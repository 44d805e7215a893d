"""Whole PPO training iterations of the LMPC policy on the device (csrc/lmpc_train.hip: philox_kernel,
lmpc_noise_kernel, lmpc_perm_kernel, lmpc_mean_update_kernel, lmpc_train_log_kernel; dart_lmpc_noise / _perms /
_mean_param_update / _train and their _dev forms).

The generator is pinned by the known answers of Philox4x32-10 and by harness.philox4x32_10, the numpy statement;
the noise is held to max(4 e32, 64 * 2^-24) * max(1, |z|) against the same formula in fp64 from the same words, e32
being the error of the numpy fp32 statement; the training entry is held bit for bit to the test's own sequence of
the public _dev entries, and its log rows to numpy sums (counts exact, means within 1e-9 of the mean |term|).
Every test prints its figures before it asserts (pytest -s).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = 64 * 2.0 ** -24
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
SEEDS = (0, 7, 2 ** 40 + 3)
B, NH, EVERY, MB, EPOCHS, SEED = 5, 10, 2, 16, 2, 11
HYPER = dict(clip_eps=0.2, vf_coef=0.25, ent_coef=0.01)


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _to_dev(torch, d):
    return {k: _dev(torch, v) for k, v in d.items()}


def _ptrs(d):
    return {k: v.data_ptr() for k, v in d.items()}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------
# Test 1: the generator's words
def test_philox_known_answers_and_keys(L, torch):
    from dart_mpc import harness
    inp = np.array([list(c) + list(k) for c, k, _ in KAT], np.uint32)
    want = np.array([w for _, _, w in KAT], np.uint32)
    assert np.array_equal(harness.philox4x32_10(inp[:, :4].T, inp[:, 4:].T), want)     # the numpy statement itself
    d_in, d_out = _dev(torch, inp), torch.zeros(3, 4, dtype=torch.int32, device="cuda")
    L.philox_dev(3, d_in.data_ptr(), d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    print("philox known answers:", [" ".join("%08x" % v for v in row) for row in got])
    assert np.array_equal(got, want)
    n, epochs = 67, 3
    for seed in SEEDS:
        for it in (0, 3):
            perm = torch.zeros(epochs, n, dtype=torch.int32, device="cuda")
            keys = torch.zeros(epochs, n, dtype=torch.int32, device="cuda")
            L.perms_dev(seed, it, epochs, n, perm.data_ptr(), key_out=keys.data_ptr(),
                        stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ref = np.stack([harness.lmpc_train_words(seed, it, 1, e, n) for e in range(epochs)])
            assert np.array_equal(keys.cpu().numpy().view(np.uint32), ref), (seed, it)
    # the high key word, the iteration and the epoch all enter
    base = harness.lmpc_train_words(3, 0, 1, 0, 8)
    for other in (harness.lmpc_train_words(2 ** 40 + 3, 0, 1, 0, 8), harness.lmpc_train_words(3, 1, 1, 0, 8),
                  harness.lmpc_train_words(3, 0, 1, 1, 8), harness.lmpc_train_words(3, 0, 0, 0, 8)):
        assert not np.array_equal(base, other)


# ------------------------------------------------------------------------------------------------------------------
# Test 2: permutations
@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 67, 257, 2304])
def test_permutations_are_the_lexsort_of_the_keys(L, torch, n, epochs):
    from dart_mpc import harness
    seed, it = 7, 2
    ref, keys = harness.lmpc_train_perms(seed, it, epochs, n)
    for k in keys:
        assert np.array_equal(np.lexsort((np.arange(n), k)), np.argsort(k, kind="stable"))
    guard = torch.full((epochs * n + 4,), -7, dtype=torch.int32, device="cuda")
    L.perms_dev(seed, it, epochs, n, guard.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    assert (got[epochs * n:] == -7).all()                  # nothing past the end
    got = got[:epochs * n].reshape(epochs, n)
    assert np.array_equal(got, ref)
    assert all(np.array_equal(np.sort(r), np.arange(n)) for r in got)
    host, hkeys = L.perms(seed, it, epochs, n, want_keys=True)
    assert np.array_equal(host, ref) and np.array_equal(hkeys, keys)


def test_permutation_of_five(L):
    """seed 7, iteration 0, epoch 0, n = 5 is [1, 3, 2, 0, 4]; the device entry agrees."""
    assert L.perms(7, 0, 1, 5).tolist() == [[1, 3, 2, 0, 4]]


# ------------------------------------------------------------------------------------------------------------------
# Test 3: noise
@pytest.mark.parametrize("steps,nb", [(1, 1), (3, 5), (32, 18)])
def test_noise_matches_the_formula(L, torch, steps, nb):
    from dart_mpc import harness
    seed, it = 7, 1
    z64 = harness.lmpc_train_noise(seed, it, steps, nb, np.float64)
    z32 = harness.lmpc_train_noise(seed, it, steps, nb, np.float32)
    scale = np.maximum(1.0, np.abs(z64))
    e32 = float(np.max(np.abs(z32.astype(np.float64) - z64) / scale))
    out = torch.full((steps * nb * 34 + 5,), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L.noise_dev(seed, it, steps, nb, out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[steps * nb * 34:]).all()           # nothing past the end (a tail of 2 at (1, 1))
    got = got[:steps * nb * 34].reshape(steps, nb, 34)
    err = float(np.max(np.abs(got.astype(np.float64) - z64) / scale))
    bar = max(4 * e32, FLOOR)
    print(f"noise ({steps}, {nb}): kernel error {err:.3e}, e32 {e32:.3e}, bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar
    # bit for bit: two calls, another iteration, the host twin
    again = torch.empty(steps * nb * 34, dtype=torch.float32, device="cuda")
    other = torch.empty_like(again)
    L.noise_dev(seed, it, steps, nb, again.data_ptr(), stream=s)
    L.noise_dev(seed, it + 1, steps, nb, other.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert _same(again.cpu().numpy().reshape(got.shape), got)
    assert not np.array_equal(other.cpu().numpy().reshape(got.shape), got)
    assert _same(L.noise(seed, it, steps, nb), got)
    if (steps, nb) == (32, 18):
        n = got.size
        mean, var = float(got.astype(np.float64).mean()), float(got.astype(np.float64).var())
        print(f"moments: mean {mean:.4f} (bar {5 / np.sqrt(n):.4f}), var - 1 {var - 1:.4f} (bar {5 * np.sqrt(2 / n):.4f})")
        assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)


# ------------------------------------------------------------------------------------------------------------------
# shared setup of tests 4 - 6
@functools.lru_cache(maxsize=None)
def _nets():
    import torch
    from dart_mpc import ppo
    torch.manual_seed(0)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return ppo.pack_weights(net)


def _inputs(L, K, ep_steps=12):
    """B = 5 controllers, N = 10, records every 2nd step, episodes of 12 steps (so that episodes end in every
    iteration), a reset pool of 2 rows."""
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    actor, critic = _nets()
    pol = LmpcPolicy(B, weights=actor.copy(), critic_weights=critic.copy())
    n = D["state"].shape[0]
    idx = (np.arange(2)[:, None] * 7 + np.arange(B)[None] + B) % n
    pool = dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx])
    rcfg = L.reward_config(record_every=EVERY, max_episode_steps=ep_steps)
    return dict(D=D, policy=pol, pool=pool, rcfg=rcfg, K=K, R=K // EVERY,
                cfg=L.ppo_config(epochs=EPOCHS, mini_batch_size=MB, **HYPER))


class _Run:
    """Device arrays of one training run."""

    def __init__(self, L, torch, s, I, iterations):
        K, R, D, pol = I["K"], I["R"], I["D"], I["policy"]
        n = R * B
        self.c = _to_dev(torch, dict(target=D["target"][:B], prm=np.tile(L.LMPC_PRM_DEFAULT, (B, 1)),
                                     pvec=D["pvec"][:B], current_k=pol.current_k, weights=pol.weights,
                                     critic=pol.critic_weights))
        self.st = _to_dev(torch, s.loop_state(D["state"][:B], policy=pol))
        self.cs = _to_dev(torch, L.LmpcSolver.collect_state(np.zeros((B, 2))))
        self.lg = _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, K, B))
        self.clg = _to_dev(torch, L.loop_logs(L.LMPC_COLLECT_LOGS, K, B))
        self.rec = _to_dev(torch, L.loop_logs(L.LMPC_COLLECT_REC, R, B))
        self.pool = _to_dev(torch, I["pool"])
        self.tr = dict(adam=torch.zeros(2, 77317, dtype=torch.float32, device="cuda"),
                       adam_step=torch.zeros(1, dtype=torch.int32, device="cuda"),
                       train_log=torch.full((iterations, 12), float("nan"), dtype=torch.float64, device="cuda"),
                       best_return=torch.full((1,), float("-inf"), dtype=torch.float64, device="cuda"),
                       best_weights=torch.zeros(77317, dtype=torch.float32, device="cuda"),
                       best_iter=torch.full((1,), -1, dtype=torch.int32, device="cuda"),
                       workspace=torch.zeros(L.train_workspace_bytes(B, K, EVERY, EPOCHS, MB), dtype=torch.uint8,
                                             device="cuda"))
        self.n = n

    def train(self, L, s, I, stream, iterations, it0=0, row0=0, **over):
        tr = _ptrs(self.tr)
        tr["train_log"] += 12 * 8 * row0
        tcfg = L.train_config(**{**dict(seed=SEED, iterations=iterations, it0=it0, steps=I["K"]), **over})
        s.train_dev(B, 2, self.c["target"].data_ptr(), self.c["prm"].data_ptr(), self.c["pvec"].data_ptr(),
                    self.c["current_k"].data_ptr(), self.c["weights"].data_ptr(), self.c["critic"].data_ptr(),
                    _ptrs(self.st), _ptrs(self.cs), _ptrs(self.lg), _ptrs(self.clg), _ptrs(self.rec), tr,
                    I["policy"].cfg, I["rcfg"], I["cfg"], tcfg, pool=_ptrs(self.pool), stream=stream)

    def snapshot(self, with_train=True):
        out = {}
        groups = [("c", self.c), ("st", self.st), ("cs", self.cs), ("lg", self.lg), ("clg", self.clg), ("rec", self.rec)]
        if with_train:
            groups.append(("tr", {k: v for k, v in self.tr.items() if k != "workspace"}))
        else:
            groups.append(("tr", {k: self.tr[k] for k in ("adam", "adam_step")}))
        for g, d in groups:
            for k, v in d.items():
                out[g + "." + k] = v.cpu().numpy()
        return out


def _own_sequence(L, torch, s, I, ts, iterations):
    """The iterations issued by the test itself through the public _dev entries, with what the log rows need."""
    K, R, cfg, pol = I["K"], I["R"], I["cfg"], I["policy"]
    r = _Run(L, torch, s, I, iterations)
    n, stream = r.n, ts.cuda_stream
    noise = torch.empty(K, B, 34, dtype=torch.float32, device="cuda")
    last_value = torch.empty(B, dtype=torch.float32, device="cuda")
    adv = torch.full((R, B), float("nan"), dtype=torch.float64, device="cuda")
    ret = torch.full_like(adv, float("nan"))
    sample = _dev(torch, np.arange(n, dtype=np.int32))
    perms = torch.empty(EPOCHS, n, dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.ppo_workspace_bytes(n, MB), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    per_it = []
    for it in range(iterations):
        ep0 = r.cs["episodes"].cpu().numpy()
        with torch.cuda.stream(ts):
            r.cs["nrec"].zero_()
        L.noise_dev(SEED, it, K, B, noise.data_ptr(), stream=stream)
        s.collect_dev(B, 0, K, K, R, 2, r.c["target"].data_ptr(), r.c["prm"].data_ptr(), r.c["pvec"].data_ptr(),
                      _ptrs(r.st), _ptrs(r.cs), _ptrs(r.lg), _ptrs(r.clg), _ptrs(r.rec), pol.cfg, I["rcfg"],
                      r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.c["current_k"].data_ptr(),
                      noise=noise.data_ptr(), pool=_ptrs(r.pool), stream=stream)
        L.critic_value_dev(B, r.c["critic"].data_ptr(), r.st["history"].data_ptr(), last_value.data_ptr(), stream=stream)
        rc = L.lib().dart_lmpc_gae_dev(B, R, 0.99, 0.95, r.cs["nrec"].data_ptr(), r.rec["rec_reward"].data_ptr(),
                                       r.rec["rec_value"].data_ptr(), r.rec["rec_done"].data_ptr(),
                                       last_value.data_ptr(), adv.data_ptr(), ret.data_ptr(), stream)
        assert rc == 0
        L.perms_dev(SEED, it, EPOCHS, n, perms.data_ptr(), stream=stream)
        L.ppo_update_dev(cfg, n, n, sample.data_ptr(), perms.data_ptr(), r.rec["rec_obs"].data_ptr(),
                         r.rec["rec_action"].data_ptr(), r.rec["rec_logp"].data_ptr(), adv.data_ptr(), ret.data_ptr(),
                         r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.tr["adam"].data_ptr(),
                         r.tr["adam_step"].data_ptr(), stats.data_ptr(), ws.data_ptr(), stream=stream)
        L.mean_param_update_dev(pol.cfg, B, r.c["weights"].data_ptr(), r.st["history"].data_ptr(),
                                r.st["model_params"].data_ptr(), r.c["current_k"].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        per_it.append(dict(ep0=ep0, episodes=r.cs["episodes"].cpu().numpy(), nrec=r.cs["nrec"].cpu().numpy(),
                           last_return=r.cs["last_return"].cpu().numpy(), reward=r.clg["reward"].cpu().numpy(),
                           status=r.lg["status"].cpu().numpy(), stats=stats.cpu().numpy(),
                           weights=np.concatenate([r.c["weights"].cpu().numpy(), r.c["critic"].cpu().numpy()])))
    return r.snapshot(with_train=False), per_it


@pytest.fixture(scope="module")
def runs(L, torch):
    """K = 32 (n = 80: five mini-batches of 16) and K = 24 (n = 60: the last mini-batch has 12): the test's own
    sequence, train_dev with 2 iterations (twice at K = 32), two calls of 1 iteration, and the host entry."""
    out = {}
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    try:
        for K in (32, 24):
            I = _inputs(L, K)
            own, per_it = _own_sequence(L, torch, s, I, ts, 2)
            whole = _Run(L, torch, s, I, 2)
            torch.cuda.synchronize()
            whole.train(L, s, I, stream, 2)
            torch.cuda.synchronize()
            o = dict(I=I, own=own, per_it=per_it, whole=whole.snapshot())
            chained = _Run(L, torch, s, I, 2)
            torch.cuda.synchronize()
            chained.train(L, s, I, stream, 1, it0=0, row0=0)
            chained.train(L, s, I, stream, 1, it0=1, row0=1)
            torch.cuda.synchronize()
            o["chained"] = chained.snapshot()
            if K == 32:
                again = _Run(L, torch, s, I, 2)
                torch.cuda.synchronize()
                again.train(L, s, I, stream, 2)
                torch.cuda.synchronize()
                o["again"] = again.snapshot()
                o["host"] = _host_run(L, s, I, 2)
            out[K] = o
    finally:
        s.close()
    return out


def _host_run(L, s, I, iterations, timestep=None):
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    K, R, D = I["K"], I["R"], I["D"]
    pol = LmpcPolicy(B, weights=I["policy"].weights.copy(), critic_weights=I["policy"].critic_weights.copy())
    state = s.loop_state(D["state"][:B], policy=pol)
    if timestep is not None:
        state["timestep"][:] = timestep
    cs = L.LmpcSolver.collect_state(np.zeros((B, 2)))
    target, pvec = np.ascontiguousarray(D["target"][:B]), np.ascontiguousarray(D["pvec"][:B])
    lg, clg = L.loop_logs(L.LMPC_LOOP_LOGS, K, B), L.loop_logs(L.LMPC_COLLECT_LOGS, K, B)
    rec = L.loop_logs(L.LMPC_COLLECT_REC, R, B)
    adam, step, best = np.zeros((2, 77317), np.float32), np.zeros(1, np.int32), ppo.new_best()
    log = np.full((iterations, 12), np.nan)
    pool = {k: np.ascontiguousarray(v) for k, v in I["pool"].items()}
    s.train(target, pvec, state, cs, lg, clg, rec, pol, adam, step, log, best["best_return"], best["best_weights"],
            best["best_iter"], I["cfg"], L.train_config(seed=SEED, iterations=iterations, steps=K), rcfg=I["rcfg"],
            pool=pool)
    out = {"c.target": target, "c.pvec": pvec, "c.current_k": pol.current_k, "c.weights": pol.weights,
           "c.critic": pol.critic_weights, "tr.adam": adam, "tr.adam_step": step, "tr.train_log": log,
           "tr.best_return": best["best_return"], "tr.best_weights": best["best_weights"],
           "tr.best_iter": best["best_iter"]}
    for g, d in (("st", state), ("cs", cs), ("lg", lg), ("clg", clg), ("rec", rec)):
        for k, v in d.items():
            out[g + "." + k] = v
    return out


def _assert_same(a, b, what, skip=()):
    keys = [k for k in a if k in b and k not in skip]
    assert len(keys) >= 40, what
    bad = [k for k in keys if not _same(a[k], b[k])]
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------------------------
# Test 4: the mean-based parameter write
def test_mean_param_update(L, torch):
    from dart_mpc import harness
    I = _inputs(L, 8)
    pol = I["policy"]
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    try:
        r = _Run(L, torch, s, I, 1)
        noise = _dev(torch, harness.lmpc_noise(3, 8, B))
        act = torch.zeros(B, 34, dtype=torch.float32, device="cuda")
        mean_exp = torch.zeros(B, 34, dtype=torch.float32, device="cuda")
        mean_out = torch.zeros(B, 34, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.collect_dev(B, 0, 8, 8, 4, 2, r.c["target"].data_ptr(), r.c["prm"].data_ptr(), r.c["pvec"].data_ptr(),
                      _ptrs(r.st), _ptrs(r.cs), _ptrs(r.lg), _ptrs(r.clg), _ptrs(r.rec), pol.cfg, I["rcfg"],
                      r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.c["current_k"].data_ptr(),
                      noise=noise.data_ptr(), pool=_ptrs(r.pool))
        s.sync()
        before = {k: v.cpu().numpy() for k, v in r.st.items()}
        assert np.abs(before["history"]).max() > 0 and before["obs_count"].tolist() == [8] * B
        # the experience kernel's recomputed mean on the same weights and history (scratch copies of what it writes)
        cs2, lg2 = _to_dev(torch, _host(r.cs)), _to_dev(torch, _host(r.clg))
        rec2 = _to_dev(torch, _host(r.rec))
        st2 = _to_dev(torch, before)
        tg2, pv2 = r.c["target"].clone(), r.c["pvec"].clone()
        torch.cuda.synchronize()
        s.experience_step_dev(B, 7, 8, 4, 0, pol.cfg, I["rcfg"], r.c["weights"].data_ptr(), r.c["critic"].data_ptr(),
                              act.data_ptr(), r.lg["X"].data_ptr(), tg2.data_ptr(), pv2.data_ptr(), _ptrs(st2),
                              _ptrs(cs2), _ptrs(lg2), _ptrs(rec2), mean_out=mean_exp.data_ptr())
        s.sync()
        stream = torch.cuda.current_stream().cuda_stream
        L.mean_param_update_dev(pol.cfg, B, r.c["weights"].data_ptr(), r.st["history"].data_ptr(),
                                r.st["model_params"].data_ptr(), r.c["current_k"].data_ptr(),
                                mean_out=mean_out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        after = {k: v.cpu().numpy() for k, v in r.st.items()}
        ck = r.c["current_k"].cpu().numpy()
        assert _same(mean_out.cpu().numpy(), mean_exp.cpu().numpy())          # the policy kernel's mean, bit for bit
        ref_mean, ref_params = harness.lmpc_mean_param_update(_nets()[0], before["history"], before["model_params"],
                                                              pol.cfg)
        d = float(np.max(np.abs(after["model_params"] - ref_params)))
        moved = float(np.max(np.abs(after["model_params"] - before["model_params"])))
        print(f"mean write: max |dparams| {d:.3e} (moved {moved:.3e}), max |dmean| "
              f"{float(np.max(np.abs(mean_out.cpu().numpy() - ref_mean))):.3e}")
        assert d <= 1e-6 and moved > 1e-6
        assert _same(ck, after["model_params"])
        for k in ("history", "obs_mean", "obs_M2", "obs_count", "timestep", "x", "u_prev", "w"):
            assert _same(before[k], after[k]), k
        # the host twin
        mp, ck2 = before["model_params"].copy(), np.zeros((B, 34))
        hmean = L.mean_param_update(pol.cfg, _nets()[0], before["history"], mp, ck2)
        assert _same(hmean, mean_out.cpu().numpy()) and _same(mp, after["model_params"]) and _same(ck2, mp)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------
# Test 5: the entry is its launches
@pytest.mark.parametrize("K", [32, 24])
def test_train_entry_equals_its_launches(runs, K):
    o = runs[K]
    last = o["per_it"][-1]
    assert last["nrec"].tolist() == [K // EVERY] * B
    assert sum(int((p["episodes"] - p["ep0"]).sum()) for p in o["per_it"]) >= B     # episodes did end
    assert o["own"]["tr.adam_step"].tolist() == [2 * EPOCHS * -(-(K // EVERY * B) // MB)]
    _assert_same(o["own"], o["whole"], f"own sequence against train_dev, K = {K}")
    assert not _same(o["whole"]["c.weights"], _nets()[0])
    assert _same(o["whole"]["c.current_k"], o["whole"]["st.model_params"])
    _assert_same(o["whole"], o["chained"], f"2 iterations against 1 + 1, K = {K}")
    assert _same(o["whole"]["tr.train_log"], o["chained"]["tr.train_log"])


def test_train_entry_is_deterministic_and_host_equals_device(runs):
    o = runs[32]
    _assert_same(o["whole"], o["again"], "two runs")
    _assert_same(o["whole"], o["host"], "host entry against device entry", skip=("c.prm",))
    assert _same(o["whole"]["tr.train_log"], o["host"]["tr.train_log"])


# ------------------------------------------------------------------------------------------------------------------
# Test 6: log rows and snapshot
@pytest.mark.parametrize("K", [32, 24])
def test_log_rows_and_snapshot(runs, K):
    o = runs[K]
    log = o["whole"]["tr.train_log"]
    best, took = -np.inf, []
    for it, p in enumerate(o["per_it"]):
        row = log[it]
        d = p["episodes"] - p["ep0"]
        adv = d > 0
        lr = p["last_return"][adv]
        print(f"K = {K}, iteration {it}: row {np.array2string(row, precision=5)}")
        assert row[0] == K // EVERY * B and row[1] == d.sum() and row[9] == (p["nrec"] != K // EVERY).sum()
        assert adv.any()
        assert abs(row[2] - lr.mean()) <= 1e-9 * np.abs(lr).mean() and row[3] == lr.max()
        assert abs(row[4] - p["reward"].mean()) <= 1e-9 * np.abs(p["reward"]).mean()
        assert abs(row[5] - np.mean(p["status"] != 0)) <= 1e-9
        assert np.array_equal(row[6:9], p["stats"])
        snap = lr.max() > best
        if snap:
            best = lr.max()
            took.append(it)
        assert row[10] == best and row[11] == float(snap)
    assert took and o["whole"]["tr.best_iter"].tolist() == [took[-1]]
    assert o["whole"]["tr.best_return"].tolist() == [best]
    assert _same(o["whole"]["tr.best_weights"], o["per_it"][took[-1]]["weights"])


def test_train_entry_rejects_bad_shapes(L, torch):
    I = _inputs(L, 32)
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    try:
        r = _Run(L, torch, s, I, 1)
        torch.cuda.synchronize()
        with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
            r.train(L, s, I, torch.cuda.current_stream().cuda_stream, 1, steps=31)      # 31 % 2 != 0
        assert L.lib().dart_lmpc_train_workspace_bytes(B, 31, 2, 2, 16) == 0
        with pytest.raises(L.DartMPCError, match=r"\(-1\).*timestep"):
            _host_run(L, s, I, 1, timestep=np.array([0, 0, 1, 0, 0]))
        torch.cuda.synchronize()
        assert r.tr["adam_step"].cpu().tolist() == [0]                                  # nothing ran
        # weights or critic off by 4 bytes: refused with every other check, before the first launch (not by the
        # update, behind iteration 0's noise and collection): the state arrays, nrec and the workspaces keep
        # what they held, with and without a global buffer
        stream = torch.cuda.current_stream().cuda_stream
        m, G = L.global_rows(r.n)
        gb = {f: torch.zeros((G, w) if w else (G,), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
              for f, w, dt in L.LMPC_GLOBAL_ARRAYS}
        glog = torch.full((1, 6), float("nan"), dtype=torch.float64, device="cuda")
        gws = torch.full((L.global_workspace_bytes(r.n, EPOCHS, MB),), 0xA5, dtype=torch.uint8, device="cuda")
        g = L.global_buffer(_ptrs(gb), G, 0, global_log=glog.data_ptr(), workspace=gws.data_ptr())
        r.tr["workspace"].fill_(0xA5)
        r.cs["nrec"].fill_(-3)
        torch.cuda.synchronize()
        before = r.snapshot()
        tcfg = L.train_config(seed=SEED, iterations=1, steps=I["K"])
        for name in ("weights", "critic"):
            c = {k: v.data_ptr() + (4 if k == name else 0) for k, v in r.c.items()}
            args = (B, 2, c["target"], c["prm"], c["pvec"], c["current_k"], c["weights"], c["critic"], _ptrs(r.st),
                    _ptrs(r.cs), _ptrs(r.lg), _ptrs(r.clg), _ptrs(r.rec), _ptrs(r.tr), I["policy"].cfg, I["rcfg"],
                    I["cfg"], tcfg)
            for entry, extra in ((s.train_dev, ()), (s.train_global_dev, (g,))):
                with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                    entry(*args, *extra, pool=_ptrs(r.pool), stream=stream)
                torch.cuda.synchronize()
                after = r.snapshot()
                assert [k for k in before if not _same(before[k], after[k])] == [], (name, len(extra))
                assert bool((r.tr["workspace"] == 0xA5).all()) and bool((gws == 0xA5).all()), (name, len(extra))
                assert all(bool((v == 0).all()) for v in gb.values()) and bool(glog.isnan().all())
    finally:
        s.close()
