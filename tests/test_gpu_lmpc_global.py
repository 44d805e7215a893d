"""The global-buffer update of the device-resident LMPC training (rlmpc2.py:823-874; csrc/lmpc_train.hip:
lmpc_perm_kernel with a stream index and a prefix length, lmpc_gbuf_append_kernel, lmpc_gae_seq_kernel,
lmpc_global_log_kernel; dart_lmpc_choice / _global_append / _gae_seq / _train_global and their _dev forms).

The choice is held to harness.lmpc_train_choice, the record gather to numpy indexing bit for bit, the sequence GAE
to |d adv_t| <= 32 * 2^-52 * A_t against harness.gae_sequence, the sequential fp64 recursion, with A the same
recursion on |delta_t| (at most 12 levels of composition of two roundings each in one tile of 1024 rows, one more
per further tile but none for the last, whose carry is 0, and delta_t's own three), and the
training entry bit for bit to the test's own sequence of the public _dev entries.  ret is held to adv + value
evaluated in fp64 from the returned adv, bit for bit: that is the statement ret = adv + value ((adv + value) - adv
need not give value back in floating point).  Every test prints its figures before it asserts (pytest -s).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, NH, EVERY, MB, EPOCHS, SEED = 5, 10, 2, 16, 2, 11
HYPER = dict(clip_eps=0.2, vf_coef=0.25, ent_coef=0.01)
GAMMA, LAM = 0.99, 0.95
FIELDS = ("obs", "action", "logp", "value", "reward", "done")
REC = ("rec_obs", "rec_action", "rec_logp", "rec_value", "rec_reward", "rec_done")


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------
# Test 1: choice without replacement
@pytest.mark.parametrize("n,m", [(1, 1), (3, 1), (5, 1), (67, 16), (257, 64), (2304, 576)])
def test_choice_is_the_prefix_of_the_stream_2_permutation(L, torch, n, m):
    from dart_mpc import harness
    s = torch.cuda.current_stream().cuda_stream
    for seed, it in ((7, 2), (2 ** 40 + 3, 0)):
        ref = harness.lmpc_train_choice(seed, it, n, m)
        guard = torch.full((m + 4,), -7, dtype=torch.int32, device="cuda")
        L.choice_dev(seed, it, n, m, guard.data_ptr(), stream=s)
        torch.cuda.synchronize()
        got = guard.cpu().numpy()
        assert (got[m:] == -7).all()                        # nothing past m
        assert np.array_equal(got[:m], ref)
        assert len(set(got[:m].tolist())) == m and got[:m].min() >= 0 and got[:m].max() < n
        assert np.array_equal(L.choice(seed, it, n, m), ref)                  # the host entry
    # the whole permutation of stream 2 through the stream entry starts with the choice
    perm = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    L.perms_stream_dev(7, 2, 2, 1, n, perm.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(perm.cpu().numpy()[:m], harness.lmpc_train_choice(7, 2, n, m))
    assert np.array_equal(np.sort(perm.cpu().numpy()), np.arange(n))


# ------------------------------------------------------------------------------------------------------------------
# Test 2: the record gather
def _patterns(rng, shape, dt):
    """Distinct bit patterns, NaN payloads among them."""
    if dt == np.float32:
        a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        flat = a.reshape(-1)
        flat[:: max(flat.size // 7, 1)] = np.array([0x7fc12345], np.uint32).view(np.float32)[0]
        flat[1:: max(flat.size // 5, 1)] = np.array([0xffa00001], np.uint32).view(np.float32)[0]     # signalling
        return a
    a = rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64).view(np.float64)
    a.reshape(-1)[::7] = np.array([0x7ff4000000abcdef], np.uint64).view(np.float64)[0]
    return a


def test_append_gathers_records_bit_for_bit(L, torch):
    R, m, cap = 4, 5, 20
    rng = np.random.default_rng(3)
    widths = dict(zip(REC, (520, 34, 0, 0, 0, 0)))
    dts = dict(zip(REC, (np.float32, np.float32, np.float32, np.float32, np.float64, np.float32)))
    rec = {k: _patterns(rng, (R, B, widths[k]) if widths[k] else (R, B), dts[k]) for k in REC}
    guard = {f: _patterns(rng, (cap, widths[k]) if widths[k] else (cap,), dts[k]) for f, k in zip(FIELDS, REC)}
    sample = np.array([19, 0, 7, 13, 2, 5, 18, 11, 4, 9, 16, 1], np.int32)         # n = 12 of the 20 records
    stream = torch.cuda.current_stream().cuda_stream
    d_rec, d_buf, d_sample = _to_dev(torch, rec), _to_dev(torch, guard), _dev(torch, sample)
    want = {f: guard[f].copy() for f in FIELDS}
    for fill, choice in ((0, [3, 11, 0, 7, 5]), (10, [2, 2, 9, 1, 10])):
        choice = np.array(choice, np.int32)
        d_choice = _dev(torch, choice)
        g = L.global_buffer(_ptrs(d_buf), cap, fill)
        L.global_append_dev(g, m, sample.size, R * B, d_sample.data_ptr(), d_choice.data_ptr(), _ptrs(d_rec),
                            stream=stream)
        torch.cuda.synchronize()
        src = sample[choice]
        for f, k in zip(FIELDS, REC):
            flat = rec[k].reshape(R * B, -1) if widths[k] else rec[k].reshape(R * B)
            want[f][fill:fill + m] = flat[src]
            got = d_buf[f].cpu().numpy()
            assert _same(got, want[f]), (fill, f)            # the rows, and every other row's guard value
    # the host entry: the same rows from host arrays
    hbuf = {f: guard[f].copy() for f in FIELDS}
    hbuf["fill"] = 0
    L.global_append(hbuf, sample, [3, 11, 0, 7, 5], rec)
    assert hbuf["fill"] == 5
    hbuf["fill"] = 10
    L.global_append(hbuf, sample, [2, 2, 9, 1, 10], rec)
    for f in FIELDS:
        assert _same(hbuf[f], want[f]), f
    # an unaligned obs base, and a row past the capacity, before any device work
    before = {f: d_buf[f].cpu().numpy() for f in FIELDS}
    odd = dict(_ptrs(d_buf), obs=d_buf["obs"].data_ptr() + 4)
    with pytest.raises(L.DartMPCError, match=r"\(-1"):
        L.global_append_dev(L.global_buffer(odd, cap - 1, 0), m, sample.size, R * B, d_sample.data_ptr(),
                            d_choice.data_ptr(), _ptrs(d_rec), stream=stream)
    with pytest.raises(L.DartMPCError, match=r"\(-1"):
        L.global_append_dev(L.global_buffer(_ptrs(d_buf), cap, 16), m, sample.size, R * B, d_sample.data_ptr(),
                            d_choice.data_ptr(), _ptrs(d_rec), stream=stream)
    torch.cuda.synchronize()
    assert all(_same(d_buf[f].cpu().numpy(), before[f]) for f in FIELDS)


# ------------------------------------------------------------------------------------------------------------------
# Test 3: GAE over one sequence
@functools.lru_cache(maxsize=None)
def _sequence(G, done_kind):
    from dart_mpc import harness
    rng = np.random.default_rng(1000 * G + ("none", "all", "random", "last").index(done_kind))
    reward = rng.standard_normal(G) * np.where(rng.random(G) < 0.2, 10.0, 1.0)      # mixed sign
    value = rng.standard_normal(G).astype(np.float32)
    done = {"none": np.zeros(G), "all": np.ones(G), "random": (rng.random(G) < 0.1).astype(float),
            "last": np.zeros(G)}[done_kind].astype(np.float32)
    if done_kind == "last":
        done[-1] = 1.0
    last = np.array([-0.83], np.float32)
    adv, ret = harness.gae_sequence(reward, value, done, last, GAMMA, LAM)
    scale, _ = harness.gae_sequence(reward, value, done, last, GAMMA, LAM, magnitude=True)
    return reward, value, done, last, adv, ret, scale


@pytest.mark.parametrize("done_kind", ["none", "all", "random", "last"])
@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2880])
def test_sequence_gae_is_within_the_derived_bar(L, torch, G, done_kind):
    reward, value, done, last, adv_ref, ret_ref, scale = _sequence(G, done_kind)
    pad = 3
    d_rw, d_vl, d_dn, d_lv = (_dev(torch, np.concatenate([a, np.full(pad, 5.0, a.dtype)]))
                              for a in (reward, value, done, last))
    adv = torch.full((G + pad,), float("nan"), dtype=torch.float64, device="cuda")
    ret = torch.full((G + pad,), float("nan"), dtype=torch.float64, device="cuda")
    L.gae_seq_dev(G, GAMMA, LAM, d_rw.data_ptr(), d_vl.data_ptr(), d_dn.data_ptr(), d_lv.data_ptr(), adv.data_ptr(),
                  ret.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a, r = adv.cpu().numpy(), ret.cpu().numpy()
    assert np.isnan(a[G:]).all() and np.isnan(r[G:]).all()                   # rows past G untouched
    a, r = a[:G], r[:G]
    bar = 32 * 2.0 ** -52 * scale
    err = np.abs(a - adv_ref)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"sequence GAE, G = {G}, done {done_kind}: worst |d adv| / bar {ratio:.3f} (max |adv| "
          f"{float(np.abs(adv_ref).max()):.3f})")
    assert np.isfinite(a).all() and ratio <= 1.0
    assert _same(r, a + value.astype(np.float64))                            # ret = adv + value, exactly
    if done_kind == "all":
        assert _same(a, adv_ref)                                             # no chain: delta_t's own bits
    if G in (65, 2880):
        ha, hr = L.gae_seq(reward, value, done, last, GAMMA, LAM)            # the host entry
        assert _same(ha, a) and _same(hr, r)


# ------------------------------------------------------------------------------------------------------------------
# shared setup of tests 4 and 5
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
    """B = 5 controllers, N = 10, records every 2nd step, episodes of 12 steps, a reset pool of 2 rows."""
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    actor, critic = _nets()
    pol = LmpcPolicy(B, weights=actor.copy(), critic_weights=critic.copy())
    n = D["state"].shape[0]
    idx = (np.arange(2)[:, None] * 7 + np.arange(B)[None] + B) % n
    pool = dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx])
    rcfg = L.reward_config(record_every=EVERY, max_episode_steps=ep_steps)
    nn = K // EVERY * B
    m, G = L.global_rows(nn)
    return dict(D=D, policy=pol, pool=pool, rcfg=rcfg, K=K, R=K // EVERY, n=nn, m=m, G=G, period=G // m,
                cfg=L.ppo_config(epochs=EPOCHS, mini_batch_size=MB, **HYPER))


class _Run:
    """Device arrays of one training run with a global buffer."""

    def __init__(self, L, torch, s, I, iterations):
        K, R, D, pol, G = I["K"], I["R"], I["D"], I["policy"], I["G"]
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
        self.gb = {f: torch.zeros((G, w) if w else (G,), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
                   for f, w, dt in L.LMPC_GLOBAL_ARRAYS}
        self.glog = torch.full((iterations, 6), float("nan"), dtype=torch.float64, device="cuda")
        self.gws = torch.zeros(L.global_workspace_bytes(I["n"], EPOCHS, MB), dtype=torch.uint8, device="cuda")
        self.fill = 0

    def train(self, L, s, I, stream, iterations, it0=0, row0=0, use_global=True, plain=False):
        tr = _ptrs(self.tr)
        tr["train_log"] += 12 * 8 * row0
        tcfg = L.train_config(seed=SEED, iterations=iterations, it0=it0, steps=I["K"], gamma=GAMMA, lam=LAM)
        args = (B, 2, self.c["target"].data_ptr(), self.c["prm"].data_ptr(), self.c["pvec"].data_ptr(),
                self.c["current_k"].data_ptr(), self.c["weights"].data_ptr(), self.c["critic"].data_ptr(),
                _ptrs(self.st), _ptrs(self.cs), _ptrs(self.lg), _ptrs(self.clg), _ptrs(self.rec), tr,
                I["policy"].cfg, I["rcfg"], I["cfg"], tcfg)
        if plain:
            s.train_dev(*args, pool=_ptrs(self.pool), stream=stream)
            return
        g = None
        if use_global:
            g = L.global_buffer(_ptrs(self.gb), I["G"], self.fill, global_log=self.glog.data_ptr() + 6 * 8 * row0,
                                workspace=self.gws.data_ptr())
        s.train_global_dev(*args, g, pool=_ptrs(self.pool), stream=stream)
        if use_global:
            self.fill = L.global_fill_after(I["n"], self.fill, iterations)

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
        for f, v in self.gb.items():
            out["gb." + f] = v.cpu().numpy()[:self.fill]         # the rows held
        out["gb.fill"] = np.array([self.fill], np.int32)
        out["glog"] = self.glog.cpu().numpy()
        return out


def _own_sequence(L, torch, s, I, ts, iterations):
    """The iterations issued by the test itself through the public _dev entries; per iteration the weights after it
    and what the log rows are checked against."""
    K, R, cfg, pol, n, m, G = I["K"], I["R"], I["cfg"], I["policy"], I["n"], I["m"], I["G"]
    r = _Run(L, torch, s, I, iterations)
    stream = ts.cuda_stream
    noise = torch.empty(K, B, 34, dtype=torch.float32, device="cuda")
    last_value = torch.empty(B, dtype=torch.float32, device="cuda")
    adv = torch.full((R, B), float("nan"), dtype=torch.float64, device="cuda")
    ret = torch.full_like(adv, float("nan"))
    sample = _dev(torch, np.arange(n, dtype=np.int32))
    perms = torch.empty(EPOCHS, n, dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.ppo_workspace_bytes(n, MB), dtype=torch.uint8, device="cuda")
    choice = torch.empty(m, dtype=torch.int32, device="cuda")
    g_last = torch.empty(1, dtype=torch.float32, device="cuda")
    g_adv = torch.full((G,), float("nan"), dtype=torch.float64, device="cuda")
    g_ret = torch.full_like(g_adv, float("nan"))
    g_sample = _dev(torch, np.arange(G, dtype=np.int32))
    g_perms = torch.empty(EPOCHS, G, dtype=torch.int32, device="cuda")
    g_stats = torch.zeros(3, dtype=torch.float64, device="cuda")
    g_steps = EPOCHS * -(-G // MB)
    g_step_log = torch.full((g_steps, 4), float("nan"), dtype=torch.float32, device="cuda")
    g_ws = torch.zeros(L.ppo_workspace_bytes(G, MB), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    per_it, fill = [], 0
    for it in range(iterations):
        with torch.cuda.stream(ts):
            r.cs["nrec"].zero_()
        L.noise_dev(SEED, it, K, B, noise.data_ptr(), stream=stream)
        s.collect_dev(B, 0, K, K, R, 2, r.c["target"].data_ptr(), r.c["prm"].data_ptr(), r.c["pvec"].data_ptr(),
                      _ptrs(r.st), _ptrs(r.cs), _ptrs(r.lg), _ptrs(r.clg), _ptrs(r.rec), pol.cfg, I["rcfg"],
                      r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.c["current_k"].data_ptr(),
                      noise=noise.data_ptr(), pool=_ptrs(r.pool), stream=stream)
        L.critic_value_dev(B, r.c["critic"].data_ptr(), r.st["history"].data_ptr(), last_value.data_ptr(), stream=stream)
        rc = L.lib().dart_lmpc_gae_dev(B, R, GAMMA, LAM, r.cs["nrec"].data_ptr(), r.rec["rec_reward"].data_ptr(),
                                       r.rec["rec_value"].data_ptr(), r.rec["rec_done"].data_ptr(),
                                       last_value.data_ptr(), adv.data_ptr(), ret.data_ptr(), stream)
        assert rc == 0
        L.perms_dev(SEED, it, EPOCHS, n, perms.data_ptr(), stream=stream)
        L.ppo_update_dev(cfg, n, n, sample.data_ptr(), perms.data_ptr(), r.rec["rec_obs"].data_ptr(),
                         r.rec["rec_action"].data_ptr(), r.rec["rec_logp"].data_ptr(), adv.data_ptr(), ret.data_ptr(),
                         r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.tr["adam"].data_ptr(),
                         r.tr["adam_step"].data_ptr(), stats.data_ptr(), ws.data_ptr(), stream=stream)
        # 6a
        L.choice_dev(SEED, it, n, m, choice.data_ptr(), stream=stream)
        L.global_append_dev(L.global_buffer(_ptrs(r.gb), G, fill), m, n, n, sample.data_ptr(), choice.data_ptr(),
                            _ptrs(r.rec), stream=stream)
        fill += m
        row = dict(fill=fill, ran=int(fill >= n), step_log=None)
        if fill >= n:                                             # 6b
            assert fill == G
            L.critic_value_dev(1, r.c["critic"].data_ptr(), r.gb["obs"].data_ptr() + (G - 1) * 520 * 4,
                               g_last.data_ptr(), stream=stream)
            L.gae_seq_dev(G, GAMMA, LAM, r.gb["reward"].data_ptr(), r.gb["value"].data_ptr(), r.gb["done"].data_ptr(),
                          g_last.data_ptr(), g_adv.data_ptr(), g_ret.data_ptr(), stream=stream)
            L.perms_stream_dev(SEED, it, 3, EPOCHS, G, g_perms.data_ptr(), stream=stream)
            L.ppo_update_dev(cfg, G, G, g_sample.data_ptr(), g_perms.data_ptr(), r.gb["obs"].data_ptr(),
                             r.gb["action"].data_ptr(), r.gb["logp"].data_ptr(), g_adv.data_ptr(), g_ret.data_ptr(),
                             r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.tr["adam"].data_ptr(),
                             r.tr["adam_step"].data_ptr(), g_stats.data_ptr(), g_ws.data_ptr(),
                             step_log=g_step_log.data_ptr(), stream=stream)
            fill = 0
        L.mean_param_update_dev(pol.cfg, B, r.c["weights"].data_ptr(), r.st["history"].data_ptr(),
                                r.st["model_params"].data_ptr(), r.c["current_k"].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        if row["ran"]:
            row["step_log"] = g_step_log.cpu().numpy().astype(np.float64)
            row["g_stats"] = g_stats.cpu().numpy()
        row["stats"] = stats.cpu().numpy()
        row["weights"] = np.concatenate([r.c["weights"].cpu().numpy(), r.c["critic"].cpu().numpy()])
        per_it.append(row)
    r.fill = fill
    return r.snapshot(with_train=False), per_it


def _host_run(L, s, I, iterations):
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    K, R, D = I["K"], I["R"], I["D"]
    pol = LmpcPolicy(B, weights=I["policy"].weights.copy(), critic_weights=I["policy"].critic_weights.copy())
    state = s.loop_state(D["state"][:B], policy=pol)
    cs = L.LmpcSolver.collect_state(np.zeros((B, 2)))
    target, pvec = np.array(D["target"][:B]), np.array(D["pvec"][:B])         # copies: the entry updates them in place
    lg, clg = L.loop_logs(L.LMPC_LOOP_LOGS, K, B), L.loop_logs(L.LMPC_COLLECT_LOGS, K, B)
    rec = L.loop_logs(L.LMPC_COLLECT_REC, R, B)
    adam, step, best = np.zeros((2, 77317), np.float32), np.zeros(1, np.int32), ppo.new_best()
    log, glog = np.full((iterations, 12), np.nan), np.full((iterations, 6), np.nan)
    pool = {k: np.ascontiguousarray(v) for k, v in I["pool"].items()}
    gbuf = ppo.new_global_buffer(I["n"])
    for f in FIELDS:
        gbuf[f][...] = 7                                           # rows not held at the end keep the caller's values
    s.train(target, pvec, state, cs, lg, clg, rec, pol, adam, step, log, best["best_return"], best["best_weights"],
            best["best_iter"], I["cfg"], L.train_config(seed=SEED, iterations=iterations, steps=K, gamma=GAMMA, lam=LAM),
            rcfg=I["rcfg"], pool=pool, global_buffer=gbuf, global_log=glog)
    out = {"c.target": target, "c.pvec": pvec, "c.current_k": pol.current_k, "c.weights": pol.weights,
           "c.critic": pol.critic_weights, "tr.adam": adam, "tr.adam_step": step, "tr.train_log": log,
           "tr.best_return": best["best_return"], "tr.best_weights": best["best_weights"],
           "tr.best_iter": best["best_iter"], "glog": glog, "gb.fill": np.array([gbuf["fill"]], np.int32)}
    for g, d in (("st", state), ("cs", cs), ("lg", lg), ("clg", clg), ("rec", rec)):
        for k, v in d.items():
            out[g + "." + k] = v
    for f in FIELDS:
        out["gb." + f] = gbuf[f][:gbuf["fill"]]
        assert (gbuf[f][gbuf["fill"]:] == 7).all(), f
    return out


@pytest.fixture(scope="module")
def runs(L, torch):
    """K = 32 (n = 80, period 4), K = 24 (n = 60, the last mini-batch of the local update has 12) and K = 36 (n = 90,
    m = 22, G = 110 > n, period 5), period + 1 iterations each: the test's own sequence, the entry in one call, twice,
    split inside the fill period and right after the update, the host entry, and the entries without the buffer."""
    out = {}
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    try:
        for K in (32, 24, 36):
            I = _inputs(L, K)
            its = I["period"] + 1
            own, per_it = _own_sequence(L, torch, s, I, ts, its)
            o = dict(I=I, own=own, per_it=per_it, its=its)

            def run(parts, **kw):
                r = _Run(L, torch, s, I, its)
                torch.cuda.synchronize()
                done = 0
                for k in parts:
                    r.train(L, s, I, stream, k, it0=done, row0=done, **kw)
                    done += k
                torch.cuda.synchronize()
                return r.snapshot()

            o["whole"] = run([its])
            o["again"] = run([its])
            o["split_inside"] = run([2, its - 2])
            o["split_after"] = run([I["period"], 1])
            o["host"] = _host_run(L, s, I, its)
            # without the buffer, iteration by iteration: the weights after every iteration
            r = _Run(L, torch, s, I, its)
            torch.cuda.synchronize()
            o["plain_weights"] = []
            for it in range(its):
                r.train(L, s, I, stream, 1, it0=it, row0=it, plain=True)
                torch.cuda.synchronize()
                o["plain_weights"].append(np.concatenate([r.c["weights"].cpu().numpy(), r.c["critic"].cpu().numpy()]))
            o["plain"] = r.snapshot()
            if K == 32:
                o["null"] = run([2, its - 2], use_global=False)
            out[K] = o
    finally:
        s.close()
    return out


def _assert_same(a, b, what, skip=()):
    keys = [k for k in a if k in b and k not in skip]
    assert len(keys) >= 40, what
    bad = [k for k in keys if not _same(a[k], b[k])]
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------------------------
# Test 4: the iteration with the global update
@pytest.mark.parametrize("K", [32, 24, 36])
def test_train_global_entry_equals_its_launches(runs, K):
    o = runs[K]
    I, its, per_it = o["I"], o["its"], o["per_it"]
    n, m, G, period = I["n"], I["m"], I["G"], I["period"]
    assert [p["ran"] for p in per_it] == [0] * (period - 1) + [1, 0]           # one update, then the refill starts
    _assert_same(o["own"], o["whole"], f"own sequence against train_global_dev, K = {K}", skip=("glog",))
    assert o["whole"]["gb.fill"].tolist() == [m] and o["whole"]["gb.obs"].shape == (m, 520)
    assert np.abs(o["whole"]["gb.obs"]).max() > 0
    glog, tlog = o["whole"]["glog"], o["whole"]["tr.train_log"]
    for it, p in enumerate(per_it):
        print(f"K = {K}, iteration {it}: global row {np.array2string(glog[it], precision=5)}")
        assert glog[it, :3].tolist() == [p["fill"], p["ran"], G]
        assert np.array_equal(tlog[it, 6:9], p["stats"])                      # the local update's means, as before
        if p["ran"]:
            steps = EPOCHS * -(-G // MB)
            assert p["step_log"].shape == (steps, 4) and np.isfinite(p["step_log"]).all()
            for c in range(3):
                col = p["step_log"][:, c]
                assert abs(glog[it, 3 + c] - col.sum() / steps) <= 1e-9 * np.abs(col).mean(), (it, c)
            assert np.array_equal(glog[it, 3:], p["g_stats"])
        else:
            assert np.isnan(glog[it, 3:]).all()
    # Adam's step count runs on through both updates
    want_steps = its * EPOCHS * -(-n // MB) + 1 * EPOCHS * -(-G // MB)
    assert o["whole"]["tr.adam_step"].tolist() == [want_steps]
    # the snapshot takes the weights after both updates
    bi = int(o["whole"]["tr.best_iter"][0])
    assert 0 <= bi < its and _same(o["whole"]["tr.best_weights"], per_it[bi]["weights"])
    # against the run without the buffer: the same weights up to the update iteration, other weights from it on
    for it in range(its):
        same = _same(per_it[it]["weights"], o["plain_weights"][it])
        assert same == (it < period - 1), it
    assert o["plain"]["tr.adam_step"].tolist() == [its * EPOCHS * -(-n // MB)]


@pytest.mark.parametrize("K", [32, 24, 36])
def test_train_global_chains_repeats_and_host_equals_device(runs, K):
    o = runs[K]
    for other in ("again", "split_inside", "split_after"):
        _assert_same(o["whole"], o[other], f"{other}, K = {K}")
        assert _same(o["whole"]["glog"], o[other]["glog"]) and _same(o["whole"]["tr.train_log"], o[other]["tr.train_log"])
    _assert_same(o["whole"], o["host"], f"host entry against device entry, K = {K}", skip=("c.prm",))
    assert _same(o["whole"]["glog"], o["host"]["glog"]) and _same(o["whole"]["tr.train_log"], o["host"]["tr.train_log"])
    for f in FIELDS:
        assert _same(o["whole"]["gb." + f], o["host"]["gb." + f]), f


def test_null_buffer_is_the_old_entry(runs):
    o = runs[32]
    skip = tuple(k for k in o["null"] if k.startswith("gb.")) + ("glog",)
    _assert_same(o["plain"], o["null"], "train_global_dev(g = NULL) against train_dev", skip=skip)
    assert _same(o["plain"]["tr.train_log"], o["null"]["tr.train_log"])
    assert np.isnan(o["null"]["glog"]).all()                                  # no row written


def test_train_global_rejects_a_bad_fill_before_any_device_work(L, torch):
    I = _inputs(L, 32)
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    try:
        r = _Run(L, torch, s, I, 1)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        for fill in (-20, 10, 80):
            r.fill = fill
            with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                r.train(L, s, I, stream, 1)
        r.fill = 0
        I2 = dict(I, G=I["G"] - 1)                                           # capacity below G
        with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
            r.train(L, s, I2, stream, 1)
        torch.cuda.synchronize()
        assert r.tr["adam_step"].cpu().tolist() == [0]                        # nothing ran
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------
# Test 5: a checkpoint in the middle of a fill period
def test_checkpoint_mid_fill_resumes_bit_for_bit(L, tmp_path):
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    I = _inputs(L, 32)
    K, D = I["K"], I["D"]
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=B)
    pool = {k: np.ascontiguousarray(v) for k, v in I["pool"].items()}

    def fresh():
        pol = LmpcPolicy(B, weights=I["policy"].weights.copy(), critic_weights=I["policy"].critic_weights.copy())
        return dict(pol=pol, state=s.loop_state(D["state"][:B], policy=pol),
                    cs=L.LmpcSolver.collect_state(np.zeros((B, 2))), target=np.array(D["target"][:B]),
                    pvec=np.array(D["pvec"][:B]), adam=np.zeros((2, 77317), np.float32),
                    step=np.zeros(1, np.int32), best=ppo.new_best(), gbuf=ppo.new_global_buffer(I["n"]))

    def go(q, iterations, it0):
        return ppo.train_device(s, q["pol"], q["target"], q["pvec"], q["state"], q["cs"], q["adam"], q["step"], q["best"],
                                K, iterations=iterations, it0=it0, seed=SEED, rcfg=I["rcfg"], pool=pool, gamma=GAMMA,
                                lam=LAM, epochs=EPOCHS, mini_batch_size=MB, global_buffer=q["gbuf"], **HYPER)

    try:
        a = fresh()
        rows_a = go(a, 5, 0)
        b = fresh()
        rows_b = go(b, 3, 0)
        assert b["gbuf"]["fill"] == 3 * I["m"] and [r["global_update"] for r in rows_b] == [0.0] * 3
        path = ppo.save_checkpoint(tmp_path / "mid", b["pol"].weights, b["pol"].critic_weights, b["adam"], b["step"],
                                   b["best"], 3, b["state"]["obs_mean"], b["state"]["obs_M2"], b["state"]["obs_count"],
                                   b["state"]["history"], b["pol"].current_k, b["state"]["model_params"],
                                   global_buffer=b["gbuf"])
        ck = ppo.load_checkpoint(path)
        # fresh arrays for everything the checkpoint holds; the plants and the collection state stay in memory
        b["pol"] = LmpcPolicy(B, weights=ck["actor"].copy(), critic_weights=ck["critic"].copy())
        b["pol"].current_k[:] = ck["current_k"]
        b["adam"], b["step"] = ck["adam"].copy(), ck["adam_step"].copy()
        b["best"] = {k: ck[k].copy() for k in ("best_return", "best_weights", "best_iter")}
        for k in ("obs_mean", "obs_M2", "obs_count", "history", "model_params"):
            b["state"][k] = ck[k].copy()
        b["gbuf"] = ppo.global_buffer_from_checkpoint(ck)
        assert b["gbuf"]["fill"] == 3 * I["m"] and int(ck["iteration"][0]) == 3
        rows_b += go(b, 2, 3)
    finally:
        s.close()
    assert [r["global_update"] for r in rows_a] == [0.0, 0.0, 0.0, 1.0, 0.0]
    assert a["gbuf"]["fill"] == I["m"] == b["gbuf"]["fill"]
    assert set(L.GLOBAL_LOG_FIELDS) <= set(rows_a[0]) and set(L.TRAIN_LOG_FIELDS) <= set(rows_a[0])
    for ra, rb in zip(rows_a, rows_b):
        for k in ra:
            assert _same(np.array([ra[k]]), np.array([rb[k]])), k
    pairs = [(a["pol"].weights, b["pol"].weights), (a["pol"].critic_weights, b["pol"].critic_weights),
             (a["pol"].current_k, b["pol"].current_k), (a["adam"], b["adam"]), (a["step"], b["step"]),
             (a["target"], b["target"]), (a["pvec"], b["pvec"])]
    pairs += [(a["state"][k], b["state"][k]) for k in a["state"]] + [(a["cs"][k], b["cs"][k]) for k in a["cs"]]
    pairs += [(a["best"][k], b["best"][k]) for k in a["best"]]
    pairs += [(a["gbuf"][f][:I["m"]], b["gbuf"][f][:I["m"]]) for f in FIELDS]
    assert all(_same(np.asarray(x), np.asarray(y)) for x, y in pairs)
