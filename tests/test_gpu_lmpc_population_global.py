"""The global-buffer update of a population of LMPC learners (dart_lmpc_train_pop_global_dev /
dart_lmpc_train_pop_global; csrc/lmpc_train.hip: lmpc_gbuf_append_pop_kernel, lmpc_gae_seq_pop_kernel,
lmpc_pop_global_sample_kernel, lmpc_global_log_pop_kernel, lmpc_perm_pop_kernel cut to a choice; csrc/lmpc_ppo.hip:
critic_value_stride_pop_kernel and the update's *_pop_kernel forms on the buffers' rows).

The reference of every number is the single-learner entry: learner l of a population is, bit for bit,
train_global_dev on that learner's arrays, its buffer and its seed.  No tolerance anywhere.  Set-up of
test_gpu_lmpc_population.py (whose members, nets and device arrays are reused) and test_gpu_lmpc_global.py: N = 10,
B = 5, records every 2nd step, episodes of 12 steps, a reset pool of 2 rows, mini-batches of 16, 2 epochs, P = 3.
K = 32 gives n = 80, m = 20, G = 80 (period 4); K = 36 gives n = 90, m = 22, G = 110 > n (period 5): the last buffer
row, the capacity stride and the partial last mini-batch of the global update all differ from n.
"""
import numpy as np
import pytest

import test_gpu_lmpc_population as TP
from test_gpu_lmpc_population import B, EPOCHS, EVERY, HYPER, MB, NH, P, PAD, SEEDS, _assert_same, _dev, _ptrs, _same

pytestmark = pytest.mark.gpu

GPAT = 0x7fc0cafe       # a NaN pattern (fp32 words; an fp64 made of two of them is a NaN too)
FIELDS = ("obs", "action", "logp", "value", "reward", "done")


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _pattern(shape, dt):
    a = np.empty(shape, dt)
    a.view(np.int32)[...] = GPAT
    return a


def _is_pattern(a):
    return bool((np.ascontiguousarray(a).view(np.int32) == GPAT).all())


class _GRun(TP._Run):
    """TP._Run with the global buffers of its learners (nl = 0: the single entry's one buffer), `extra` rows beyond G
    each, every row starting as a NaN pattern."""

    def __init__(self, L, torch, host, C, iterations, nl, pad=None, extra=0):
        super().__init__(L, torch, host, C, iterations, nl, pad=pad)
        self.torch, self.iterations = torch, iterations
        nb = max(nl, 1)
        self.n = C["R"] * (self.B if nl else self.NI)
        self.m, self.G = L.global_rows(self.n)
        self.cap = self.G + extra
        self.gb = {f: _dev(torch, _pattern((nb, self.cap, w) if w else (nb, self.cap), dt))
                   for f, w, dt in L.LMPC_GLOBAL_ARRAYS}
        self.glog = torch.full((nb, iterations, 6), float("nan"), dtype=torch.float64, device="cuda")
        ws = (L.global_pop_workspace_bytes(nl, self.n, self.cap, EPOCHS, MB) if nl
              else L.global_workspace_bytes(self.n, EPOCHS, MB))
        assert ws > 0
        self.gws = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        self.fill = 0

    def train(self, L, s, C, pcfg, stream, iterations, seeds, it0=0, use_global=True, over=None, P_=None, B_=None,
              gover=None, cap=None, plain=False):
        """One call of `iterations` iterations; its log rows ([learners][iterations] of this call) are gathered into
        rows it0 .. of the run's logs."""
        torch = self.torch
        nb = max(self.nl, 1)
        tcfg = L.train_config(seed=int(seeds[0]) if not self.nl else 0, iterations=iterations, it0=it0, steps=C["K"])
        a = self.args(C, pcfg, tcfg, over)
        tlog = torch.full((nb, iterations, 12), float("nan"), dtype=torch.float64, device="cuda")
        glog = torch.full((nb, iterations, 6), float("nan"), dtype=torch.float64, device="cuda")
        a["train"]["train_log"] = tlog.data_ptr()
        g = None
        if use_global:
            g = L.global_buffer(dict(_ptrs(self.gb), **(gover or {})), self.cap if cap is None else cap, self.fill,
                                global_log=glog.data_ptr(), workspace=self.gws.data_ptr())
        if plain:
            L.LmpcSolver.train_pop_dev(s, self.nl, seeds, self.B, 2, stream=stream, **a)
        elif self.nl:
            L.LmpcSolver.train_pop_global_dev(s, self.nl if P_ is None else P_, seeds, self.B if B_ is None else B_, 2,
                                              gbuf=g, stream=stream, **a)
        else:
            s.train_global_dev(self.NI, 2, gbuf=g, stream=stream, **a)
        torch.cuda.synchronize()
        self.tr["train_log"][:, it0:it0 + iterations] = tlog
        self.glog[:, it0:it0 + iterations] = glog
        if use_global:
            self.fill = L.global_fill_after(self.n, self.fill, iterations)

    def member_snapshot(self, l, rows=None):
        out = super().member_snapshot(l)
        held = self.fill if rows is None else rows
        for f, v in self.gb.items():
            out["gb." + f] = np.ascontiguousarray(v.cpu().numpy()[l, :held])
        out["gb.fill"] = np.array([self.fill], np.int32)
        out["glog"] = np.ascontiguousarray(self.glog.cpu().numpy()[l])
        return out

    def extra_rows(self):
        return {f: v.cpu().numpy()[:, self.G:] for f, v in self.gb.items()}


def _single(L, torch, s, C, m, stream, iterations, seed):
    from dart_mpc import ppo
    r = _GRun(L, torch, ppo.population_stack([m]) | dict(critic=m["critic"], weights=m["weights"]), C, iterations, 0)
    torch.cuda.synchronize()
    r.train(L, s, C, m["pcfg"], stream, iterations, (seed,))
    return r.member_snapshot(0)


def _pop(L, torch, s, C, members, stream, iterations, seeds, calls=None, extra=0, **kw):
    from dart_mpc import ppo
    r = _GRun(L, torch, ppo.population_stack(members), C, iterations, len(members), pad=PAD, extra=extra)
    torch.cuda.synchronize()
    it0 = 0
    for c in calls or (iterations,):
        r.train(L, s, C, members[0]["pcfg"], stream, c, seeds, it0=it0, **kw)
        it0 += c
    assert it0 == iterations
    return r


def _period(L, K):
    n = K // EVERY * B
    m, G = L.global_rows(n)
    return n, m, G, G // m


def _host_run(L, s, C, iterations, calls, keep=None):
    """The host entry on the population, the buffers' rows starting as NaN patterns; returns the stacked arrays, the
    policies, the last call's outputs and the rows of every learner."""
    from dart_mpc import ppo
    M = TP._members(L, s)
    H = ppo.population_stack(M)
    pols = TP._policies(M)
    gb = ppo.new_population_global_buffer(P, C["R"] * B)
    for f in FIELDS:
        gb[f].view(np.int32)[...] = GPAT
    got, rows, it0 = {}, [[] for _ in range(P)], 0
    for c in calls:
        part = ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"],
                                    H["adam_step"], H["best"], C["K"], SEEDS, iterations=c, it0=it0, rcfg=C["rcfg"],
                                    pool=H["pool"], epochs=EPOCHS, mini_batch_size=MB, out=got, global_buffer=gb,
                                    **HYPER)
        for l in range(P):
            rows[l] += part[l]
        it0 += c
    H["global_buffer"] = gb
    return M, H, pols, got, rows


def _host_snapshot(H, pols, got, l, held):
    from dart_mpc import ppo
    out = TP._host_snapshot(H, pols, got, l)
    g = ppo.population_member(l, P, H)["global_buffer"]
    for f in FIELDS:
        out["gb." + f] = np.ascontiguousarray(g[f][:held])
    out["gb.fill"] = np.array([g["fill"]], np.int32)
    out["glog"] = np.ascontiguousarray(got["global_log"][l])
    return out


def _member_continues(L, s, C, total, l=1):
    """Two population iterations (host entry, mid fill), then learner l alone: its slice and its buffer through
    ppo.population_member, its training state through a checkpoint round trip, the rest through train_device."""
    import os
    import tempfile
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    M, H, pols, _, rows = _host_run(L, s, C, 2, (2,))
    mem = ppo.population_member(l, P, H)
    st = mem["state"]
    assert mem["global_buffer"]["fill"] == 2 * L.global_rows(C["R"] * B)[0]
    with tempfile.TemporaryDirectory() as tmp:
        path = ppo.save_checkpoint(os.path.join(tmp, "member"), pols[l].weights, pols[l].critic_weights, mem["adam"],
                                   mem["adam_step"], mem["best"], 2, st["obs_mean"], st["obs_M2"], st["obs_count"],
                                   st["history"], pols[l].current_k, st["model_params"],
                                   global_buffer=mem["global_buffer"])
        ck = ppo.load_checkpoint(path)
    gbuf = ppo.global_buffer_from_checkpoint(ck)
    assert int(ck["iteration"][0]) == 2 and gbuf["fill"] == mem["global_buffer"]["fill"]
    pol = LmpcPolicy(B, weights=ck["actor"].copy(), critic_weights=ck["critic"].copy(), current_k=ck["current_k"].copy())
    state = {k: np.array(v) for k, v in st.items()}
    for k in ("obs_mean", "obs_M2", "obs_count", "history", "model_params"):
        state[k] = ck[k].copy()
    q = dict(target=np.array(mem["target"]), plant_pvec=np.array(mem["plant_pvec"]), state=state,
             cstate={k: np.array(v) for k, v in mem["cstate"].items()}, adam=ck["adam"].copy(),
             adam_step=ck["adam_step"].copy(),
             best={k: ck[k].copy() for k in ("best_return", "best_weights", "best_iter")})
    got = {}
    rows_l = rows[l] + ppo.train_device(s, pol, q["target"], q["plant_pvec"], q["state"], q["cstate"], q["adam"],
                                        q["adam_step"], q["best"], C["K"], iterations=total - 2, it0=2, seed=SEEDS[l],
                                        rcfg=C["rcfg"], pool=mem["pool"], epochs=EPOCHS, mini_batch_size=MB, out=got,
                                        global_buffer=gbuf, **HYPER)
    held = gbuf["fill"]
    out = {"c.target": q["target"], "c.pvec": q["plant_pvec"], "c.current_k": pol.current_k, "c.weights": pol.weights,
           "c.critic": pol.critic_weights, "tr.adam": q["adam"], "tr.adam_step": q["adam_step"],
           "tr.best_return": q["best"]["best_return"], "tr.best_weights": q["best"]["best_weights"],
           "tr.best_iter": q["best"]["best_iter"], "gb.fill": np.array([held], np.int32)}
    for g, d in (("st", q["state"]), ("cs", q["cstate"]), ("lg", got["logs"]), ("clg", got["clogs"]),
                 ("rec", got["rec"])):
        for k, v in d.items():
            out[g + "." + k] = v
    for f in FIELDS:
        out["gb." + f] = gbuf[f][:held]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}, rows_l


@pytest.fixture(scope="module")
def runs(L, torch):
    """K = 32 and K = 36, period + 1 iterations: every learner alone through train_global_dev and the population; at
    K = 32 also the population again, split, with learner 1's seed changed and three rows of spare capacity, without
    a buffer, with one learner, through the host entry, and with a member continuing alone."""
    out = {}
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    try:
        for K in (32, 36):
            C = TP._cfgs(L, K)
            n, m, G, period = _period(L, K)
            its = period + 1
            o = dict(C=C, its=its)
            o["single"] = [_single(L, torch, s, C, mem, stream, its, SEEDS[l])
                           for l, mem in enumerate(TP._members(L, s))]
            pop = _pop(L, torch, s, C, TP._members(L, s), stream, its, SEEDS)
            o["pop"] = [pop.member_snapshot(l) for l in range(P)]
            o["pads"] = pop.pads()
            if K == 32:
                r = _pop(L, torch, s, C, TP._members(L, s), stream, its, SEEDS)
                o["again"] = [r.member_snapshot(l) for l in range(P)]
                for name, calls in (("split_a", (2, period - 1)), ("split_b", (period, 1))):
                    r = _pop(L, torch, s, C, TP._members(L, s), stream, its, SEEDS, calls=calls)
                    o[name] = [r.member_snapshot(l) for l in range(P)]
                r = _pop(L, torch, s, C, TP._members(L, s), stream, its, (SEEDS[0], 12345, SEEDS[2]), extra=3)
                o["other_seed"] = [r.member_snapshot(l) for l in range(P)]
                o["other_pads"], o["other_extra"] = r.pads(), r.extra_rows()
                r = _pop(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, use_global=False)
                o["null"] = [r.member_snapshot(l, rows=r.cap) for l in range(P)]
                r = _pop(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, use_global=False, plain=True)
                o["plain"] = [r.member_snapshot(l, rows=r.cap) for l in range(P)]
                r = _pop(L, torch, s, C, TP._members(L, s, [0]), stream, its, SEEDS[:1])
                o["one"] = r.member_snapshot(0)
                _, H, pols, got, rows = _host_run(L, s, C, its, (its,))
                held = L.global_fill_after(n, 0, its)
                o["host"] = [_host_snapshot(H, pols, got, l, held) for l in range(P)]
                o["host_rows"], o["host_buffer"], o["held"] = rows, H["global_buffer"], held
                o["member"], o["member_rows"] = _member_continues(L, s, C, its)
            out[K] = o
    finally:
        s.close()
    return out


# ------------------------------------------------------------------------------------------------------------------
# Test 1: population = P single runs
@pytest.mark.parametrize("K", [32, 36])
def test_population_equals_single_runs(L, runs, K):
    o = runs[K]
    n, m, G, period = _period(L, K)
    its = o["its"]
    steps_local, steps_global = EPOCHS * -(-n // MB), EPOCHS * -(-G // MB)
    for l in range(P):
        a, b = o["single"][l], o["pop"][l]
        print(f"K = {K}, learner {l}: train_log {np.array2string(b['tr.train_log'], precision=4)}")
        print(f"K = {K}, learner {l}: global_log {np.array2string(b['glog'], precision=4)}")
        glog = b["glog"]
        assert glog[:, 0].tolist() == [m * (j + 1) for j in range(period)] + [m]
        assert glog[:, 1].tolist() == [0.0] * (period - 1) + [1.0, 0.0] and (glog[:, 2] == G).all()
        assert np.isfinite(glog[period - 1, 3:]).all() and np.isnan(glog[period, 3:]).all()
        assert b["tr.adam_step"].tolist() == [its * steps_local + steps_global]
        assert b["gb.fill"].tolist() == [m] and b["gb.logp"].shape == (m,) and not _is_pattern(b["gb.obs"])
        _assert_same(a, b, f"learner {l} alone against learner {l} of the population, K = {K}")
    assert not _same(o["pop"][0]["c.weights"], o["pop"][1]["c.weights"])
    assert not _same(o["pop"][1]["gb.obs"], o["pop"][2]["gb.obs"])
    assert not _same(o["pop"][0]["glog"], o["pop"][2]["glog"])
    assert (o["pads"] == PAD).all()


# ------------------------------------------------------------------------------------------------------------------
# Test 2: the kernels alone, each against the single kernel per learner
def test_append_pop_equals_the_single_kernel_per_learner(L, torch):
    from dart_mpc import ppo
    from test_gpu_lmpc_global import REC, _patterns
    R, m, cap = 4, 5, 20
    n = R * B
    rng = np.random.default_rng(5)
    widths = dict(zip(REC, (520, 34, 0, 0, 0, 0)))
    dts = dict(zip(REC, (np.float32, np.float32, np.float32, np.float32, np.float64, np.float32)))
    rec = {k: _patterns(rng, (R, P * B, widths[k]) if widths[k] else (R, P * B), dts[k]) for k in REC}
    guard = {f: _patterns(rng, (P, cap, widths[k]) if widths[k] else (P, cap), dts[k]) for f, k in zip(FIELDS, REC)}
    sample = ppo.population_samples(P, B, R)
    stream = torch.cuda.current_stream().cuda_stream
    d_rec, d_sample = TP._to_dev(torch, rec), _dev(torch, sample)
    one, pop = TP._to_dev(torch, guard), TP._to_dev(torch, guard)
    want = {f: guard[f].copy() for f in FIELDS}
    # per learner: distinct choices, a repeated one, and one out of range (it must write nothing)
    for fill, choice in ((0, [[3, 11, 0, 7, 5], [19, 1, 2, 8, 4], [6, 6, 13, 0, 17]]),
                         (10, [[2, 2, 9, 1, 10], [5, n, 3, 3, 0], [-1, 18, 7, 12, 12]])):
        choice = np.array(choice, np.int32)
        d_choice = _dev(torch, choice)
        for l in range(P):
            g = L.global_buffer({f: one[f][l].data_ptr() for f in FIELDS}, cap, fill)
            L.global_append_dev(g, m, n, R * P * B, d_sample[l].data_ptr(), d_choice[l].data_ptr(), _ptrs(d_rec),
                                stream=stream)
        L.global_append_pop_dev(L.global_buffer(_ptrs(pop), cap, fill), P, m, n, R * P * B, d_sample.data_ptr(),
                                d_choice.data_ptr(), _ptrs(d_rec), stream=stream)
        torch.cuda.synchronize()
        for f, k in zip(FIELDS, REC):
            flat = rec[k].reshape(R * P * B, -1) if widths[k] else rec[k].reshape(R * P * B)
            for l in range(P):
                for j, c in enumerate(choice[l]):
                    if 0 <= c < n:
                        want[f][l, fill + j] = flat[sample[l, c]]
            got = pop[f].cpu().numpy()
            assert _same(got, one[f].cpu().numpy()), (fill, f)     # the single kernel's rows, guards included
            assert _same(got, want[f]), (fill, f)                  # = the stated rows; every other row untouched


@pytest.mark.parametrize("G", [1, 65, 1025])
def test_sequence_gae_pop_equals_the_single_kernel_per_learner(L, torch, G):
    cap = G + 2
    rng = np.random.default_rng(70 + G)
    reward = rng.standard_normal((P, cap)) * np.where(rng.random((P, cap)) < 0.2, 10.0, 1.0)
    value = rng.standard_normal((P, cap)).astype(np.float32)
    done = (rng.random((P, cap)) < 0.1).astype(np.float32)
    last = np.array([-0.83, 0.4, 1.7], np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    d = TP._to_dev(torch, dict(reward=reward, value=value, done=done, last=last))
    out = {k: _dev(torch, _pattern((P, cap), np.float64)) for k in ("adv1", "ret1", "advp", "retp")}
    for l in range(P):
        L.gae_seq_dev(G, 0.99, 0.95, d["reward"][l].data_ptr(), d["value"][l].data_ptr(), d["done"][l].data_ptr(),
                      d["last"][l:].data_ptr(), out["adv1"][l].data_ptr(), out["ret1"][l].data_ptr(), stream=stream)
    L.gae_seq_pop_dev(P, cap, G, 0.99, 0.95, d["reward"].data_ptr(), d["value"].data_ptr(), d["done"].data_ptr(),
                      d["last"].data_ptr(), out["advp"].data_ptr(), out["retp"].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert _same(h["adv1"], h["advp"]) and _same(h["ret1"], h["retp"])
    assert np.isfinite(h["advp"][:, :G]).all() and _is_pattern(h["advp"][:, G:]) and _is_pattern(h["retp"][:, G:])
    assert not _same(h["advp"][0, :G], h["advp"][1, :G])


@pytest.mark.parametrize("n,m", [(5, 1), (67, 16), (257, 64)])
def test_choice_pop_rows_are_the_single_choices(L, torch, n, m):
    stream = torch.cuda.current_stream().cuda_stream
    for it in (0, 3):
        pop = torch.full((P * m + 4,), -7, dtype=torch.int32, device="cuda")
        one = torch.full((P, m), -7, dtype=torch.int32, device="cuda")
        L.choice_pop_dev(SEEDS, it, n, m, pop.data_ptr(), stream=stream)
        for l in range(P):
            L.choice_dev(SEEDS[l], it, n, m, one[l].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        got = pop.cpu().numpy()
        assert (got[P * m:] == -7).all()                                   # nothing past [P][m]
        assert np.array_equal(got[:P * m].reshape(P, m), one.cpu().numpy())
        assert got[:P * m].min() >= 0 and got[:P * m].max() < n


# ------------------------------------------------------------------------------------------------------------------
# Test 3: chaining, a start inside a fill period, repeatability
def test_population_global_chains_and_repeats(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["pop"][l], o["again"][l], f"two runs, learner {l}")
        _assert_same(o["pop"][l], o["split_a"][l], f"one call against 2 + (period - 1), learner {l}")
        _assert_same(o["pop"][l], o["split_b"][l], f"one call against period + 1, learner {l}")


# ------------------------------------------------------------------------------------------------------------------
# Test 4: isolation
def test_population_global_learners_are_isolated(runs):
    o = runs[32]
    for l in (0, 2):
        _assert_same(o["pop"][l], o["other_seed"][l], f"learner {l} with another seed for learner 1")
    a, b = o["pop"][1], o["other_seed"][1]
    for k in ("rec.rec_action", "c.weights", "c.critic", "tr.adam", "tr.train_log", "glog", "gb.obs", "gb.action"):
        assert not _same(a[k], b[k]), k
    # capacity = G + 3: the spare rows of every learner keep their pattern, as do the critics' pad floats
    for f, v in o["other_extra"].items():
        assert v.shape[:2] == (P, 3) and _is_pattern(v), f
    assert (o["pads"] == PAD).all() and (o["other_pads"] == PAD).all()


# ------------------------------------------------------------------------------------------------------------------
# Test 5: without a buffer it is train_pop_dev
def test_null_buffer_is_train_pop_dev(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["plain"][l], o["null"][l], f"g = NULL against train_pop_dev, learner {l}")
        assert all(_is_pattern(o["null"][l]["gb." + f]) for f in FIELDS) and np.isnan(o["null"][l]["glog"]).all()
        assert o["null"][l]["tr.adam_step"][0] > 0


# ------------------------------------------------------------------------------------------------------------------
# Test 6: one learner
def test_population_of_one_equals_train_global_dev(runs):
    o = runs[32]
    _assert_same(o["single"][0], o["one"], "P = 1 against train_global_dev")


# ------------------------------------------------------------------------------------------------------------------
# Test 7: host entry = device entry
def test_population_global_host_entry_equals_device_entry(L, runs):
    o = runs[32]
    held = o["held"]
    assert held == L.global_rows(32 // EVERY * B)[0]
    for l in range(P):
        _assert_same(o["pop"][l], o["host"][l], f"host entry against device entry, learner {l}", skip=("c.prm",))
        rows = o["host_rows"][l]
        assert [r["global_update"] for r in rows] == o["pop"][l]["glog"][:, 1].tolist()
        assert [r["global_fill"] for r in rows] == o["pop"][l]["glog"][:, 0].tolist()
        assert set(L.GLOBAL_LOG_FIELDS) | set(L.TRAIN_LOG_FIELDS) <= set(rows[0])
    # only the rows held at the end came down: every other row of the host arrays keeps its pattern
    gb = o["host_buffer"]
    assert gb["fill"] == held
    for f in FIELDS:
        assert gb[f].shape[:2] == (P, 80) and _is_pattern(gb[f][:, held:]) and not _is_pattern(gb[f][:, :held]), f


# ------------------------------------------------------------------------------------------------------------------
# Test 8: a member continues alone from the middle of a fill period
def test_member_continues_alone_mid_fill(runs):
    o = runs[32]
    want, got = o["host"][1], o["member"]
    skip = ("tr.train_log", "glog")
    _assert_same({k: v for k, v in want.items() if k not in skip}, got,
                 "learner 1 continued alone against learner 1 of the population")
    for ra, rb in zip(o["host_rows"][1], o["member_rows"]):
        assert set(ra) == set(rb)
        for k in ra:
            assert _same(np.array([ra[k]]), np.array([rb[k]])), k
    assert len(o["member_rows"]) == o["its"]


# ------------------------------------------------------------------------------------------------------------------
# Test 9: refusals
def test_population_global_refusals(L, torch):
    from dart_mpc import ppo
    C = TP._cfgs(L, 32)
    n, m, G, _ = _period(L, 32)
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    small = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B - 1)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        M = TP._members(L, s)
        pcfg = M[0]["pcfg"]
        r = _GRun(L, torch, ppo.population_stack(M), C, 1, P)
        r.tr["workspace"].fill_(0xA5)
        r.gws.fill_(0xA5)
        r.cs["nrec"].fill_(-3)
        torch.cuda.synchronize()
        before = r.member_snapshot(1, rows=r.cap)
        many = tuple(range(L.POP_MAX + 1))
        rec_odd = dict(_ptrs(r.rec), rec_obs=r.rec["rec_obs"].data_ptr() + 4)
        cases = [("fill = m + 1", s, dict(fill=m + 1)), ("fill = n", s, dict(fill=n)),
                 ("capacity = G - 1", s, dict(cap=G - 1)), ("a null reward", s, dict(gover=dict(reward=0))),
                 ("obs off by 4 bytes", s, dict(gover=dict(obs=r.gb["obs"].data_ptr() + 4))),
                 ("rec_obs off by 4 bytes", s, dict(over=dict(rec=rec_odd))),
                 ("weights off by 4 bytes", s, dict(over=dict(weights=r.c["weights"].data_ptr() + 4))),
                 ("critic off by 4 bytes", s, dict(over=dict(critic=r.c["critic"].data_ptr() + 4))),
                 ("P = POP_MAX + 1", s, dict(P_=L.POP_MAX + 1, seeds=many, B_=1)),
                 ("P B = B_max + 1", small, dict())]
        for what, solver, kw in cases:
            seeds = kw.pop("seeds", SEEDS)
            r.fill = kw.pop("fill", 0)
            with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                r.train(L, solver, C, pcfg, stream, 1, seeds, **kw)
            torch.cuda.synchronize()
            r.fill = 0
            _assert_same(before, r.member_snapshot(1, rows=r.cap), what)
            assert bool((r.tr["workspace"] == 0xA5).all()) and bool((r.gws == 0xA5).all()), what   # nothing launched
            print("refused:", what)
        assert L.global_pop_workspace_bytes(0, n, G, EPOCHS, MB) == 0
        assert L.global_pop_workspace_bytes(P, n, G, EPOCHS, MB) > 0
    finally:
        s.close()
        small.close()


# ------------------------------------------------------------------------------------------------------------------
# Test 10: the switches of the iteration (no other training test sets them), each alone and all three together
SWITCHES = {"epochs = 0": dict(epochs=0), "mean_update = 0": dict(mean_update=0), "track_best = 0": dict(track_best=0),
            "all three": dict(epochs=0, mean_update=0, track_best=0)}


@pytest.mark.parametrize("with_global", [True, False])
@pytest.mark.parametrize("what", list(SWITCHES))
def test_switches_population_equals_single_runs(L, torch, what, with_global):
    """K = 8: n = 20 (one full and one ragged mini-batch of 16), m = 5, G = 20, period 4; period + 1 iterations, so
    that the update on the buffers runs once.  Learner l of train_pop_global_dev is train_global_dev on its member bit
    for bit, and each switch does what it says."""
    from dart_mpc import ppo
    sw = dict(epochs=EPOCHS, mean_update=1, track_best=1) | SWITCHES[what]
    K = 8
    C = TP._cfgs(L, K)
    n, m, G, period = _period(L, K)
    assert (n, m, G, period) == (20, 5, 20, 4)
    its = period + 1
    over = lambda seed: dict(ppo_cfg=L.ppo_config(epochs=sw["epochs"], mini_batch_size=MB, **HYPER),
                             tcfg=L.train_config(seed=seed, iterations=its, steps=K, mean_update=sw["mean_update"],
                                                 track_best=sw["track_best"]))
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        init = TP._members(L, s)
        single = []
        for l, mem in enumerate(TP._members(L, s)):
            r = _GRun(L, torch, ppo.population_stack([mem]) | dict(critic=mem["critic"], weights=mem["weights"]), C, its, 0)
            torch.cuda.synchronize()
            r.train(L, s, C, mem["pcfg"], stream, its, (SEEDS[l],), use_global=with_global, over=over(SEEDS[l]))
            single.append(r.member_snapshot(0, rows=None if with_global else r.cap))
        r = _GRun(L, torch, ppo.population_stack(TP._members(L, s)), C, its, P, pad=PAD)
        torch.cuda.synchronize()
        r.train(L, s, C, init[0]["pcfg"], stream, its, SEEDS, use_global=with_global, over=over(0))
        pop = [r.member_snapshot(l, rows=None if with_global else r.cap) for l in range(P)]
        assert (r.pads() == PAD).all()
    finally:
        s.close()
    steps = sw["epochs"] * -(-n // MB) * its + (sw["epochs"] * -(-G // MB) if with_global else 0)
    for l in range(P):
        b, start = pop[l], init[l]
        _assert_same(single[l], b, f"{what}: learner {l} alone against learner {l} of the population")
        log = b["tr.train_log"]
        print(f"{what}, buffer {with_global}, learner {l}: train_log {np.array2string(log, precision=4)}")
        assert log[:, 0].tolist() == [n] * its and b["tr.adam_step"].tolist() == [steps]
        nets_kept = _same(b["c.weights"], start["weights"]) and _same(b["c.critic"], start["critic"])
        if sw["epochs"] == 0:
            assert (log[:, 6:9] == 0).all() and nets_kept
        else:
            assert np.isfinite(log[:, 6:9]).all() and (log[:, 6:9] != 0).any() and not nets_kept
        if sw["mean_update"] == 0:
            # nothing but the parameter write sets current_k; model_params stays what the last step's policy left
            assert _same(b["c.current_k"], start["current_k"]) and _same(b["st.model_params"], b["lg.pvec"][-1])
        else:
            assert _same(b["c.current_k"], b["st.model_params"]) and not _same(b["c.current_k"], start["current_k"])
        if sw["track_best"] == 0:
            assert b["tr.best_return"].tolist() == [-np.inf] and b["tr.best_iter"].tolist() == [-1]
            assert not b["tr.best_weights"].any() and (log[:, 11] == 0).all()
        else:
            assert log[:, 11].sum() >= 1 and b["tr.best_iter"][0] >= 0 and b["tr.best_weights"].any()
        if with_global:
            glog = b["glog"]
            assert glog[:, 1].tolist() == [0.0] * (period - 1) + [1.0, 0.0] and b["gb.fill"].tolist() == [m]
            if sw["epochs"] == 0:
                assert (glog[period - 1, 3:] == 0).all()
        else:
            assert all(_is_pattern(b["gb." + f]) for f in FIELDS) and np.isnan(b["glog"]).all()
