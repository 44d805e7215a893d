"""Per-learner PPO hyper-parameters and the device-resident exploit/explore step of a population of LMPC learners
(dart_lmpc_train_pop_hyper(_dev), dart_lmpc_pbt_step(_dev); csrc/lmpc_ppo.hip: the table read by ppo_grad_pop_kernel
and ppo_apply_pop_kernel, csrc/lmpc_pbt.hip: lmpc_pbt_rank_kernel and lmpc_pbt_copy_kernel; dart_mpc.ppo: pbt_plan,
pbt_step, train_pbt).

Every comparison is bit for bit.  The reference of a trained learner is the single-learner entry: learner l of a
population with a table is train_dev (train_global_dev) on that learner's arrays with its seed and
ppo_config(**row l).  The reference of the step is ppo.pbt_plan, the numpy statement of the rule.  Set-up of
test_gpu_lmpc_population.py (whose nets, device arrays and snapshots are reused): N = 10, B = 5, records every 2nd
step, episodes of 12 steps, a reset pool of 2 rows, mini-batches of 16, 2 epochs, P = 3, K = 32 (five full
mini-batches) and K = 24 (the last one has 12), two iterations; four iterations with the global buffer, whose update
runs in the fourth (n = 80, m = 20, G = 80).  The whole cycle runs P = 4 learners of B = 4 instances.
"""
import numpy as np
import pytest

import test_gpu_lmpc_population as TP
import test_gpu_lmpc_population_global as TG
from test_gpu_lmpc_population import B, EPOCHS, EVERY, MB, NH, P, PAD, SEEDS, _assert_same, _dev, _ptrs, _same

pytestmark = pytest.mark.gpu

NACT, NCRIT, STRIDE, NPAR, COLS = 39748, 37569, 37572, 77317, 9
GUARD, GPAT = 16, 0x7fc0d00d            # guard words behind every array of the step's tests: a NaN pattern
PADPAT = 0x7fc0beef


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _table(L, P_, salt=0):
    """Rows that differ in all nine columns, every row a config the entries take."""
    l = np.arange(P_) + salt
    return L.hyper_table(P_, clip_eps=0.15 + 0.05 * l, vf_coef=0.2 + 0.1 * l, ent_coef=0.005 * (1 + l),
                         max_grad_norm=0.4 + 0.15 * l, lr=2e-4 * (1 + l), beta1=0.8 + 0.005 * l,
                         beta2=0.99 + 0.0002 * l, adam_eps=1e-8 * (1 + l), weight_decay=1e-5 * (1 + 2 * l))


def _row_cfg(L, row):
    return L.ppo_config(epochs=EPOCHS, mini_batch_size=MB, **dict(zip(L.HYPER_FIELDS, (float(v) for v in row))))


def _members(L, s, P_, B_):
    """TP._members for P_ learners of B_ instances (fresh host arrays; the nets are TP._nets(l))."""
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    n = D["state"].shape[0]
    assert n >= P_ * B_
    out = []
    for l in range(P_):
        sl = slice(l * B_, (l + 1) * B_)
        actor, critic = TP._nets(l)
        pol = LmpcPolicy(B_, weights=actor.copy(), critic_weights=critic.copy(), seed=l)
        idx = (np.arange(2)[:, None] * 7 + np.arange(B_)[None] + B_ + 3 * l + 1) % n
        out.append(dict(target=np.ascontiguousarray(D["target"][sl]), plant_pvec=np.ascontiguousarray(D["pvec"][sl]),
                        state=s.loop_state(D["state"][sl], policy=pol),
                        cstate=L.LmpcSolver.collect_state(np.zeros((B_, 2))), adam=np.zeros((2, NPAR), np.float32),
                        adam_step=np.zeros(1, np.int32), best=ppo.new_best(),
                        pool={k: np.ascontiguousarray(v) for k, v in
                              dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx]).items()},
                        current_k=pol.current_k.copy(), weights=actor.copy(), critic=critic.copy(), pcfg=pol.cfg))
    return out


def _hyper_call(L, torch, s, r, C, pcfg, stream, seeds, hyper, it0=0, iterations=1, gbuf=None, over=None, cfg=None):
    """One call of train_pop_hyper_dev on the run r (TP._Run / TG._GRun), asynchronous; returns the call's log tensor
    [P][iterations][12] (kept alive by the caller until the stream is synchronised)."""
    tcfg = L.train_config(seed=0, iterations=iterations, it0=it0, steps=C["K"])
    a = r.args(C if cfg is None else dict(C, cfg=cfg), pcfg, tcfg, over)
    tlog = torch.full((r.nl, iterations, 12), float("nan"), dtype=torch.float64, device="cuda")
    a["train"]["train_log"] = tlog.data_ptr()
    s.train_pop_hyper_dev(r.nl, seeds, r.B, 2, gbuf=gbuf, hyper=hyper, stream=stream, **a)
    return tlog


def _pop_hyper(L, torch, s, C, members, stream, iterations, seeds, table, cfg=None):
    """A population run through the table's entry, one call; table None: hyper = NULL."""
    from dart_mpc import ppo
    r = TP._Run(L, torch, ppo.population_stack(members), C, iterations, len(members), pad=PAD)
    t = None if table is None else _dev(torch, table)
    torch.cuda.synchronize()
    tlog = _hyper_call(L, torch, s, r, C, members[0]["pcfg"], stream, seeds, 0 if t is None else t.data_ptr(),
                       iterations=iterations, cfg=cfg)
    torch.cuda.synchronize()
    r.tr["train_log"] = tlog
    return r


def _single_cfg(L, torch, s, C, m, stream, iterations, seed, cfgs, it0=0):
    """Learner alone through train_dev: one chained call of one iteration per config in `cfgs` (or one call of
    `iterations` with a single config), no synchronisation between the calls."""
    from dart_mpc import ppo
    r = TP._Run(L, torch, ppo.population_stack([m]) | dict(critic=m["critic"], weights=m["weights"]), C, iterations, 0)
    torch.cuda.synchronize()
    if len(cfgs) == 1:
        r.train(L, s, dict(C, cfg=cfgs[0]), m["pcfg"], stream, iterations, (seed,), it0=it0)
    else:
        assert len(cfgs) == iterations
        for j, cfg in enumerate(cfgs):
            r.train(L, s, dict(C, cfg=cfg), m["pcfg"], stream, 1, (seed,), it0=it0 + j, row0=j)
    torch.cuda.synchronize()
    return r.member_snapshot(0)


@pytest.fixture(scope="module")
def runs(L, torch):
    out = {}
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    stream = torch.cuda.Stream().cuda_stream
    try:
        T = _table(L, P)
        out["table"] = T
        for K in (32, 24):
            C = TP._cfgs(L, K)
            o = dict(C=C)
            o["single"] = [_single_cfg(L, torch, s, C, m, stream, 2, SEEDS[l], [_row_cfg(L, T[l])])
                           for l, m in enumerate(TP._members(L, s))]
            r = _pop_hyper(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, T)
            o["pop"] = [r.member_snapshot(l) for l in range(P)]
            o["pads"] = r.pads()
            if K == 32:
                # the shared config three ways: train_pop_dev, a table of equal rows, no table
                r = TP._pop(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS)
                o["plain"] = [r.member_snapshot(l) for l in range(P)]
                cfg = C["cfg"]
                E = np.tile(np.array([getattr(cfg, f) for f in L.HYPER_FIELDS]), (P, 1))
                # (the shared config handed over beside an equal table is another one: only the table may count)
                other = L.ppo_config(epochs=EPOCHS, mini_batch_size=MB, clip_eps=0.37, vf_coef=0.9, ent_coef=0.2,
                                     max_grad_norm=3.0, lr=0.01, beta1=0.5, beta2=0.7, adam_eps=1e-3, weight_decay=0.1)
                r = _pop_hyper(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, E, cfg=other)
                o["equal"] = [r.member_snapshot(l) for l in range(P)]
                r = _pop_hyper(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, None)
                o["null"] = [r.member_snapshot(l) for l in range(P)]
                # isolation: row 1 changed
                T1 = T.copy()
                T1[1] = _table(L, P, salt=5)[1]
                r = _pop_hyper(L, torch, s, C, TP._members(L, s), stream, 2, SEEDS, T1)
                o["other_row"] = [r.member_snapshot(l) for l in range(P)]
                # the table read at run time: two chained calls, the table overwritten on the stream in between
                Tb = _table(L, P, salt=3)
                o["chained"] = _chained(L, torch, s, C, T, Tb)
                o["chained_single"] = [
                    _single_cfg(L, torch, s, C, m, stream, 2, SEEDS[l], [_row_cfg(L, T[l]), _row_cfg(L, Tb[l])])
                    for l, m in enumerate(TP._members(L, s))]
                # the host entry
                o["host"] = _host(L, s, C, T)
            out[K] = o
    finally:
        s.close()
    return out


def _chained(L, torch, s, C, Ta, Tb):
    from dart_mpc import ppo
    M = TP._members(L, s)
    r = TP._Run(L, torch, ppo.population_stack(M), C, 2, P, pad=PAD)
    t, tb = _dev(torch, Ta), _dev(torch, Tb)
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(ts):
        log0 = _hyper_call(L, torch, s, r, C, M[0]["pcfg"], ts.cuda_stream, SEEDS, t.data_ptr(), it0=0)
        t.copy_(tb, non_blocking=True)                  # on the same stream, nothing waits for it
        log1 = _hyper_call(L, torch, s, r, C, M[0]["pcfg"], ts.cuda_stream, SEEDS, t.data_ptr(), it0=1)
    torch.cuda.synchronize()
    r.tr["train_log"] = torch.cat([log0, log1], dim=1)
    return [r.member_snapshot(l) for l in range(P)]


def _host(L, s, C, T):
    from dart_mpc import ppo
    M = TP._members(L, s)
    H = ppo.population_stack(M)
    pols = TP._policies(M)
    got = {}
    ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"], H["adam_step"],
                         H["best"], C["K"], SEEDS, iterations=2, rcfg=C["rcfg"], pool=H["pool"], epochs=EPOCHS,
                         mini_batch_size=MB, out=got, hyper_table=T)
    return [TP._host_snapshot(H, pols, got, l) for l in range(P)]


# ------------------------------------------------------------------------------------------------------------------
# Test 1: equal rows = the shared config; no table = the shared config
def test_equal_rows_and_null_table_equal_train_pop_dev(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["plain"][l], o["equal"][l], f"a table of equal rows against train_pop_dev, learner {l}")
        _assert_same(o["plain"][l], o["null"][l], f"hyper = NULL against train_pop_dev, learner {l}")


@pytest.fixture(scope="module")
def global_runs(L, torch):
    """With the global buffer (TG's set-up), four iterations: the global update runs in the fourth."""
    from dart_mpc import ppo
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    stream = torch.cuda.Stream().cuda_stream
    C = TP._cfgs(L, 32)
    T = _table(L, P)
    cfg = C["cfg"]
    E = np.tile(np.array([getattr(cfg, f) for f in L.HYPER_FIELDS]), (P, 1))
    o = {}
    try:
        r = TG._pop(L, torch, s, C, TP._members(L, s), stream, 4, SEEDS)
        o["plain"] = [r.member_snapshot(l) for l in range(P)]
        for name, table in (("equal", E), ("distinct", T)):
            M = TP._members(L, s)
            r = TG._GRun(L, torch, ppo.population_stack(M), C, 4, P, pad=PAD)
            t = _dev(torch, table)
            g = L.global_buffer(_ptrs(r.gb), r.cap, 0, global_log=r.glog.data_ptr(), workspace=r.gws.data_ptr())
            torch.cuda.synchronize()
            tlog = _hyper_call(L, torch, s, r, C, M[0]["pcfg"], stream, SEEDS, t.data_ptr(), iterations=4, gbuf=g)
            torch.cuda.synchronize()
            r.tr["train_log"] = tlog
            r.fill = L.global_fill_after(r.n, 0, 4)
            o[name] = [r.member_snapshot(l) for l in range(P)]
        single = []
        for l, m in enumerate(TP._members(L, s)):
            r = TG._GRun(L, torch, ppo.population_stack([m]) | dict(critic=m["critic"], weights=m["weights"]), C, 4, 0)
            torch.cuda.synchronize()
            r.train(L, s, dict(C, cfg=_row_cfg(L, T[l])), m["pcfg"], stream, 4, (SEEDS[l],))
            single.append(r.member_snapshot(0))
        o["single"] = single
    finally:
        s.close()
    return o


def test_table_with_the_global_buffer(global_runs):
    o = global_runs
    for l in range(P):
        assert o["plain"][l]["glog"][:, 1].tolist() == [0, 0, 0, 1], "the global update must run in the fourth"
        _assert_same(o["plain"][l], o["equal"][l], f"equal rows against train_pop_global_dev, learner {l}")
        _assert_same(o["single"][l], o["distinct"][l], f"learner {l} alone (train_global_dev) against the table's run")
    assert not _same(o["plain"][0]["c.weights"], o["distinct"][0]["c.weights"])


# Test 2: distinct rows = P single runs with ppo_config(**row)
@pytest.mark.parametrize("K", [32, 24])
def test_distinct_rows_equal_single_runs(runs, K):
    o = runs[K]
    n = K // EVERY * B
    for l in range(P):
        a, b = o["single"][l], o["pop"][l]
        print(f"K = {K}, learner {l}: rows {np.array2string(b['tr.train_log'], precision=4)}")
        assert b["tr.adam_step"].tolist() == [2 * EPOCHS * -(-n // MB)]
        _assert_same(a, b, f"learner {l} alone with its row against learner {l} of the population, K = {K}")
    assert (o["pads"] == PAD).all()
    if K == 32:     # the table did something: no learner is its shared-config run
        for l in range(P):
            assert not _same(o["plain"][l]["c.weights"], o["pop"][l]["c.weights"]), l


# Test 3: isolation
def test_rows_are_isolated(runs):
    o = runs[32]
    for l in (0, 2):
        _assert_same(o["pop"][l], o["other_row"][l], f"learner {l} with another row for learner 1")
    a, b = o["pop"][1], o["other_row"][1]
    for k in ("c.weights", "c.critic", "tr.adam", "tr.train_log"):
        assert not _same(a[k], b[k]), k


# Test 4: the table is read when the kernels run
def test_table_is_read_at_run_time(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["chained_single"][l], o["chained"][l],
                     f"learner {l}: config a then config b alone against the table rewritten between two calls")
        assert not _same(o["chained"][l]["c.weights"], o["pop"][l]["c.weights"]), l


# Test 8a: the host entry with a table = the device entry
def test_host_entry_with_table_equals_device_entry(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["pop"][l], o["host"][l], f"host entry against device entry, learner {l}", skip=("c.prm",))


# ------------------------------------------------------------------------------------------------------------------
# The step alone, on synthetic arrays

def _guarded(torch, a):
    """`a` on the device with GUARD words of a NaN pattern behind it: (the whole tensor, the view of a)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    words = flat.itemsize // 4 * GUARD
    whole = np.concatenate([flat.view(np.int32), np.full(words, GPAT, np.int32)])
    t = _dev(torch, whole)
    return t, t[:flat.size * flat.itemsize // 4]


class _Step:
    """The step's arrays for P_ learners: random bits everywhere (NaN and inf patterns among them), a planted pattern
    in the critics' pad floats, guard words behind every array; `fitness` at `stride`."""

    def __init__(self, L, torch, P_, fitness, stride, table, seed=0, adam_shift=0):
        rng = np.random.default_rng(1000 + P_ + seed)
        bits = lambda *shape: rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
        self.P, self.stride, self.L, self.torch = P_, stride, L, torch
        self.h = dict(weights=bits(P_, NACT).view(np.float32), critic=bits(P_, STRIDE).view(np.float32),
                      adam=bits(P_, 2, NPAR).view(np.float32), adam_step=(np.arange(P_) * 7 + 3).astype(np.int32),
                      hyper=np.array(table, np.float64), rank=np.full(P_, -7, np.int32),
                      parent=np.full(P_, -7, np.int32))
        self.h["critic"].view(np.int32)[:, NCRIT:] = PADPAT
        fit = np.full((P_ - 1) * stride + 1, 123.0)
        fit[::stride] = fitness
        self.h["fitness"] = fit
        # adam_shift floats in front of adam: rows that are only 4-byte aligned
        if adam_shift:
            self.h["adam"] = np.concatenate([np.zeros(adam_shift, np.float32), self.h["adam"].reshape(-1)])
        self.whole, self.d = {}, {}
        for k, v in self.h.items():
            self.whole[k], self.d[k] = _guarded(torch, v)
        self.adam_shift = adam_shift
        torch.cuda.synchronize()

    def ptr(self, k):
        return self.d[k].data_ptr() + (4 * self.adam_shift if k == "adam" else 0)

    def run(self, cfg, stream=0, over=None, P_=None, stride=None):
        p = {k: self.ptr(k) for k in self.h}
        p.update(over or {})
        self.L.LmpcSolver.pbt_step_dev(cfg, self.P if P_ is None else P_, p["fitness"],
                                       self.stride if stride is None else stride, p["weights"], p["critic"], p["adam"],
                                       p["adam_step"], p["hyper"], p["rank"], p["parent"], stream=stream)
        self.torch.cuda.synchronize()

    def host(self):
        """Everything on the device now, guards included, as int32 words."""
        return {k: v.cpu().numpy().copy() for k, v in self.whole.items()}

    def expected(self, rank, parent, table):
        """The words the device must hold after a step with this plan, from the initial host arrays."""
        from dart_mpc import ppo
        h = {k: v.copy() for k, v in self.h.items()}
        adam = h["adam"][self.adam_shift:].reshape(self.P, 2, NPAR) if self.adam_shift else h["adam"]
        ppo.pbt_apply(parent, h["weights"], h["critic"], adam, h["adam_step"])
        h["hyper"], h["rank"], h["parent"] = table, rank, parent
        out = {}
        for k, v in h.items():
            flat = np.ascontiguousarray(v).reshape(-1)
            out[k] = np.concatenate([flat.view(np.int32), np.full(flat.itemsize // 4 * GUARD, GPAT, np.int32)])
        return out


def _fitness(P_):
    """Ties, a NaN, +inf and -inf where the population is large enough for them."""
    f = np.array([3.0, 1.0, 1.0, np.nan, np.inf, -np.inf, 2.0, np.nan, 0.0, -0.0][:P_])
    if P_ > f.size:
        f = np.concatenate([f, (np.arange(P_ - f.size) * 5 % 7).astype(np.float64) - 2.5])
    return f


def _step_cases():
    cases, i = [], 0
    for P_ in (1, 2, 3, 8, 32):
        for k in sorted({0, 1, P_ // 2}):
            if k and 2 * k > P_:
                continue
            for higher in (0, 1):
                cases.append((P_, k, higher, (1, 8)[i % 2], i))
                i += 1
    return cases


# Test 5
@pytest.mark.parametrize("P_,k,higher,stride,i", _step_cases())
def test_step_matches_plan(L, torch, P_, k, higher, stride, i):
    from dart_mpc import ppo
    # every mask bit over the cases; bounds that bind from below (lr) and from above (clip_eps, beta2)
    mask = [0x15, 0x1ff, 0x0aa, 0x001 << (i % 9), 0x155][i % 5]
    T = _table(L, P_)
    T[:, 4] = 1.1e-6 * (1 + np.arange(P_) % 3)          # lr near its lower bound
    T[:, 0] = 0.45 + 0.01 * (np.arange(P_) % 4)         # clip_eps near its upper bound
    if P_ >= 2:
        T[1, 2] = np.nan                                # a NaN entry passes through factor and clamp
    settings = dict(n_replace=k, higher_is_better=higher, explore_mask=mask, factor_down=0.8, factor_up=1.25,
                    lo=dict(lr=1e-6, clip_eps=0.01), hi=dict(clip_eps=0.5, beta2=0.9905))
    f = _fitness(P_)
    seed, gen = 2 ** 40 + 17 + i, 3 + i
    rank, parent, table = ppo.pbt_plan(f, T, seed=seed, generation=gen, **settings)
    S = _Step(L, torch, P_, f, stride, T, adam_shift=1 if i % 7 == 3 else 0)
    cfg = L.pbt_config(seed=seed, generation=gen, **settings)
    S.run(cfg)
    got, want = S.host(), S.expected(rank, parent, table)
    bad = [key for key in want if not np.array_equal(got[key], want[key])]
    assert not bad, (bad, rank, parent, got["rank"][:P_], got["parent"][:P_])
    k_eff = k or P_ // 4
    assert sorted(rank.tolist()) == list(range(P_))
    assert int((parent != np.arange(P_)).sum()) <= k_eff and set(rank[parent[parent != np.arange(P_)]]) <= set(range(k_eff))
    if k_eff:
        assert (rank[parent != np.arange(P_)] >= P_ - k_eff).all()
        assert int((rank >= P_ - k_eff).sum()) == k_eff


def test_step_repeats_and_depends_on_seed_and_generation(L, torch):
    from dart_mpc import ppo
    P_, f, T = 32, _fitness(32), _table(L, 32) * np.array([0.5, 1, 0.2, 1, 0.1, 1, 1, 1, 1])
    settings = dict(n_replace=16, explore_mask=0x1ff)
    words = []
    for seed, gen in ((5, 0), (5, 0), (5, 1), (6, 0)):
        S = _Step(L, torch, P_, f, 1, T)
        S.run(L.pbt_config(seed=seed, generation=gen, **settings))
        got = S.host()
        want = S.expected(*ppo.pbt_plan(f, T, seed=seed, generation=gen, **settings))
        assert all(np.array_equal(got[key], want[key]) for key in want), (seed, gen)
        words.append(got)
    same = lambda a, b: all(np.array_equal(a[key], b[key]) for key in a)
    assert same(words[0], words[1]), "two runs"
    for j in (2, 3):
        assert not np.array_equal(words[0]["parent"], words[j]["parent"]), "the parents' draws"
        assert not np.array_equal(words[0]["hyper"], words[j]["hyper"]), "the perturbations' draws"


# Test 6
@pytest.mark.parametrize("P_", [1, 3])
def test_step_with_nothing_to_do(L, torch, P_):
    f = _fitness(P_)
    S = _Step(L, torch, P_, f, 1, _table(L, P_))
    before = S.host()
    S.run(L.pbt_config(seed=9, explore_mask=0x1ff))         # k = P / 4 = 0
    got = S.host()
    for key in before:
        if key not in ("rank", "parent"):
            assert np.array_equal(before[key], got[key]), key
    assert got["parent"][:P_].tolist() == list(range(P_))
    assert got["rank"][:P_].tolist() == {1: [0], 3: [2, 0, 1]}[P_]      # lower is better: 1.0 (index 1), 1.0, 3.0
    assert (got["rank"][P_:] == GPAT).all() and (got["parent"][P_:] == GPAT).all()


# Test 8b: the host entry of the step = the device entry
def test_step_host_entry_equals_device_entry(L, torch):
    from dart_mpc import ppo
    P_, f, T = 8, _fitness(8), _table(L, 8)
    settings = dict(n_replace=3, higher_is_better=1, explore_mask=0x1ff)
    S = _Step(L, torch, P_, f, 8, T)
    S.run(L.pbt_config(seed=77, generation=2, **settings))
    got = S.host()
    pop = {k: S.h[k].copy() for k in ("weights", "critic", "adam", "adam_step")}
    hyper = T.copy()
    res = ppo.pbt_step(pop, hyper, S.h["fitness"], seed=77, generation=2, fitness_stride=8, **settings)
    words = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.int32)
    for key, a in dict(pop, hyper=hyper, rank=res["rank"], parent=res["parent"]).items():
        assert np.array_equal(words(a), got[key][:words(a).size]), key
    assert (res["parent"] != np.arange(P_)).sum() == 3


# Test 9: refusals
def test_step_refusals(L, torch):
    P_ = 8
    S = _Step(L, torch, P_, _fitness(P_), 1, _table(L, P_))
    before = S.host()
    ok = dict(seed=1, n_replace=2)
    nan = float("nan")
    cases = [("P = 0", dict(P_=0), ok), ("P = POP_MAX + 1", dict(P_=L.POP_MAX + 1), ok),
             ("k < 0", {}, dict(ok, n_replace=-1)), ("2 k > P", {}, dict(ok, n_replace=5)),
             ("fitness_stride = 0", dict(stride=0), ok), ("generation < 0", {}, dict(ok, generation=-1)),
             ("lo > hi", {}, dict(ok, lo=dict(lr=1e-2), hi=dict(lr=1e-3))), ("a NaN bound", {}, dict(ok, hi=dict(lr=nan))),
             ("a NaN lower bound", {}, dict(ok, lo=dict(vf_coef=nan))),
             ("factor_down = 0", {}, dict(ok, factor_down=0.0)), ("factor_up < 0", {}, dict(ok, factor_up=-1.25)),
             ("a NaN factor", {}, dict(ok, factor_up=nan)),
             ("weights off by 4 bytes", dict(over=dict(weights=S.ptr("weights") + 4)), ok),
             ("critic off by 8 bytes", dict(over=dict(critic=S.ptr("critic") + 8)), ok)]
    cases += [(f"null {name}", dict(over={name: 0}), ok) for name in S.h]
    for what, kw, settings in cases:
        with pytest.raises(L.DartMPCError, match=r"\(-1"):
            S.run(L.pbt_config(**settings), **kw)
        torch.cuda.synchronize()
        got = S.host()
        assert all(np.array_equal(before[key], got[key]) for key in before), what      # nothing was launched
        print("refused:", what)
    # the host entry of the step
    from dart_mpc import ppo
    pop = {k: S.h[k].copy() for k in ("weights", "critic", "adam", "adam_step")}
    hyper = S.h["hyper"].copy()
    with pytest.raises(L.DartMPCError, match=r"\(-1"):
        L.pbt_step(L.pbt_config(n_replace=5), S.h["fitness"], pop["weights"], pop["critic"], pop["adam"],
                   pop["adam_step"], hyper)
    assert all(_same(pop[k], S.h[k]) for k in pop) and _same(hyper, S.h["hyper"])


def test_training_refuses_a_bad_table(L, torch):
    """The host training entry refuses a row that is no config, before any device work; the device entry refuses a
    table without a population's shape as train_pop_dev does, and launches nothing."""
    from dart_mpc import ppo
    C = TP._cfgs(L, 32)
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for col, bad in (("lr", float("nan")), ("lr", -1e-4), ("beta1", 1.0), ("clip_eps", -0.1), ("adam_eps", -1.0),
                         ("max_grad_norm", float("nan")), ("beta2", -0.5)):
            T = _table(L, P)
            T[2, L.HYPER_FIELDS.index(col)] = bad
            M = TP._members(L, s)
            H = ppo.population_stack(M)
            pols = TP._policies(M)
            w0, a0 = [p.weights.copy() for p in pols], H["adam"].copy()
            x0 = H["state"]["x"].copy()
            with pytest.raises(L.DartMPCError, match=r"\(-1\).*hyper-parameter table"):
                ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"],
                                     H["adam_step"], H["best"], 32, SEEDS, rcfg=C["rcfg"], pool=H["pool"], epochs=EPOCHS,
                                     mini_batch_size=MB, hyper_table=T)
            assert H["adam_step"].tolist() == [0] * P and all(_same(a, p.weights) for a, p in zip(w0, pols)), col
            assert _same(a0, H["adam"]) and _same(x0, H["state"]["x"]), col
        # the device entry: the refusals of train_pop_dev hold with a table, and nothing is launched
        M = TP._members(L, s)
        r = TP._Run(L, torch, ppo.population_stack(M), C, 1, P)
        r.tr["workspace"].fill_(0xA5)
        t = _dev(torch, _table(L, P))
        torch.cuda.synchronize()
        before = r.member_snapshot(1)
        for what, over in (("critic off by 4 bytes", dict(critic=r.c["critic"].data_ptr() + 4)),
                           ("weights off by 4 bytes", dict(weights=r.c["weights"].data_ptr() + 4))):
            with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                _hyper_call(L, torch, s, r, C, M[0]["pcfg"], stream, SEEDS, t.data_ptr(), over=over)
            torch.cuda.synchronize()
            _assert_same(before, r.member_snapshot(1), what)
            assert bool((r.tr["workspace"] == 0xA5).all()), what
        with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
            _hyper_call(L, torch, s, r, C, M[0]["pcfg"], stream, None, t.data_ptr())        # null seeds
        torch.cuda.synchronize()
        assert bool((r.tr["workspace"] == 0xA5).all())
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------
# Test 7: train -> evaluate -> step -> train on one stream against the same cycle done by hand

CP, CB, CK, ESTEPS, SLOT = 4, 4, 32, 16, 0
CSEEDS = (21, 5, 2 ** 33 + 1, 8)
PBT = dict(seed=4242, n_replace=1, explore_mask=0x1ff)


def _eval_inputs(L, torch, s, r):
    """The evaluation's device arrays for the run r: every learner on the same CB experiments, zeroed loop state."""
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    NI = CP * CB
    tile = lambda a: np.ascontiguousarray(np.tile(np.asarray(a, np.float64)[:CB], (CP, 1)))
    st = {name: np.zeros(L._loop_shape(NI, width, nw=s.nw), dt) for name, width, dt in L.LMPC_LOOP_STATE}
    st["x"][:] = tile(D["state"][10:10 + CB])
    st["metrics"] = L.loop_metrics(NI)
    e = dict(state={k: _dev(torch, v) for k, v in st.items()}, target=_dev(torch, tile(D["target"][10:10 + CB])),
             pvec=_dev(torch, tile(D["pvec"][10:10 + CB])), prm=_dev(torch, np.tile(L.LMPC_PRM_DEFAULT, (NI, 1))),
             scores=torch.full((CP, 8), float("nan"), dtype=torch.float64, device="cuda"),
             x0=D["state"][10:10 + CB], targets=D["target"][10:10 + CB], pvecs=D["pvec"][10:10 + CB])
    return e


def _evaluate(L, torch, s, r, e, pcfg, stream):
    """evaluate_dev (metrics only) on copies of the learners' policy state, enqueued on the current torch stream."""
    for name in ("obs_mean", "obs_M2", "obs_count", "history", "timestep", "model_params"):
        e["state"][name].copy_(r.st[name].reshape(e["state"][name].shape), non_blocking=True)
    s.evaluate_dev(CP, CB, 0, ESTEPS, ESTEPS, e["target"].data_ptr(), e["prm"].data_ptr(), e["pvec"].data_ptr(),
                   _ptrs(e["state"]), None, pcfg=pcfg, weights=r.c["weights"].data_ptr(),
                   current_k=r.c["current_k"].data_ptr(), scores=e["scores"].data_ptr(), stream=stream)


@pytest.fixture(scope="module")
def cycle(L, torch):
    from dart_mpc import ppo
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=CP * CB)
    C = TP._cfgs(L, CK)
    T = _table(L, CP)
    o = dict(table=T)
    try:
        # (a) one stream, no synchronisation
        M = _members(L, s, CP, CB)
        pcfg = M[0]["pcfg"]
        r = TP._Run(L, torch, ppo.population_stack(M), C, 2, CP, pad=PAD)
        e = _eval_inputs(L, torch, s, r)
        t = _dev(torch, T)
        rank = torch.full((CP,), -1, dtype=torch.int32, device="cuda")
        parent = torch.full((CP,), -1, dtype=torch.int32, device="cuda")
        ts = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            log0 = _hyper_call(L, torch, s, r, C, pcfg, ts.cuda_stream, CSEEDS, t.data_ptr(), it0=0)
            _evaluate(L, torch, s, r, e, pcfg, ts.cuda_stream)
            s.pbt_step_dev(L.pbt_config(generation=0, **PBT), CP, e["scores"].data_ptr() + 8 * SLOT, 8,
                           r.c["weights"].data_ptr(), r.c["critic"].data_ptr(), r.tr["adam"].data_ptr(),
                           r.tr["adam_step"].data_ptr(), t.data_ptr(), rank.data_ptr(), parent.data_ptr(),
                           stream=ts.cuda_stream)
            log1 = _hyper_call(L, torch, s, r, C, pcfg, ts.cuda_stream, CSEEDS, t.data_ptr(), it0=1)
        torch.cuda.synchronize()
        r.tr["train_log"] = torch.cat([log0, log1], dim=1)
        o["stream"] = [r.member_snapshot(l) for l in range(CP)]
        o["stream_rank"], o["stream_parent"] = rank.cpu().numpy(), parent.cpu().numpy()
        o["stream_table"], o["stream_scores"] = t.cpu().numpy(), e["scores"].cpu().numpy()
        o["pads"] = r.pads()

        # (b) by hand: synchronise after each part, the plan in numpy, every learner alone
        M = _members(L, s, CP, CB)
        r = TP._Run(L, torch, ppo.population_stack(M), C, 1, CP, pad=PAD)
        e = _eval_inputs(L, torch, s, r)
        t = _dev(torch, T)
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        log0 = _hyper_call(L, torch, s, r, C, pcfg, stream, CSEEDS, t.data_ptr(), it0=0)
        torch.cuda.synchronize()
        r.tr["train_log"] = log0
        _evaluate(L, torch, s, r, e, pcfg, stream)
        torch.cuda.synchronize()
        scores = e["scores"].cpu().numpy()
        snaps = [r.member_snapshot(l) for l in range(CP)]
        prank, pparent, ptable = ppo.pbt_plan(scores[:, SLOT], T, generation=0, **PBT)
        o["hand_rank"], o["hand_parent"], o["hand_table"], o["hand_scores"] = prank, pparent, ptable, scores
        hand = []
        for l in range(CP):
            a, d = snaps[l], snaps[pparent[l]]          # the learner's own state, the donor's nets and optimizer
            m = dict(target=a["c.target"], plant_pvec=a["c.pvec"],
                     state={k[3:]: v for k, v in a.items() if k.startswith("st.")},
                     cstate={k[3:]: v for k, v in a.items() if k.startswith("cs.")},
                     adam=d["tr.adam"].copy(), adam_step=d["tr.adam_step"].copy(),
                     best=dict(best_return=a["tr.best_return"], best_weights=a["tr.best_weights"],
                               best_iter=a["tr.best_iter"]),
                     pool=M[l]["pool"], current_k=a["c.current_k"], weights=d["c.weights"].copy(),
                     critic=d["c.critic"].copy(), pcfg=pcfg)
            snap = _single_cfg(L, torch, s, C, m, stream, 1, CSEEDS[l], [_row_cfg(L, ptable[l])], it0=1)
            snap["tr.train_log"] = np.concatenate([a["tr.train_log"], snap["tr.train_log"]])
            hand.append(snap)
        o["hand"] = hand

        # (c) the loop: two generations of one iteration each
        M = _members(L, s, CP, CB)
        H = ppo.population_stack(M)
        from dart_mpc.lmpc import LmpcPolicy
        pols = [LmpcPolicy(CB, weights=m["weights"].copy(), critic_weights=m["critic"].copy(),
                           current_k=m["current_k"].copy()) for m in M]
        hyper = T.copy()
        o["pbt"] = ppo.train_pbt(s, pols, H, hyper, e["x0"], e["targets"], e["pvecs"], ESTEPS, 2, 1, CSEEDS,
                                 fitness_slot=SLOT, steps=CK, rcfg=C["rcfg"], epochs=EPOCHS, mini_batch_size=MB,
                                 pbt=PBT)
        o["pbt_pop"], o["pbt_hyper"], o["pbt_pols"] = H, hyper, pols
    finally:
        s.close()
    return o


def test_cycle_on_one_stream_equals_cycle_by_hand(cycle):
    o = cycle
    print("scores", o["stream_scores"][:, SLOT], "rank", o["stream_rank"], "parent", o["stream_parent"])
    assert _same(o["stream_scores"], o["hand_scores"])
    assert o["stream_rank"].tolist() == o["hand_rank"].tolist()
    assert o["stream_parent"].tolist() == o["hand_parent"].tolist()
    assert int((o["hand_parent"] != np.arange(CP)).sum()) == 1, "k = 1: one child"
    assert _same(o["stream_table"], o["hand_table"]) and not _same(o["stream_table"], o["table"])
    for l in range(CP):
        _assert_same(o["hand"][l], o["stream"][l], f"learner {l}: the cycle by hand against the cycle on one stream")
    assert (o["pads"] == PAD).all()


# Test 8c: train_pbt over two generations = the cycle
def test_train_pbt_equals_the_cycle(cycle):
    from dart_mpc import ppo
    o, res = cycle, cycle["pbt"]
    assert res["rank"][0].tolist() == o["hand_rank"].tolist() and res["parent"][0].tolist() == o["hand_parent"].tolist()
    assert _same(res["hyper"][0], o["hand_table"]) and _same(res["scores"][0], o["hand_scores"])
    for l in range(CP):
        assert _same(res["train_log"][l], o["stream"][l]["tr.train_log"]), f"log rows of learner {l}"
        assert [row["n"] for row in res["rows"][l]] == [CK // EVERY * CB] * 2
    # the second generation's step follows the plan for the final scores, and acts on the cycle's final state
    rank, parent, table = ppo.pbt_plan(res["scores"][1][:, SLOT], res["hyper"][0], generation=1, **PBT)
    assert res["rank"][1].tolist() == rank.tolist() and res["parent"][1].tolist() == parent.tolist()
    assert _same(res["hyper"][1], table) and _same(o["pbt_hyper"], table)
    H, pols = o["pbt_pop"], o["pbt_pols"]
    for l in range(CP):
        d = o["stream"][parent[l]]
        assert _same(pols[l].weights.reshape(-1), d["c.weights"]), l
        assert _same(pols[l].critic_weights.reshape(-1), d["c.critic"]), l
        assert _same(H["adam"][l], d["tr.adam"]) and H["adam_step"][l] == d["tr.adam_step"][0], l
        a = o["stream"][l]
        assert _same(H["state"]["history"][l * CB:(l + 1) * CB], a["st.history"]), l
        assert _same(H["best"]["best_weights"][l], a["tr.best_weights"]), l
