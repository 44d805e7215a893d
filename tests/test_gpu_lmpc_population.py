"""A population of LMPC learners in one device-resident iteration (dart_lmpc_train_pop_dev / dart_lmpc_train_pop;
csrc/lmpc_train.hip and csrc/lmpc_ppo.hip: the *_pop_kernel forms, and the learner index in policy_step_wave,
lmpc_experience_kernel, lmpc_mean_update_kernel and critic_value_kernel).

The reference of every number is the single-learner entry: learner l of a population is, bit for bit, train_dev on
that learner's arrays with its seed.  The learners differ in everything a wrong index could mix up: seeds, initial
actors and critics, instances (disjoint slices of lmpc_batch) and reset-pool rows.  Set-up of test_gpu_lmpc_train.py:
N = 10, B = 5, records every 2nd step, episodes of 12 steps, a reset pool of 2 rows, mini-batches of 16; P = 3, two
iterations.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, NH, EVERY, MB, EPOCHS, P = 5, 10, 2, 16, 2, 3
SEEDS = (11, 7, 2 ** 40 + 3)
HYPER = dict(clip_eps=0.2, vf_coef=0.25, ent_coef=0.01)
NCRIT = 37569


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


def _assert_same(a, b, what, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip), (what, sorted(set(a) ^ set(b)))
    keys = [k for k in a if k not in skip]
    assert len(keys) >= 45, what
    bad = [k for k in keys if not _same(a[k], b[k])]
    assert not bad, (what, bad)


@functools.lru_cache(maxsize=None)
def _nets(l):
    """Learner l's initial actor and critic: its own perturbation of its own PolicyNet."""
    import torch
    from dart_mpc import ppo
    torch.manual_seed(100 + l)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return ppo.pack_weights(net)


def _members(L, s, learners=range(P), timestep=None):
    """One member dict (ppo.population_stack's) per learner: fresh host arrays."""
    from dart_mpc import ppo
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    D = lmpc_batch(1)
    n = D["state"].shape[0]
    assert n >= P * B
    out = []
    for l in learners:
        sl = slice(l * B, (l + 1) * B)
        actor, critic = _nets(l)
        pol = LmpcPolicy(B, weights=actor.copy(), critic_weights=critic.copy(), seed=l)
        idx = (np.arange(2)[:, None] * 7 + np.arange(B)[None] + B + 3 * l + 1) % n
        state = s.loop_state(D["state"][sl], policy=pol)
        if timestep is not None:
            state["timestep"][:] = timestep[sl]
        out.append(dict(target=np.ascontiguousarray(D["target"][sl]), plant_pvec=np.ascontiguousarray(D["pvec"][sl]),
                        state=state, cstate=L.LmpcSolver.collect_state(np.zeros((B, 2))),
                        adam=np.zeros((2, 77317), np.float32), adam_step=np.zeros(1, np.int32), best=ppo.new_best(),
                        pool={k: np.ascontiguousarray(v) for k, v in
                              dict(reset_x=D["state"][idx], reset_target=D["target"][idx], reset_pvec=D["pvec"][idx]).items()},
                        current_k=pol.current_k.copy(), weights=actor.copy(), critic=critic.copy(), pcfg=pol.cfg))
    return out


def _cfgs(L, K):
    return dict(K=K, R=K // EVERY, rcfg=L.reward_config(record_every=EVERY, max_episode_steps=12),
                cfg=L.ppo_config(epochs=EPOCHS, mini_batch_size=MB, **HYPER))


class _Run:
    """Device arrays of one run of `nl` learners (nl = 0: the single entry's layout) from host arrays stacked as
    ppo.population_stack lays them out."""

    def __init__(self, L, torch, host, C, iterations, nl, pad=None):
        K, R = C["K"], C["R"]
        NI = host["target"].shape[0]
        self.nl, self.NI, self.B = nl, NI, NI // max(nl, 1)
        critic = host["critic"]
        if nl and pad is not None:
            critic = critic.copy()
            critic[:, NCRIT:].view(np.int32)[:] = pad
        self.c = _to_dev(torch, dict(target=host["target"], prm=np.tile(L.LMPC_PRM_DEFAULT, (NI, 1)),
                                     pvec=host["plant_pvec"], current_k=host["current_k"], weights=host["weights"],
                                     critic=critic))
        self.st, self.cs = _to_dev(torch, host["state"]), _to_dev(torch, host["cstate"])
        self.lg = _to_dev(torch, L.loop_logs(L.LMPC_LOOP_LOGS, K, NI))
        self.clg = _to_dev(torch, L.loop_logs(L.LMPC_COLLECT_LOGS, K, NI))
        self.rec = _to_dev(torch, L.loop_logs(L.LMPC_COLLECT_REC, R, NI))
        self.pool = _to_dev(torch, host["pool"])
        m = max(nl, 1)
        ws = (L.train_pop_workspace_bytes(nl, self.B, K, EVERY, EPOCHS, MB) if nl
              else L.train_workspace_bytes(NI, K, EVERY, EPOCHS, MB))
        assert ws > 0
        self.tr = dict(adam=_dev(torch, host["adam"]), adam_step=_dev(torch, host["adam_step"]),
                       train_log=torch.full((m, iterations, 12), float("nan"), dtype=torch.float64, device="cuda"),
                       best_return=_dev(torch, host["best"]["best_return"]),
                       best_weights=_dev(torch, host["best"]["best_weights"]),
                       best_iter=_dev(torch, host["best"]["best_iter"]),
                       workspace=torch.zeros(ws, dtype=torch.uint8, device="cuda"))

    def args(self, C, pcfg, tcfg, over=None):
        a = dict(target=self.c["target"].data_ptr(), prm=self.c["prm"].data_ptr(), plant_pvec=self.c["pvec"].data_ptr(),
                 current_k=self.c["current_k"].data_ptr(), weights=self.c["weights"].data_ptr(),
                 critic=self.c["critic"].data_ptr(), state=_ptrs(self.st), cstate=_ptrs(self.cs), logs=_ptrs(self.lg),
                 clogs=_ptrs(self.clg), rec=_ptrs(self.rec), train=_ptrs(self.tr), pcfg=pcfg, rcfg=C["rcfg"],
                 ppo_cfg=C["cfg"], tcfg=tcfg, pool=_ptrs(self.pool))
        a.update(over or {})
        return a

    def train(self, L, s, C, pcfg, stream, iterations, seeds, it0=0, row0=0, steps=None, over=None, P_=None, B_=None):
        tcfg = L.train_config(seed=int(seeds[0]) if not self.nl else 0, iterations=iterations, it0=it0,
                              steps=C["K"] if steps is None else steps)
        a = self.args(C, pcfg, tcfg, over)
        a["train"]["train_log"] += 12 * 8 * row0
        if self.nl:
            # (rows of a chained call: [P][iterations] of this call, so a chained run keeps one log per call)
            L.LmpcSolver.train_pop_dev(s, self.nl if P_ is None else P_, seeds, self.B if B_ is None else B_, 2,
                                       stream=stream, **a)
        else:
            s.train_dev(self.NI, 2, stream=stream, **a)

    def member_snapshot(self, l):
        """Learner l's slice of everything, in the single run's shapes."""
        nl, Bl = max(self.nl, 1), self.B if self.nl else self.NI
        sl = slice(l * Bl, (l + 1) * Bl)
        h = lambda v: v.cpu().numpy()
        out = {"c." + k: h(self.c[k])[sl] for k in ("target", "prm", "pvec", "current_k")}
        out["c.weights"] = h(self.c["weights"]).reshape(nl, -1)[l]
        out["c.critic"] = h(self.c["critic"]).reshape(nl, -1)[l, :NCRIT]
        for g, d in (("st", self.st), ("cs", self.cs)):
            for k, v in d.items():
                out[g + "." + k] = h(v)[sl]
        for g, d in (("lg", self.lg), ("clg", self.clg), ("rec", self.rec)):
            for k, v in d.items():
                out[g + "." + k] = h(v)[:, sl]
        out["tr.adam"] = h(self.tr["adam"]).reshape(nl, 2, -1)[l]
        out["tr.adam_step"] = h(self.tr["adam_step"])[l:l + 1]
        out["tr.train_log"] = h(self.tr["train_log"])[l]
        out["tr.best_return"] = h(self.tr["best_return"])[l:l + 1]
        out["tr.best_weights"] = h(self.tr["best_weights"]).reshape(nl, -1)[l]
        out["tr.best_iter"] = h(self.tr["best_iter"])[l:l + 1]
        return {k: np.ascontiguousarray(v) for k, v in out.items()}

    def pads(self):
        return self.c["critic"].cpu().numpy().reshape(self.nl, -1)[:, NCRIT:].view(np.int32)


PAD = 0x7fc0beef        # a NaN pattern


def _single(L, torch, s, C, m, stream, iterations, seed, it0=0):
    from dart_mpc import ppo
    r = _Run(L, torch, ppo.population_stack([m]) | dict(critic=m["critic"], weights=m["weights"]), C, iterations, 0)
    torch.cuda.synchronize()
    r.train(L, s, C, m["pcfg"], stream, iterations, (seed,), it0=it0)
    torch.cuda.synchronize()
    return r.member_snapshot(0)


def _pop(L, torch, s, C, members, stream, iterations, seeds, calls=None, pad=PAD):
    from dart_mpc import ppo
    r = _Run(L, torch, ppo.population_stack(members), C, iterations, len(members), pad=pad)
    torch.cuda.synchronize()
    if calls is None:
        r.train(L, s, C, members[0]["pcfg"], stream, iterations, seeds)
        torch.cuda.synchronize()
        return r
    # chained calls of one iteration each: every call writes a log of [P][1], gathered into [P][iterations]
    log = torch.full((len(members), iterations, 12), float("nan"), dtype=torch.float64, device="cuda")
    one = torch.full((len(members), 1, 12), float("nan"), dtype=torch.float64, device="cuda")
    r.tr["train_log"] = one
    for it in calls:
        r.train(L, s, C, members[0]["pcfg"], stream, 1, seeds, it0=it)
        torch.cuda.synchronize()
        log[:, it] = one[:, 0]
    r.tr["train_log"] = log
    return r


@pytest.fixture(scope="module")
def runs(L, torch):
    """K = 32 (n = 80 per learner: five mini-batches of 16) and K = 24 (n = 60: the last mini-batch has 12): every
    learner alone through train_dev, and the population; at K = 32 also the population again, chained, with learner
    1's seed changed, with one learner, and through the host entry."""
    from dart_mpc import ppo
    out = {}
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    try:
        for K in (32, 24):
            C = _cfgs(L, K)
            o = dict(C=C)
            o["single"] = [_single(L, torch, s, C, m, stream, 2, SEEDS[l]) for l, m in enumerate(_members(L, s))]
            pop = _pop(L, torch, s, C, _members(L, s), stream, 2, SEEDS)
            o["pop"] = [pop.member_snapshot(l) for l in range(P)]
            o["pads"] = pop.pads()
            if K == 32:
                r = _pop(L, torch, s, C, _members(L, s), stream, 2, SEEDS)
                o["again"] = [r.member_snapshot(l) for l in range(P)]
                r = _pop(L, torch, s, C, _members(L, s), stream, 2, SEEDS, calls=(0, 1))
                o["chained"] = [r.member_snapshot(l) for l in range(P)]
                r = _pop(L, torch, s, C, _members(L, s), stream, 2, (SEEDS[0], 12345, SEEDS[2]))
                o["other_seed"] = [r.member_snapshot(l) for l in range(P)]
                o["other_pads"] = r.pads()
                r = _pop(L, torch, s, C, _members(L, s, [0]), stream, 2, SEEDS[:1])
                o["one"] = r.member_snapshot(0)
                # the host entry, two iterations
                M = _members(L, s)
                H = ppo.population_stack(M)
                pols = _policies(M)
                got = {}
                rows = ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"],
                                            H["adam_step"], H["best"], K, SEEDS, iterations=2, rcfg=C["rcfg"],
                                            pool=H["pool"], epochs=EPOCHS, mini_batch_size=MB, out=got, **HYPER)
                o["host"] = [_host_snapshot(H, pols, got, l) for l in range(P)]
                o["host_rows"] = rows
                # one iteration through the host entry; learner 2 goes on alone
                o["member"] = _member_continues(L, torch, s, C, stream)
            out[K] = o
    finally:
        s.close()
    return out


def _policies(members):
    from dart_mpc.lmpc import LmpcPolicy
    pols = [LmpcPolicy(B, weights=m["weights"].copy(), critic_weights=m["critic"].copy(), current_k=m["current_k"].copy())
            for m in members]
    return pols


def _host_snapshot(H, pols, got, l):
    from dart_mpc import ppo
    m = ppo.population_member(l, P, H)
    sl = slice(l * B, (l + 1) * B)
    out = {"c.target": m["target"], "c.pvec": m["plant_pvec"], "c.current_k": pols[l].current_k,
           "c.weights": pols[l].weights, "c.critic": pols[l].critic_weights, "tr.adam": m["adam"],
           "tr.adam_step": m["adam_step"], "tr.train_log": got["train_log"][l],
           "tr.best_return": m["best"]["best_return"], "tr.best_weights": m["best"]["best_weights"],
           "tr.best_iter": m["best"]["best_iter"]}
    for g, d in (("st", m["state"]), ("cs", m["cstate"])):
        for k, v in d.items():
            out[g + "." + k] = v
    for g, d in (("lg", got["logs"]), ("clg", got["clogs"]), ("rec", got["rec"])):
        for k, v in d.items():
            out[g + "." + k] = v[:, sl]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def _member_continues(L, torch, s, C, stream, l=2):
    """One population iteration (host entry), then learner l alone: its slice through ppo.population_member, its
    training state through a save_checkpoint / load_checkpoint round trip, one train_dev iteration with it0 = 1."""
    import os
    import tempfile
    from dart_mpc import ppo
    M = _members(L, s)
    H = ppo.population_stack(M)
    pols = _policies(M)
    ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"], H["adam_step"],
                         H["best"], C["K"], SEEDS, iterations=1, rcfg=C["rcfg"], pool=H["pool"], epochs=EPOCHS,
                         mini_batch_size=MB, **HYPER)
    m = ppo.population_member(l, P, H)
    st = m["state"]
    with tempfile.TemporaryDirectory() as tmp:
        path = ppo.save_checkpoint(os.path.join(tmp, "member"), pols[l].weights, pols[l].critic_weights, m["adam"],
                                   m["adam_step"], m["best"], 1, st["obs_mean"], st["obs_M2"], st["obs_count"],
                                   st["history"], pols[l].current_k, st["model_params"])
        ck = ppo.load_checkpoint(path)
    assert int(ck["iteration"][0]) == 1
    state = dict(st)
    for k in ("obs_mean", "obs_M2", "obs_count", "history", "model_params"):
        state[k] = ck[k]
    alone = dict(target=m["target"], plant_pvec=m["plant_pvec"], state=state, cstate=m["cstate"], adam=ck["adam"],
                 adam_step=ck["adam_step"], pool=m["pool"], current_k=ck["current_k"], weights=ck["actor"],
                 critic=ck["critic"], pcfg=M[l]["pcfg"],
                 best=dict(best_return=ck["best_return"], best_weights=ck["best_weights"], best_iter=ck["best_iter"]))
    return _single(L, torch, s, C, alone, stream, 1, SEEDS[l], it0=1)


# ------------------------------------------------------------------------------------------------------------------
# Test 1: population = P single runs
@pytest.mark.parametrize("K", [32, 24])
def test_population_equals_single_runs(runs, K):
    o = runs[K]
    n = K // EVERY * B
    for l in range(P):
        a, b = o["single"][l], o["pop"][l]
        log = b["tr.train_log"]
        print(f"K = {K}, learner {l}: rows {np.array2string(log, precision=4)}")
        assert log[:, 0].tolist() == [n, n] and b["cs.nrec"].tolist() == [K // EVERY] * B
        assert log[:, 1].sum() >= 1, "no episode ended"
        assert log[:, 11].sum() >= 1 and b["tr.best_iter"][0] >= 0, "no snapshot taken"
        assert b["tr.adam_step"].tolist() == [2 * EPOCHS * -(-n // MB)]
        _assert_same(a, b, f"learner {l} alone against learner {l} of the population, K = {K}")
    # the learners are different runs
    assert not _same(o["pop"][0]["c.weights"], o["pop"][1]["c.weights"])
    assert not _same(o["pop"][1]["clg.reward"], o["pop"][2]["clg.reward"])
    assert (o["pads"] == PAD).all()


# Test 2: one learner
def test_population_of_one_equals_train_dev(runs):
    o = runs[32]
    _assert_same(o["single"][0], o["one"], "P = 1 against train_dev")


# Test 3: chaining and repeatability
def test_population_chains_and_repeats(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["pop"][l], o["again"][l], f"two runs, learner {l}")
        _assert_same(o["pop"][l], o["chained"][l], f"2 iterations against 1 + 1, learner {l}")


# Test 4: isolation
def test_population_learners_are_isolated(runs):
    o = runs[32]
    for l in (0, 2):
        _assert_same(o["pop"][l], o["other_seed"][l], f"learner {l} with another seed for learner 1")
    a, b = o["pop"][1], o["other_seed"][1]
    for k in ("rec.rec_action", "clg.logp", "clg.reward", "c.weights", "c.critic", "tr.adam", "st.model_params",
              "tr.train_log"):
        assert not _same(a[k], b[k]), k
    assert (o["pads"] == PAD).all() and (o["other_pads"] == PAD).all()


# Test 5: host entry = device entry
def test_population_host_entry_equals_device_entry(runs):
    o = runs[32]
    for l in range(P):
        _assert_same(o["pop"][l], o["host"][l], f"host entry against device entry, learner {l}", skip=("c.prm",))
        rows = o["host_rows"][l]
        assert [r["snapshot"] for r in rows] == o["pop"][l]["tr.train_log"][:, 11].tolist()


# Test 6: a member continues alone
def test_member_continues_alone(runs):
    o = runs[32]
    want, got = o["pop"][2], o["member"]
    # (the continued run's logs and records are its one iteration's = the population's last; its log has one row)
    _assert_same({k: (v[1:] if k == "tr.train_log" else v) for k, v in want.items()}, got,
                 "learner 2 continued alone against learner 2 of the population")


# Test 7: refusals
def test_population_refusals(L, torch):
    from dart_mpc import ppo
    C = _cfgs(L, 32)
    s = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    small = L.LmpcSolver(N=NH, Ts=0.002, B_max=P * B - 1)
    rm = L.RmpcSolver(N=NH, Ts=0.002, B_max=P * B)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        M = _members(L, s)
        pcfg = M[0]["pcfg"]
        r = _Run(L, torch, ppo.population_stack(M), C, 1, P)
        r.tr["workspace"].fill_(0xA5)
        r.cs["nrec"].fill_(-3)
        torch.cuda.synchronize()
        before = r.member_snapshot(1)
        many = tuple(range(L.POP_MAX + 1))
        cases = [("P = 0", s, dict(P_=0, seeds=())), ("P = POP_MAX + 1", s, dict(P_=L.POP_MAX + 1, seeds=many, B_=1)),
                 ("P B = B_max + 1", small, dict(seeds=SEEDS)), ("null seeds", s, dict(seeds=None)),
                 ("critic off by 4 bytes", s, dict(seeds=SEEDS, over=dict(critic=r.c["critic"].data_ptr() + 4))),
                 ("weights off by 4 bytes", s, dict(seeds=SEEDS, over=dict(weights=r.c["weights"].data_ptr() + 4))),
                 ("K = 25", s, dict(seeds=SEEDS, steps=25)), ("an RMPC handle", rm, dict(seeds=SEEDS))]
        for what, solver, kw in cases:
            seeds = kw.pop("seeds")
            with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                r.train(L, solver, C, pcfg, stream, 1, seeds, **kw)
            torch.cuda.synchronize()
            _assert_same(before, r.member_snapshot(1), what)
            assert bool((r.tr["workspace"] == 0xA5).all()), what     # nothing was launched
            print("refused:", what)
        # the same two pointers through the entry with the global buffer (here without one)
        for name in ("weights", "critic"):
            tcfg = L.train_config(iterations=1, steps=C["K"])
            a = r.args(C, pcfg, tcfg, {name: r.c[name].data_ptr() + 4})
            with pytest.raises(L.DartMPCError, match=r"\(-1\)"):
                s.train_pop_global_dev(P, SEEDS, B, 2, gbuf=None, stream=stream, **a)
            torch.cuda.synchronize()
            _assert_same(before, r.member_snapshot(1), name)
            assert bool((r.tr["workspace"] == 0xA5).all()), name
        assert L.train_pop_workspace_bytes(P, B, 25, EVERY, EPOCHS, MB) == 0
        # the host entry: one instance's timestep advanced
        ts = np.zeros(P * B, np.int32)
        ts[7] = 1
        M = _members(L, s, timestep=ts)
        H = ppo.population_stack(M)
        pols = _policies(M)
        w0 = [p.weights.copy() for p in pols]
        with pytest.raises(L.DartMPCError, match=r"\(-1\).*timestep"):
            ppo.train_population(s, pols, H["target"], H["plant_pvec"], H["state"], H["cstate"], H["adam"],
                                 H["adam_step"], H["best"], 32, SEEDS, rcfg=C["rcfg"], pool=H["pool"], epochs=EPOCHS,
                                 mini_batch_size=MB, **HYPER)
        assert H["adam_step"].tolist() == [0] * P and all(_same(a, p.weights) for a, p in zip(w0, pols))
    finally:
        s.close()
        small.close()
        rm.close()
