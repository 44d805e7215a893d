"""The PPO update of the LMPC policy on the device (csrc/lmpc_ppo.hip: ppo_prepare_kernel, ppo_grad_kernel,
ppo_apply_kernel, critic_value_kernel; dart_lmpc_ppo_* and dart_lmpc_critic_value(_dev)).

The reference is an fp64 torch restatement of rlmpc2.py:783-819 written below (PolicyNet.double(), autograd,
clip_grad_norm_, torch.optim.Adam); the yardstick is the fp32 torch path the package had before,
dart_mpc.ppo.ppo_update and fp32 autograd on the CPU.  For a quantity q, e32(q) = |q_fp32torch - q_fp64| / |q_fp64|;
the kernel's error against fp64 may be at most max(4 e32(q), 64 * 2^-24): the kernel and fp32 torch incur the same
fp32 roundings in another summation order, and the floor is fp32 summation over one mini-batch (e32 of a small
group such as log_std can be tiny by accident).

Measured on one MI355X (every test prints its figures before it asserts, pytest -s); the largest over both batches
and M = 64, 22, 16, 1, 80 of the kernel's relative error against fp64, of e32, and of their ratio case by case:
  gradient, actor matrices and biases   l2 7.9e-6 (e32 5.4e-5, ratio <= 0.28)   max 7.8e-6 (5.4e-5, <= 0.31)
  gradient, log_std                     l2 7.0e-6 (e32 6.7e-5, ratio <= 0.22)   max 5.8e-6 (6.7e-5, <= 0.21)
  gradient, critic                      l2 5.5e-7 (e32 6.9e-7, ratio <= 1.09)   max 6.0e-7 (7.2e-7, <= 1.54)
  policy loss 1.4e-5 (e32 6.8e-5, ratio <= 2.54), value loss 7.0e-7 (7.0e-7, <= 1.00), entropy 1.2e-7 (2.0e-7,
  <= 3.12, under the floor), gradient norm 3.5e-6 (5.4e-5, <= 0.83); the worst case stands at 0.63 of its bar.
  The actor's forward sums run in fp64 (csrc/lmpc_ppo.hip, fwd_layer): with fp32 sums the actor's gradient stood at
  1.7 e32 and the gradient norm missed its bar at M = 80 (4.1e-6 against 3.8e-6, e32 6.8e-7).
  Whole update, 24 steps: rms(dk) 3.0e-7 against rms(d32) 1.4e-6, max |dk| 3.4e-6 against max |d32| 1.7e-5, movement
  7.2e-3; mean losses within 0.25 e32.  Normalised inputs: equal to numpy's / torch's to the last bit.
  critic_value: max |dvalue| 8.6e-7.
"""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = 64 * 2.0 ** -24
N, MB = 150, 64
GROUPS = {"actor": slice(0, 39714), "log_std": slice(39714, 39748), "critic": slice(39748, 77317)}
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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _batch(kind):
    """The benign and the edge batch of n = 150 samples: a perturbed net with non-zero biases, standard normal
    observations whose last 52 columns are zero (a padded history), actions drawn from the net, old_logp the net's
    log-probability plus noise, adv ~ N(0, 2), ret ~ N(5, 3)."""
    import torch
    from torch.distributions import Normal
    from dart_mpc import ppo
    torch.manual_seed(0)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
        if kind == "edge":
            net.log_std[0] = float(np.log(3.0)); net.log_std[1] = float(np.log(5e-3))
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(N, 520, generator=g); obs[:, 468:] = 0.0
    with torch.no_grad():
        mean, std, _ = net(obs)
        act = mean + std * torch.randn(N, 34, generator=g)
        logp = Normal(mean, std).log_prob(act).sum(-1) + (0.25 if kind == "edge" else 0.15) * torch.randn(N, generator=g)
    adv = 2.0 * torch.randn(N, generator=g, dtype=torch.float64)
    ret = 5.0 + 3.0 * torch.randn(N, generator=g, dtype=torch.float64)
    # normalised as ppo_update does (:783 numpy fp64 population std, :790 torch fp32 unbiased std)
    ret64 = ret.numpy()
    ret_n = torch.as_tensor((ret64 - ret64.mean()) / (ret64.std() + 1e-8), dtype=torch.float32)
    adv32 = adv.to(torch.float32)
    adv_n = (adv32 - adv32.mean()) / (adv32.std() + 1e-8)
    actor, critic = ppo.pack_weights(net)
    return dict(net=net, obs=obs, act=act, logp=logp, adv=adv.numpy(), ret=ret64, adv_n=adv_n, ret_n=ret_n,
                actor=actor, critic=critic, sample=np.arange(N, dtype=np.int32),
                perms=ppo.make_perms(N, 8, torch.Generator().manual_seed(7)))


def _loss(net, obs, act, old_logp, adv_n, ret_n):
    """:800-815 on one mini-batch, in the dtype of the net."""
    import torch
    from torch.distributions import Normal
    mean, std, val = net(obs)
    dist = Normal(mean, torch.clamp(std, min=1e-6))
    ratio = torch.exp(dist.log_prob(act).sum(-1) - old_logp)
    surr1 = ratio * adv_n
    surr2 = torch.clamp(ratio, 1.0 - HYPER["clip_eps"], 1.0 + HYPER["clip_eps"]) * adv_n
    policy_loss = -torch.min(surr1, surr2).mean()
    value_loss = torch.nn.functional.mse_loss(val, ret_n)
    entropy = dist.entropy().sum(-1).mean()
    clipped = float(((ratio < 1 - HYPER["clip_eps"]) | (ratio > 1 + HYPER["clip_eps"])).double().mean())
    return policy_loss + HYPER["vf_coef"] * value_loss - HYPER["ent_coef"] * entropy, (policy_loss, value_loss, entropy), clipped


def _torch_grad(kind, idx, dtype):
    """(packed gradient, [policy loss, value loss, entropy, gradient norm], clipped fraction) by autograd."""
    import torch
    from dart_mpc import ppo
    b = _batch(kind)
    net = copy.deepcopy(b["net"]).to(dtype)
    ix = torch.as_tensor(np.asarray(idx, np.int64))
    c = lambda t: t[ix].to(dtype)
    loss, terms, clipped = _loss(net, c(b["obs"]), c(b["act"]), c(b["logp"]), c(b["adv_n"]), c(b["ret_n"]))
    loss.backward()
    g = ppo.pack_grads(net, np.float64)
    return g, np.array([float(t.detach()) for t in terms] + [float(np.sqrt(np.sum(g * g)))]), clipped


def _within(name, got, ref64, ref32, norms=("l2", "max")):
    """|got - ref64| <= max(4 e32, FLOOR) |ref64| in the l2 and the max norm; prints the figures first."""
    got, ref64, ref32 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, ref64, ref32))
    ok = True
    for nm in norms:
        f = (lambda v: float(np.sqrt(np.sum(v * v)))) if nm == "l2" else (lambda v: float(np.max(np.abs(v))))
        scale = f(ref64)
        if scale == 0.0:
            print(f"  {name} {nm}: reference is zero, kernel {f(got):.3e}")
            ok &= f(got) == 0.0
            continue
        e32, ek = f(ref32 - ref64) / scale, f(got - ref64) / scale
        print(f"  {name} {nm}: kernel {ek:.3e}  e32 {e32:.3e}  bar {max(4 * e32, FLOOR):.3e}")
        ok &= ek <= max(4 * e32, FLOOR)
    return ok


# ------------------------------------------------------------------------------------------------------------------
# Test 1: the gradient of one mini-batch
@pytest.mark.parametrize("M", [64, 22, 16, 1, 80])
@pytest.mark.parametrize("kind", ["benign", "edge"])
def test_grad_matches_fp64_autograd(L, torch, kind, M):
    """Measured on one MI355X: the module docstring's table."""
    b = _batch(kind)
    idx = b["perms"][0][:M]
    g64, t64, clipped = _torch_grad(kind, idx, torch.float64)
    g32, t32, _ = _torch_grad(kind, idx, torch.float32)
    cfg = L.ppo_config(**HYPER)
    g, terms = L.ppo_grad(cfg, b["sample"], idx, b["obs"].numpy(), b["act"].numpy(), b["logp"].numpy(), b["adv"], b["ret"],
                          b["actor"], b["critic"])
    print(f"{kind} M = {M}: {100 * clipped:.1f} % of the ratios outside the clip range, |g| = {t64[3]:.3e}")
    assert g.shape == (77317,) and g.dtype == np.float32 and np.isfinite(g).all()
    ok = True
    for name, sl in GROUPS.items():
        ok &= _within(name, g[sl], g64[sl], g32[sl])
    for i, name in enumerate(("policy loss", "value loss", "entropy", "gradient norm")):
        ok &= _within(name, terms[i], t64[i], t32[i], norms=("max",))
    assert ok
    # the rows of W1 and V1 that meet a zero observation column get exactly no gradient
    assert not g[468 * 64:520 * 64].any() and not g[39748 + 468 * 64:39748 + 520 * 64].any()
    assert g[:468 * 64].any() and g[39748:39748 + 468 * 64].any()
    if kind == "edge":          # log_std strictly outside its clamp range: no gradient, data or entropy
        assert g[39714] == 0.0 and g[39715] == 0.0 and g[39716:39748].all()
        assert g64[39714] == 0.0 and g64[39715] == 0.0
    if M >= 16:
        assert 0.0 < clipped < 1.0          # both branches of the clip occur


# ------------------------------------------------------------------------------------------------------------------
# Test 2: one clip + Adam step
@pytest.mark.parametrize("prior_steps", [0, 5])
@pytest.mark.parametrize("scaled", [False, True])
def test_apply_matches_torch_clip_and_adam(L, torch, prior_steps, scaled):
    """A gradient from fp32 torch into clip_grad_norm_ + Adam.step() (fp32, CPU) and into ppo_apply.  Bars from the
    update's elementwise operations plus a 1e-6 relative difference in the summation order of the norm: m and v
    within 1e-5 relative + 1e-12, |dw| <= 1e-5 lr + 2^-23 |w|, the step counter equal.

    The five prior steps apply the same gradient that is fed afterwards.  A bar relative to the result presumes
    that the update does not cancel: m + 0.1 (g - m) does wherever g is near -9 m, and there a last-bit difference
    of the clip coefficient (the norm is summed in another order than torch sums it) comes out arbitrarily large
    relative to m -- two correct fp32 implementations part by more than 1e-5 on such entries.  Measured on one
    MI355X with prior steps that recompute the gradient after every step instead (signs of small entries flip):
    with the clip inactive every m, v and w equal torch's bit for bit (the kernel places Adam's roundings as torch's
    CPU kernel does); with the clip active the worst m exceeds its bar by 1.4e-10 absolute, every v and w within.
    With the prior steps used here, measured: every m and v within the bars, max |dw| 3.0e-8."""
    from dart_mpc import ppo
    b = _batch("benign")
    net = copy.deepcopy(b["net"])
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)
    idx = torch.as_tensor(b["perms"][0][:64].astype(np.int64))
    loss, _, _ = _loss(net, b["obs"][idx], b["act"][idx], b["logp"][idx], b["adv_n"][idx], b["ret_n"][idx])
    loss.backward()
    fed = [p.grad.clone() for p in net.parameters()]

    def backward():
        for p, g0 in zip(net.parameters(), fed):
            p.grad = g0.clone()
    for _ in range(prior_steps):
        backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=0.5)
        opt.step()
    backward()
    norm0 = float(np.linalg.norm(ppo.pack_grads(net, np.float64)))
    if scaled:                  # norm 0.1: the clip is inactive
        for p in net.parameters():
            p.grad.mul_(0.1 / norm0)
    g = ppo.pack_grads(net)
    actor, critic = ppo.pack_weights(net)
    adam, step = ppo.pack_adam(net, opt)
    assert step.tolist() == [prior_steps] and (adam.any() == (prior_steps > 0))
    w0 = np.concatenate([actor, critic])
    row = L.ppo_apply(L.ppo_config(), g, actor, critic, adam, step)
    total = float(torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=0.5))
    opt.step()
    ra, rc = ppo.pack_weights(net)
    radam, rstep = ppo.pack_adam(net, opt)
    w, rw = np.concatenate([actor, critic]), np.concatenate([ra, rc])
    dm = np.abs(adam.astype(np.float64) - radam) - 1e-5 * np.abs(radam) - 1e-12
    dw = np.abs(w.astype(np.float64) - rw) - (1e-5 * 3e-4 + 2.0 ** -23 * np.abs(rw))
    print(f"prior steps {prior_steps}, norm {total:.4e} (kernel {row[3]:.4e}): max excess m, v {dm.max():.3e}, "
          f"w {dw.max():.3e}; max |dw| {np.abs(w - rw).max():.3e}, movement {np.abs(rw - w0).max():.3e}")
    assert (total > 0.5) != scaled and abs(row[3] - total) <= 1e-5 * total
    assert step.tolist() == rstep.tolist() == [prior_steps + 1]
    assert dm.max() <= 0.0 and dw.max() <= 0.0
    assert np.abs(rw - w0).max() > 1e-4                  # the step moved the weights


# ------------------------------------------------------------------------------------------------------------------
# Test 3: the update is its launches
class _DevRun:
    """Device copies of a batch and of a fresh training state, and the update on them."""

    def __init__(self, L, torch, b, mb=MB, records=None):
        self.L, self.torch, self.mb = L, torch, mb
        r = records or dict(sample=b["sample"], obs=b["obs"].numpy(), act=b["act"].numpy(), logp=b["logp"].numpy(),
                            adv=b["adv"], ret=b["ret"])
        self.n, self.total = int(np.asarray(r["sample"]).size), int(np.asarray(r["logp"]).size)
        self.d = {k: _dev(torch, v) for k, v in r.items()}
        self.w, self.c = _dev(torch, b["actor"]), _dev(torch, b["critic"])
        self.adam = torch.zeros(2, 77317, dtype=torch.float32, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ws = torch.zeros(L.ppo_workspace_bytes(self.n, mb), dtype=torch.uint8, device="cuda")
        self.stats = torch.zeros(3, dtype=torch.float64, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def update(self, perms):
        perms = np.ascontiguousarray(perms, np.int32)
        steps = perms.shape[0] * (-(-self.n // self.mb))
        log = self.torch.full((steps, 4), float("nan"), dtype=self.torch.float32, device="cuda")
        d, p = self.d, _dev(self.torch, perms)
        cfg = self.L.ppo_config(epochs=perms.shape[0], mini_batch_size=self.mb, **HYPER)
        self.L.ppo_update_dev(cfg, self.n, self.total, d["sample"].data_ptr(), p.data_ptr(), d["obs"].data_ptr(),
                              d["act"].data_ptr(), d["logp"].data_ptr(), d["adv"].data_ptr(), d["ret"].data_ptr(),
                              self.w.data_ptr(), self.c.data_ptr(), self.adam.data_ptr(), self.step.data_ptr(),
                              self.stats.data_ptr(), self.ws.data_ptr(), step_log=log.data_ptr(), stream=self.stream)
        self.torch.cuda.synchronize()
        return log.cpu().numpy()

    def one_by_one(self, perms):
        L, d, t = self.L, self.d, self.torch
        perms = np.ascontiguousarray(perms, np.int32)
        p = _dev(t, perms)
        steps = perms.shape[0] * (-(-self.n // self.mb))
        log = t.full((steps, 4), float("nan"), dtype=t.float32, device="cuda")
        grad, terms = t.empty(77317, dtype=t.float32, device="cuda"), t.empty(4, dtype=t.float32, device="cuda")
        cfg = L.ppo_config(epochs=perms.shape[0], mini_batch_size=self.mb, **HYPER)
        L.ppo_prepare_dev(self.n, self.total, d["sample"].data_ptr(), d["adv"].data_ptr(), d["ret"].data_ptr(),
                          self.ws.data_ptr(), stream=self.stream)
        k = 0
        for e in range(perms.shape[0]):
            for start in range(0, self.n, self.mb):
                M = min(self.mb, self.n - start)
                L.ppo_grad_dev(cfg, self.n, self.total, M, d["sample"].data_ptr(), p.data_ptr() + 4 * (e * self.n + start),
                               d["obs"].data_ptr(), d["act"].data_ptr(), d["logp"].data_ptr(), self.w.data_ptr(),
                               self.c.data_ptr(), grad.data_ptr(), terms.data_ptr(), self.ws.data_ptr(), stream=self.stream)
                L.ppo_apply_dev(cfg, grad.data_ptr(), self.w.data_ptr(), self.c.data_ptr(), self.adam.data_ptr(),
                                self.step.data_ptr(), self.ws.data_ptr(), terms=terms.data_ptr(),
                                stats=self.stats.data_ptr(), step_log=log.data_ptr(), step_in_call=k, stream=self.stream)
                k += 1
        t.cuda.synchronize()
        return log.cpu().numpy()

    def state(self):
        return dict(w=self.w.cpu().numpy(), c=self.c.cpu().numpy(), adam=self.adam.cpu().numpy(),
                    step=self.step.cpu().numpy(), stats=self.stats.cpu().numpy())


def _same_state(a, b, names=("w", "c", "adam", "step")):
    for k in names:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_update_is_its_launches(L, torch):
    b = _batch("benign")
    whole = _DevRun(L, torch, b)
    log = whole.update(b["perms"])
    assert log.shape == (24, 4) and np.isfinite(log).all() and whole.state()["step"].tolist() == [24]
    seq = _DevRun(L, torch, b)
    log_seq = seq.one_by_one(b["perms"])
    _same_state(whole.state(), seq.state(), ("w", "c", "adam", "step", "stats"))
    assert np.array_equal(_bits(log), _bits(log_seq))
    # 3 epochs, then 5 with the Adam state carried over = 8
    split = _DevRun(L, torch, b)
    log_a, log_b = split.update(b["perms"][:3]), split.update(b["perms"][3:])
    _same_state(whole.state(), split.state())
    assert np.array_equal(_bits(log), _bits(np.concatenate([log_a, log_b])))
    # a second run gives the same bits (no atomics)
    again = _DevRun(L, torch, b)
    log_again = again.update(b["perms"])
    _same_state(whole.state(), again.state(), ("w", "c", "adam", "step", "stats"))
    assert np.array_equal(_bits(log), _bits(log_again))
    # the host entry
    actor, critic = b["actor"].copy(), b["critic"].copy()
    adam, step = np.zeros((2, 77317), np.float32), np.zeros(1, np.int32)
    out = L.ppo_update(L.ppo_config(**HYPER), b["sample"], b["perms"], b["obs"].numpy(), b["act"].numpy(),
                       b["logp"].numpy(), b["adv"], b["ret"], actor, critic, adam, step)
    _same_state(whole.state(), dict(w=actor, c=critic, adam=adam, step=step))
    assert np.array_equal(_bits(log), _bits(out["step_log"]))
    assert [out["policy_loss"], out["value_loss"], out["entropy"]] == whole.state()["stats"].tolist()
    assert np.abs(actor - b["actor"]).max() > 1e-4 and np.abs(critic - b["critic"]).max() > 1e-4


# ------------------------------------------------------------------------------------------------------------------
# Tests 4, 5: the whole update against the fp64 restatement; the normalisation
@functools.lru_cache(maxsize=None)
def _whole_update():
    import torch
    from dart_mpc import _lib, ppo
    b = _batch("benign")
    batch = dict(obs=b["obs"].numpy(), action=b["act"].numpy(), logp=b["logp"].numpy(), adv=b["adv"], ret=b["ret"])
    # fp32 torch: the path the package had (the generator draws the permutations make_perms drew)
    net32 = copy.deepcopy(b["net"])
    opt32 = torch.optim.Adam(net32.parameters(), lr=3e-4, weight_decay=1e-5)
    s32 = ppo.ppo_update(net32, opt32, batch, generator=torch.Generator().manual_seed(7), **HYPER)
    # fp64 restatement of :783-819 on the same normalised inputs and permutations
    net64 = copy.deepcopy(b["net"]).double()
    opt64 = torch.optim.Adam(net64.parameters(), lr=3e-4, weight_decay=1e-5)
    c = lambda t: t.double()
    obs, act, logp, adv_n, ret_n = c(b["obs"]), c(b["act"]), c(b["logp"]), c(b["adv_n"]), c(b["ret_n"])
    s64 = np.zeros(3)
    for perm in b["perms"]:
        for start in range(0, N, MB):
            ix = torch.as_tensor(perm[start:start + MB].astype(np.int64))
            loss, terms, _ = _loss(net64, obs[ix], act[ix], logp[ix], adv_n[ix], ret_n[ix])
            opt64.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net64.parameters(), max_norm=0.5)
            opt64.step()
            s64 += [float(t.detach()) for t in terms]
    s64 /= 24
    actor, critic = b["actor"].copy(), b["critic"].copy()
    adam, step = np.zeros((2, 77317), np.float32), np.zeros(1, np.int32)
    out = ppo.ppo_update_device(actor, critic, adam, step, dict(rec_obs=batch["obs"], rec_action=batch["action"],
                                                                rec_logp=batch["logp"]), b["sample"], b["adv"], b["ret"],
                                b["perms"], **HYPER)
    raw = _lib.ppo_update(_lib.ppo_config(epochs=1, **HYPER), b["sample"], b["perms"][:1], batch["obs"], batch["action"],
                          batch["logp"], b["adv"], b["ret"], b["actor"].copy(), b["critic"].copy(), adam.copy(), step.copy())
    pk = lambda net: np.concatenate([a.astype(np.float64) for a in _pack64(net)])
    return dict(w0=np.concatenate([b["actor"], b["critic"]]).astype(np.float64), w32=pk(net32), w64=pk(net64),
                wk=np.concatenate([actor, critic]).astype(np.float64), s32=s32, s64=s64, sk=out, step=step,
                adv_norm=raw["adv_norm"], ret_norm=raw["ret_norm"])


def _pack64(net):
    from dart_mpc import ppo
    return [(p.detach().numpy().T if tr else p.detach().numpy()).reshape(-1) for p, tr in ppo._packed_params(net)]


def test_whole_update_against_fp64_restatement():
    """Benign batch, 8 epochs, 24 steps.  Measured on one MI355X: rms(dk) 3.0e-7 <= 4 x 1.4e-6, max |dk| 3.4e-6 <=
    8 x 1.7e-5, max |d32| / movement 2.4e-3."""
    r = _whole_update()
    d32, dk, move = r["w32"] - r["w64"], r["wk"] - r["w64"], r["w64"] - r["w0"]
    rms = lambda v: float(np.sqrt(np.mean(v * v)))
    print(f"rms: kernel {rms(dk):.3e} fp32 torch {rms(d32):.3e}; max: kernel {np.abs(dk).max():.3e} "
          f"fp32 torch {np.abs(d32).max():.3e}; movement {np.abs(move).max():.3e}")
    ok = True
    for i, name in enumerate(("policy_loss", "value_loss", "entropy")):
        ok &= _within("mean " + name, r["sk"][name], r["s64"][i], r["s32"][name], norms=("max",))
    assert r["step"].tolist() == [24]
    assert np.abs(d32).max() <= 1e-2 * np.abs(move).max()       # the comparison is meaningful
    assert rms(dk) <= 4 * rms(d32)
    assert np.abs(dk).max() <= 8 * np.abs(d32).max()
    assert ok


def test_normalisation_matches_numpy_and_torch():
    b, r = _batch("benign"), _whole_update()
    for name, got, ref in (("adv", r["adv_norm"], b["adv_n"].numpy()), ("ret", r["ret_norm"], b["ret_n"].numpy())):
        err = float(np.max(np.abs(got.astype(np.float64) - ref))) / float(np.max(np.abs(ref)))
        print(f"{name}_norm: {err:.3e} of the largest entry")
        assert got.dtype == np.float32 and err <= 1e-6


# ------------------------------------------------------------------------------------------------------------------
# Test 6: ragged records
@pytest.mark.parametrize("mb", [64, 8])
def test_ragged_records_equal_compacted(L, torch, mb):
    """Record arrays [9][5 + 2] with NaN wherever row >= nrec[b] and in two guard instances past the batch: the
    update on the 21 samples the mask names equals, bit for bit, the update on them compacted."""
    from dart_mpc import ppo
    b = _batch("benign")
    rows, cols = 9, 7
    nrec = np.array([0, 1, 9, 4, 7, 0, 0])
    m = np.arange(rows)[:, None] < nrec[None]
    sample = np.flatnonzero(m.reshape(-1)).astype(np.int32)        # row-major, the order rec[m] gives
    n = sample.size
    assert n == 21
    take = np.arange(n) * 7 % N                                      # 21 samples of the batch
    full = lambda a, dt: np.full((rows * cols,) + a.shape[1:], np.nan, dt)
    src = dict(obs=b["obs"].numpy()[take], act=b["act"].numpy()[take], logp=b["logp"].numpy()[take], adv=b["adv"][take],
               ret=b["ret"][take])
    ragged = {k: full(v, v.dtype) for k, v in src.items()}
    for k, v in src.items():
        ragged[k][sample] = v
    assert all(np.isnan(v).any() for v in ragged.values())
    perms = ppo.make_perms(n, 8, torch.Generator().manual_seed(3))
    a = _DevRun(L, torch, b, mb=mb, records=dict(sample=sample, **ragged))
    log_a = a.update(perms)
    c = _DevRun(L, torch, b, mb=mb, records=dict(sample=np.arange(n, dtype=np.int32), **src))
    log_c = c.update(perms)
    assert log_a.shape == (8 * (-(-n // mb)), 4) and np.isfinite(log_a).all()
    _same_state(a.state(), c.state(), ("w", "c", "adam", "step", "stats"))
    assert np.array_equal(_bits(log_a), _bits(log_c))
    st = a.state()
    assert np.isfinite(st["w"]).all() and np.isfinite(st["c"]).all() and np.isfinite(st["adam"]).all()
    assert np.abs(st["w"] - b["actor"]).max() > 1e-4
    # the host entry compacts while it stages: the same bits again
    actor, critic = b["actor"].copy(), b["critic"].copy()
    adam, step = np.zeros((2, 77317), np.float32), np.zeros(1, np.int32)
    L.ppo_update(L.ppo_config(mini_batch_size=mb, **HYPER), sample, perms, ragged["obs"], ragged["act"], ragged["logp"],
                 ragged["adv"], ragged["ret"], actor, critic, adam, step)
    _same_state(st, dict(w=actor, c=critic, adam=adam, step=step))


# ------------------------------------------------------------------------------------------------------------------
# Test 7: the critic's forward pass
@pytest.mark.parametrize("n", [1, 5, 67])
def test_critic_value_matches_numpy(L, torch, n):
    from dart_mpc import harness
    b = _batch("benign")
    obs = np.random.default_rng(n).standard_normal((n, 520)).astype(np.float32)
    ref = harness.lmpc_critic_value(b["critic"], obs)
    got = L.critic_value(b["critic"], obs)
    print(f"n = {n}: max |dvalue| {float(np.max(np.abs(got - ref))):.3e}")
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5)
    d_obs, d_c = _dev(torch, obs), _dev(torch, b["critic"])
    out = torch.full((n + 3,), float("nan"), dtype=torch.float32, device="cuda")
    L.critic_value_dev(n, d_c.data_ptr(), d_obs.data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.array_equal(_bits(out[:n]), _bits(got)) and np.isnan(out[n:]).all()


# ------------------------------------------------------------------------------------------------------------------
# Test 8: collect -> critic value -> GAE -> update -> collect on device pointers
def test_training_cycle_on_device_pointers(L, torch):
    from dart_mpc import harness, ppo
    from dart_mpc.lmpc import LmpcPolicy
    from dart_mpc.workload import lmpc_batch
    B, K, every = 5, 32, 2
    rec_rows = K // every
    b = _batch("benign")
    D = lmpc_batch(1)
    pol = LmpcPolicy(B, weights=b["actor"], critic_weights=b["critic"])
    rcfg = L.reward_config(record_every=every, max_episode_steps=1000)
    dev = lambda arrays: {k: _dev(torch, v) for k, v in arrays.items()}
    ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()}
    s = L.LmpcSolver(N=10, Ts=0.002, B_max=B)
    try:
        c = dev(dict(target=D["target"][:B], prm=np.tile(L.LMPC_PRM_DEFAULT, (B, 1)), pvec=D["pvec"][:B],
                     current_k=pol.current_k, weights=b["actor"], critic=b["critic"],
                     noise=np.random.default_rng(2).standard_normal((2 * K, B, 34)).astype(np.float32)))
        st = dev(s.loop_state(D["state"][:B], policy=pol))
        cs = dev(L.LmpcSolver.collect_state(np.zeros((B, 2))))
        lg, clg = dev(L.loop_logs(L.LMPC_LOOP_LOGS, 2 * K, B)), dev(L.loop_logs(L.LMPC_COLLECT_LOGS, 2 * K, B))
        rec = dev(L.loop_logs(L.LMPC_COLLECT_REC, rec_rows, B))
        stream = torch.cuda.current_stream().cuda_stream

        def collect(k0, steps):
            torch.cuda.synchronize()                            # (the handle launches on its own stream)
            s.collect_dev(B, k0, steps, 2 * K, rec_rows, 0, c["target"].data_ptr(), c["prm"].data_ptr(),
                          c["pvec"].data_ptr(), ptrs(st), ptrs(cs), ptrs(lg), ptrs(clg), ptrs(rec), pol.cfg, rcfg,
                          c["weights"].data_ptr(), c["critic"].data_ptr(), c["current_k"].data_ptr(),
                          noise=c["noise"].data_ptr())
            s.sync()
        collect(0, K)
        last_value = torch.empty(B, dtype=torch.float32, device="cuda")
        L.critic_value_dev(B, c["critic"].data_ptr(), st["history"].data_ptr(), last_value.data_ptr(), stream=stream)
        adv = torch.full((rec_rows, B), float("nan"), dtype=torch.float64, device="cuda")
        ret = torch.full_like(adv, float("nan"))
        rc = L.lib().dart_lmpc_gae_dev(B, rec_rows, 0.99, 0.95, cs["nrec"].data_ptr(), rec["rec_reward"].data_ptr(),
                                       rec["rec_value"].data_ptr(), rec["rec_done"].data_ptr(), last_value.data_ptr(),
                                       adv.data_ptr(), ret.data_ptr(), stream)
        assert rc == 0
        # (the sample list is the one thing the host decides: which records exist; every instance recorded every row)
        n = rec_rows * B
        torch.cuda.synchronize()
        assert cs["nrec"].cpu().tolist() == [rec_rows] * B
        sample = _dev(torch, np.arange(n, dtype=np.int32))
        perms = _dev(torch, ppo.make_perms(n, 2, torch.Generator().manual_seed(1)))
        cfg = L.ppo_config(epochs=2, mini_batch_size=16, **HYPER)
        adam = torch.zeros(2, 77317, dtype=torch.float32, device="cuda")
        step = torch.zeros(1, dtype=torch.int32, device="cuda")
        stats = torch.zeros(3, dtype=torch.float64, device="cuda")
        ws = torch.zeros(L.ppo_workspace_bytes(n, 16), dtype=torch.uint8, device="cuda")
        L.ppo_update_dev(cfg, n, n, sample.data_ptr(), perms.data_ptr(), rec["rec_obs"].data_ptr(),
                         rec["rec_action"].data_ptr(), rec["rec_logp"].data_ptr(), adv.data_ptr(), ret.data_ptr(),
                         c["weights"].data_ptr(), c["critic"].data_ptr(), adam.data_ptr(), step.data_ptr(),
                         stats.data_ptr(), ws.data_ptr(), stream=stream)
        cs["nrec"].zero_()
        collect(K, 1)                                           # (one step first: its observation stays in history)
        obs_k = st["history"].cpu().numpy()
        collect(K + 1, K - 1)
        torch.cuda.synchronize()
        w, cw = c["weights"].cpu().numpy(), c["critic"].cpu().numpy()
        assert step.cpu().tolist() == [2 * 5] and np.isfinite(stats.cpu().numpy()).all()
        assert np.isfinite(w).all() and np.isfinite(cw).all()
        assert np.abs(w - b["actor"]).max() > 1e-4 and np.abs(cw - b["critic"]).max() > 1e-4
        status = lg["status"].cpu().numpy()
        assert (status == 0).all(), np.unique(status)
        # the second collection ran on the updated weights: its first values are the numpy critic on them
        got = clg["value"].cpu().numpy()[K]
        ref = harness.lmpc_critic_value(cw, obs_k)
        print(f"max |dvalue| of the second collection's first row: {float(np.max(np.abs(got - ref))):.3e}")
        assert np.max(np.abs(got - ref)) <= 1e-5
    finally:
        s.close()
