"""PPO update of the LMPC parameter policy on collected experience.

Restates the training half of RLMPC._rl_worker (LMPC/src/controller/rlmpc2.py): ``PolicyNet`` is ``Policy``
(:33-80), ``ppo_update`` the clipped-surrogate update of :783-819 in plain torch, ``ppo_update_device`` the same
update as HIP kernels (csrc/lmpc_ppo.hip, ``_lib.ppo_update``) on the packed weights and Adam state in place.  The
torch path is the reference the device path is tested against; ``make_perms`` gives both the same mini-batches.
Experience comes from ``dart_lmpc_collect`` (harness.collect_lmpc) and ``_lib.gae``; ``pack_weights`` /
``load_weights`` and ``pack_adam`` / ``load_adam`` move the weights and Adam's state between the torch objects and
the packed input-major arrays the kernels read.  ``train_device`` runs whole iterations -- noise, collection,
GAE, permutations, update, the mean-based parameter write, log row and best-policy snapshot -- through
``LmpcSolver.train`` (csrc/lmpc_train.hip) without the host in between; with ``global_buffer=new_global_buffer(n)``
the iterations also contain the loop's second update on the global buffer (:823-874).  ``save_checkpoint`` /
``load_checkpoint`` keep a training state, the global buffer included when given, in one ``.npz`` of plain arrays (no
pickle); its fields stand in for the reference's ``best_agent.pth`` / ``latest_agent.pth``, which are not loaded.
A population (``train_population``) may train with one row of hyper-parameters per learner (``hyper_table=``,
``_lib.hyper_table``); ``pbt_plan`` states the exploit/explore step of population-based training in numpy, ``pbt_step``
runs it through the library on host arrays, and ``train_pbt`` chains training, evaluation and the step on one stream
(csrc/lmpc_pbt.hip).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.distributions import Normal

OBS_DIM, HIDDEN, ACT_DIM = 520, 64, 34


class PolicyNet(nn.Module):
    """``Policy`` (:33-80): mean_net 520-64-64-34 and value_net 520-64-64-1 with tanh, log_std [34] clamped in
    ``forward``; orthogonal init with gain sqrt(2), zero bias."""

    def __init__(self, std_init=0.1, std_min=1e-2, std_max=2.0):
        super().__init__()
        self.mean_net = nn.Sequential(nn.Linear(OBS_DIM, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN), nn.Tanh(),
                                      nn.Linear(HIDDEN, ACT_DIM))
        self.value_net = nn.Sequential(nn.Linear(OBS_DIM, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN), nn.Tanh(),
                                       nn.Linear(HIDDEN, 1))
        self.log_std = nn.Parameter(torch.ones(ACT_DIM) * float(np.log(std_init)))
        self.min_log_std, self.max_log_std = float(np.log(std_min)), float(np.log(std_max))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight, gain=float(np.sqrt(2)))
                nn.init.constant_(m.bias, 0.0)

    def forward(self, obs):
        mean = self.mean_net(obs)
        std = torch.exp(torch.clamp(self.log_std, self.min_log_std, self.max_log_std))
        return mean, std, self.value_net(obs).squeeze(-1)


def _linears(seq):
    return [m for m in seq if isinstance(m, nn.Linear)]


def pack_weights(net: PolicyNet):
    """(actor fp32 [39748], critic fp32 [37569]) in the kernels' input-major layout (nn.Linear stores [out, in])."""
    def pack(seq, tail=()):
        parts = []
        for m in _linears(seq):
            parts += [m.weight.detach().cpu().numpy().T, m.bias.detach().cpu().numpy()]
        parts += list(tail)
        return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts]).astype(np.float32)
    return pack(net.mean_net, (net.log_std.detach().cpu().numpy(),)), pack(net.value_net)


def load_weights(net: PolicyNet, actor, critic):
    """Inverse of ``pack_weights``: packed arrays into the module's parameters."""
    def load(seq, w, tail=None):
        w = np.asarray(w, np.float32).reshape(-1)
        o = 0
        with torch.no_grad():
            for m in _linears(seq):
                n_out, n_in = m.weight.shape
                m.weight.copy_(torch.from_numpy(w[o:o + n_in * n_out].reshape(n_in, n_out).T.copy())); o += n_in * n_out
                m.bias.copy_(torch.from_numpy(w[o:o + n_out].copy())); o += n_out
            if tail is not None:
                tail.copy_(torch.from_numpy(w[o:o + tail.numel()].copy())); o += tail.numel()
        if o != w.size:
            raise ValueError(f"packed weights have {w.size} floats, the module takes {o}")
    load(net.mean_net, actor, net.log_std)
    load(net.value_net, critic)
    return net


def _packed_params(net: PolicyNet):
    """The module's parameters in the packed order (actor, then critic) with a flag: stored transposed."""
    out = []
    for m in _linears(net.mean_net):
        out += [(m.weight, True), (m.bias, False)]
    out.append((net.log_std, False))
    for m in _linears(net.value_net):
        out += [(m.weight, True), (m.bias, False)]
    return out


def pack_grads(net: PolicyNet, dtype=np.float32):
    """The parameters' ``.grad`` in the packed order of the device update: [77317]."""
    return np.concatenate([(p.grad.detach().cpu().numpy().T if tr else p.grad.detach().cpu().numpy()).reshape(-1)
                           for p, tr in _packed_params(net)]).astype(dtype)


def pack_adam(net: PolicyNet, optimizer):
    """(adam float32 [2, 77317], step int32 [1]): ``exp_avg``, ``exp_avg_sq`` and ``step`` of a torch Adam in the
    packed order of the device update.  A fresh optimizer (no state yet) packs to zeros."""
    m, v, step = [], [], 0
    for p, tr in _packed_params(net):
        st = optimizer.state.get(p, {})
        for name, parts in (("exp_avg", m), ("exp_avg_sq", v)):
            a = st[name].detach().cpu().numpy() if name in st else np.zeros(tuple(p.shape), np.float32)
            parts.append(np.asarray(a.T if tr else a, np.float32).reshape(-1))
        if "step" in st:
            step = int(st["step"])
    return np.stack([np.concatenate(m), np.concatenate(v)]).astype(np.float32), np.array([step], np.int32)


def load_adam(net: PolicyNet, optimizer, adam, step):
    """Inverse of ``pack_adam``: the packed moments and step count into the optimizer's state."""
    adam = np.asarray(adam, np.float32).reshape(2, -1)
    step = int(np.asarray(step).reshape(-1)[0])
    o = 0
    for p, tr in _packed_params(net):
        st = optimizer.state[p]
        shape = tuple(p.shape[::-1]) if tr else tuple(p.shape)
        for name, row in (("exp_avg", adam[0]), ("exp_avg_sq", adam[1])):
            a = row[o:o + p.numel()].reshape(shape)
            st[name] = torch.from_numpy((a.T if tr else a).copy()).to(p.device)
        st["step"] = torch.tensor(float(step))
        o += p.numel()
    if o != adam.shape[1]:
        raise ValueError(f"packed Adam state has {adam.shape[1]} entries per moment, the module takes {o}")
    return optimizer


def make_perms(n, epochs, generator=None):
    """int32 [epochs, n]: ``torch.randperm(n, generator=generator)`` once per epoch, the draws ``ppo_update`` makes,
    so that the device update can be given the same mini-batches."""
    return np.stack([torch.randperm(int(n), generator=generator).numpy() for _ in range(int(epochs))]).astype(np.int32) \
        if int(epochs) > 0 else np.zeros((0, int(n)), np.int32)


def ppo_update_device(actor, critic, adam, adam_step, records, sample, adv, ret, perms, **hyper):
    """``ppo_update`` on the device (``_lib.ppo_update``: HIP kernels for the normalisation, both nets' forward and
    backward pass, the clip and Adam).  ``actor`` [39748], ``critic`` [37569], ``adam`` [2, 77317] (float32) and
    ``adam_step`` [1] (int32) are updated in place; ``records`` maps rec_obs / rec_action / rec_logp to the record
    arrays [rec_rows, B, ..], ``sample`` [n] holds flat record indices row * B + b, ``adv`` / ``ret`` are the
    float64 [rec_rows, B] arrays of ``_lib.gae``, ``perms`` [epochs, n] comes from ``make_perms``.  ``hyper``
    overrides fields of ``_lib.ppo_config`` (epochs is taken from ``perms``).  Returns the dict ``ppo_update``
    returns."""
    from . import _lib
    perms = np.ascontiguousarray(perms, np.int32).reshape(-1, np.asarray(sample).size)
    cfg = _lib.ppo_config(**dict(hyper, epochs=perms.shape[0]))
    out = _lib.ppo_update(cfg, sample, perms, records["rec_obs"], records["rec_action"], records["rec_logp"], adv, ret,
                          actor, critic, adam, adam_step)
    return dict(policy_loss=out["policy_loss"], value_loss=out["value_loss"], entropy=out["entropy"])


def ppo_update(net, optimizer, batch, clip_eps=0.2, epochs=8, mini_batch_size=64, vf_coef=0.25, ent_coef=0.01,
               max_grad_norm=0.5, generator=None):
    """The clipped-surrogate update of :783-819 on ``batch`` = dict(obs [n, 520], action [n, 34], logp [n], adv [n],
    ret [n]) (arrays or tensors): returns normalised as :783, advantages as :790, ``epochs`` passes over shuffled
    mini-batches (``generator`` seeds the permutations).  Returns the mean policy loss, value loss and entropy."""
    dev = next(net.parameters()).device
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
    ret64 = np.asarray(batch["ret"], np.float64)
    ret = t((ret64 - ret64.mean()) / (ret64.std() + 1e-8))
    obs, act, old_logp, adv = t(batch["obs"]), t(batch["action"]), t(batch["logp"]), t(batch["adv"])
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    n = obs.shape[0]
    stats = np.zeros(3)
    count = 0
    for _ in range(int(epochs)):
        idxs = torch.randperm(n, generator=generator).to(dev)
        for start in range(0, n, int(mini_batch_size)):
            mb = idxs[start:start + int(mini_batch_size)]
            mean, std, val = net(obs[mb])
            dist = Normal(mean, torch.clamp(std, min=1e-6))
            logp = dist.log_prob(act[mb]).sum(-1)
            ratio = torch.exp(logp - old_logp[mb])
            surr1 = ratio * adv[mb]
            surr2 = torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv[mb]
            policy_loss = -torch.min(surr1, surr2).mean()
            value_loss = nn.functional.mse_loss(val, ret[mb])
            entropy = dist.entropy().sum(-1).mean()
            loss = policy_loss + vf_coef * value_loss - ent_coef * entropy
            optimizer.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(net.parameters(), max_norm=max_grad_norm)
            optimizer.step()
            stats += [policy_loss.item(), value_loss.item(), entropy.item()]
            count += 1
    stats /= max(count, 1)
    return dict(policy_loss=stats[0], value_loss=stats[1], entropy=stats[2])


def train_device(solver, policy, target, plant_pvec, state, cstate, adam, adam_step, best, steps, iterations=1, it0=0,
                 seed=0, rcfg=None, pool=None, prm=None, gamma=0.99, lam=0.95, mean_update=True, track_best=True,
                 epochs=8, mini_batch_size=64, out=None, global_buffer=None, **hyper):
    """``iterations`` complete PPO iterations of ``steps`` closed-loop steps on the device (``LmpcSolver.train``): the
    exploration noise and the mini-batch permutations come from the device generator of (``seed``, iteration index
    ``it0`` ..), nothing passes through the host between the steps of an iteration or between iterations.  Updated
    in place: ``target``, ``plant_pvec``, ``state`` (``solver.loop_state``), ``cstate`` (``solver.collect_state``),
    ``policy.weights`` / ``critic_weights`` / ``current_k``, ``adam`` [2, 77317], ``adam_step`` [1] and ``best`` =
    dict(best_return float64 [1] starting at -inf, best_weights float32 [77317], best_iter int32 [1]).  ``hyper``
    overrides fields of ``_lib.ppo_config``.  ``out`` (a dict, optional) receives the last iteration's ``logs``,
    ``clogs`` and ``rec``.  Returns one dict per iteration with the keys of ``_lib.TRAIN_LOG_FIELDS``.

    With ``global_buffer`` (``new_global_buffer(n)``, n = B * steps / record_every) every iteration also runs the
    reference's second update (rlmpc2.py:823-874): a quarter of its records is appended to the buffer, and a buffer
    that holds n records is updated on and cleared, before the parameter write.  The dict is updated in place,
    ``fill`` included, so it carries over to the next call; each returned row gains the keys of
    ``_lib.GLOBAL_LOG_FIELDS``."""
    from . import _lib
    rcfg = rcfg if rcfg is not None else _lib.reward_config()
    B, K = state["x"].shape[0], int(steps)
    cfg = _lib.ppo_config(**dict(hyper, epochs=epochs, mini_batch_size=mini_batch_size))
    tcfg = _lib.train_config(seed=seed, iterations=iterations, it0=it0, steps=K, gamma=gamma, lam=lam,
                             mean_update=int(bool(mean_update)), track_best=int(bool(track_best)))
    R = K // max(int(rcfg.record_every), 1)
    logs, clogs = _lib.loop_logs(_lib.LMPC_LOOP_LOGS, K, B), _lib.loop_logs(_lib.LMPC_COLLECT_LOGS, K, B)
    rec = _lib.loop_logs(_lib.LMPC_COLLECT_REC, R, B)
    train_log = np.full((int(iterations), _lib.TRAIN_LOG_COLS), np.nan)
    global_log = None if global_buffer is None else np.full((int(iterations), _lib.GLOBAL_LOG_COLS), np.nan)
    solver.train(target, plant_pvec, state, cstate, logs, clogs, rec, policy, adam, adam_step, train_log,
                 best["best_return"], best["best_weights"], best["best_iter"], cfg, tcfg, rcfg=rcfg, prm=prm, pool=pool,
                 global_buffer=global_buffer, global_log=global_log)
    if out is not None:
        out.update(logs=logs, clogs=clogs, rec=rec, train_log=train_log)
    rows = [dict(zip(_lib.TRAIN_LOG_FIELDS, (float(v) for v in row))) for row in train_log]
    if global_buffer is not None:
        if out is not None:
            out.update(global_log=global_log)
        for row, grow in zip(rows, global_log):
            row.update(zip(_lib.GLOBAL_LOG_FIELDS, (float(v) for v in grow)))
    return rows


def new_population_best(P):
    """``new_best`` for ``P`` learners, stacked: best_return [P], best_weights [P, 77317], best_iter [P]."""
    return dict(best_return=np.full(int(P), -np.inf), best_weights=np.zeros((int(P), 77317), np.float32),
                best_iter=np.full(int(P), -1, np.int32))


def stack_critics(critics):
    """Packed critics (37569 weights each) as ``train_pop`` takes them: float32 [P, POP_CRITIC_STRIDE], every row
    16-byte aligned; the three pad floats of a row are never read or written by the library."""
    from . import _lib
    out = np.zeros((len(critics), _lib.POP_CRITIC_STRIDE), np.float32)
    for l, c in enumerate(critics):
        out[l, :_lib.CRITIC_NWEIGHTS] = np.asarray(c, np.float32).reshape(-1)
    return out


def population_stack(members):
    """The stacked arrays of a population from its members' (the inverse of ``population_member``).  A member is a
    dict of what ``train_device`` takes for one learner of B instances: ``target`` [B, 8], ``plant_pvec`` [B, 34],
    ``state`` and ``cstate`` (dicts of [B, ..] arrays), ``adam`` [2, 77317], ``adam_step`` [1], ``best``
    (``new_best``), and optionally ``pool`` (dict of [rows, B, ..] arrays), ``current_k`` [B, 34], ``weights`` [39748]
    and ``critic`` [37569].  Returns the same keys with the instances stacked learner-major (instance l B + b), ``adam``
    [P, 2, 77317], ``adam_step`` [P], ``best`` as ``new_population_best``, ``weights`` [P, 39748] and ``critic``
    [P, POP_CRITIC_STRIDE] (``stack_critics``).  Members that carry a ``global_buffer`` (``new_global_buffer``
    dicts) give the population's: arrays [P, capacity, ..] and the one ``fill`` all learners share; members that
    differ in fill or capacity raise ``DartMPCError`` (they share n, so a population's buffers fill in step)."""
    from . import _lib
    cat = lambda arrs, axis=0: np.ascontiguousarray(np.concatenate([np.asarray(a) for a in arrs], axis=axis))
    m0 = members[0]
    out = dict(target=cat([m["target"] for m in members]), plant_pvec=cat([m["plant_pvec"] for m in members]),
               state={k: cat([m["state"][k] for m in members]) for k in m0["state"]},
               cstate={k: cat([m["cstate"][k] for m in members]) for k in m0["cstate"]},
               adam=np.ascontiguousarray(np.stack([np.asarray(m["adam"]).reshape(2, -1) for m in members])),
               adam_step=cat([np.asarray(m["adam_step"]).reshape(1) for m in members]),
               best={k: (np.ascontiguousarray(np.stack([np.asarray(m["best"][k]).reshape(-1) for m in members]))
                         if k == "best_weights" else cat([np.asarray(m["best"][k]).reshape(1) for m in members]))
                     for k in ("best_return", "best_weights", "best_iter")})
    if m0.get("pool"):
        out["pool"] = {k: cat([m["pool"][k] for m in members], axis=1) for k in m0["pool"]}
    if "current_k" in m0:
        out["current_k"] = cat([np.asarray(m["current_k"]).reshape(-1, 34) for m in members])
    if "weights" in m0:
        out["weights"] = np.ascontiguousarray(np.stack([np.asarray(m["weights"], np.float32).reshape(-1)
                                                        for m in members]))
    if "critic" in m0:
        out["critic"] = stack_critics([m["critic"] for m in members])
    if m0.get("global_buffer") is not None:
        bufs = [m.get("global_buffer") for m in members]
        if any(b is None for b in bufs):
            raise _lib.DartMPCError("population_stack: some members have a global_buffer and some have none")
        fills = {int(b["fill"]) for b in bufs}
        caps = {int(np.asarray(b["logp"]).size) for b in bufs}
        if len(fills) != 1:
            raise _lib.DartMPCError(f"population_stack: members differ in global_buffer fill ({sorted(fills)})")
        if len(caps) != 1:
            raise _lib.DartMPCError(f"population_stack: members differ in global_buffer capacity ({sorted(caps)})")
        cap = caps.pop()
        gb = {name: np.ascontiguousarray(np.stack(
                  [np.asarray(b[name], dt).reshape((cap, width) if width else (cap,)) for b in bufs]))
              for name, width, dt in _lib.LMPC_GLOBAL_ARRAYS}
        gb["fill"] = fills.pop()
        out["global_buffer"] = gb
    return out


def population_member(l, P, pop):
    """Learner ``l`` of the ``P`` in ``pop`` (a dict as ``population_stack`` returns it; keys it lacks are left out),
    in the shapes ``train_device`` and ``save_checkpoint`` take: views of its slice of every stacked array -- writing
    through them writes the population -- except ``pool``, whose slice is not contiguous and is copied (it is only
    read).  ``critic`` is the 37569 weights of its row, without the pad.  ``global_buffer`` (when the population
    has one) is the learner's buffer as views [capacity, ..] plus the shared ``fill``: the dict ``train_device(...,
    global_buffer=...)`` and ``save_checkpoint(..., global_buffer=...)`` take, so a member can be checkpointed in the
    middle of a fill period and continued alone."""
    from . import _lib
    l, P = int(l), int(P)
    if not 0 <= l < P:
        raise _lib.DartMPCError(f"population_member: learner {l} of {P}")
    NI = np.asarray(pop["target"]).shape[0]
    if NI % P:
        raise _lib.DartMPCError(f"population_member: {NI} instances are not {P} learners of equal size")
    B = NI // P
    sl = slice(l * B, (l + 1) * B)
    out = dict(target=pop["target"][sl], plant_pvec=pop["plant_pvec"][sl],
               state={k: v[sl] for k, v in pop["state"].items()}, cstate={k: v[sl] for k, v in pop["cstate"].items()},
               adam=pop["adam"][l], adam_step=pop["adam_step"][l:l + 1],
               best={k: (pop["best"][k][l] if k == "best_weights" else pop["best"][k][l:l + 1])
                     for k in ("best_return", "best_weights", "best_iter")})
    if pop.get("pool"):
        out["pool"] = {k: np.ascontiguousarray(v[:, sl]) for k, v in pop["pool"].items()}
    if "current_k" in pop:
        out["current_k"] = pop["current_k"][sl]
    if "weights" in pop:
        out["weights"] = pop["weights"][l]
    if "critic" in pop:
        out["critic"] = pop["critic"][l, :_lib.CRITIC_NWEIGHTS]
    if pop.get("global_buffer") is not None:
        gb = pop["global_buffer"]
        out["global_buffer"] = dict({name: gb[name][l] for name, _, _ in _lib.LMPC_GLOBAL_ARRAYS}, fill=int(gb["fill"]))
    return out


def population_samples(P, B, R):
    """The sample lists of a population, int32 [P, R B]: entry r B + b of learner l is r (P B) + l B + b, the flat
    index of record r of instance l B + b in the stacked record arrays [R, P B]."""
    l, r, b = np.arange(P)[:, None, None], np.arange(R)[None, :, None], np.arange(B)[None, None, :]
    return (r * (P * B) + l * B + b).reshape(P, R * B).astype(np.int32)


def population_noise(seeds, iteration, steps, B):
    """The numpy statement of a population's stacked noise, float32 [steps, P B, 34]: learner l's block
    [:, l B:(l + 1) B] is ``harness.lmpc_train_noise(seeds[l], iteration, steps, B)``, the single run's draws."""
    from . import harness
    return np.ascontiguousarray(np.concatenate(
        [harness.lmpc_train_noise(int(sd), iteration, steps, B, np.float32) for sd in seeds], axis=1))


def train_population(solver, policies, target, plant_pvec, state, cstate, adam, adam_step, best, steps, seeds,
                     iterations=1, it0=0, rcfg=None, pool=None, prm=None, gamma=0.99, lam=0.95, mean_update=True,
                     track_best=True, epochs=8, mini_batch_size=64, out=None, global_buffer=None, hyper_table=None,
                     **hyper):
    """``train_device`` for a population: ``policies`` is a list of P ``LmpcPolicy(B, ...)`` that share one config,
    the other arrays are stacked learner-major as ``population_stack`` lays them out (``target`` [P B, 8], ``state``
    / ``cstate`` of P B instances, ``adam`` [P, 2, 77317], ``adam_step`` [P], ``best`` = ``new_population_best(P)``,
    ``pool`` [rows, P B, ..]), ``seeds`` are P integers.  All learners run in the same launches
    (``LmpcSolver.train_pop``); learner l is bit for bit ``train_device`` on ``population_member(l, ...)`` with
    ``seed=seeds[l]``.  Updated in place: the stacked arrays, and every policy's ``weights``, ``critic_weights`` and
    ``current_k``.  Returns one list of ``TRAIN_LOG_FIELDS`` dicts (one per iteration) per learner.

    With ``global_buffer`` (``new_population_global_buffer(P, n)``, or ``population_stack``'s) every iteration also
    runs the global-buffer update for every learner (``LmpcSolver.train_pop`` with the buffer): learner l is then bit
    for bit ``train_device(..., global_buffer=population_member(l, ...)["global_buffer"])``.  The dict is updated in
    place, ``fill`` included, and every returned row gains the keys of ``_lib.GLOBAL_LOG_FIELDS``.

    With ``hyper_table`` (float64 [P, HYPER_COLS], ``_lib.hyper_table``; read only) learner l trains with row l in
    place of the first nine fields of the shared config (``_lib.HYPER_FIELDS``): it is bit for bit ``train_device``
    with those values as ``hyper``.  None takes the entries above, unchanged."""
    from . import _lib
    P = len(policies)
    rcfg = rcfg if rcfg is not None else _lib.reward_config()
    NI, K = state["x"].shape[0], int(steps)
    if P < 1 or NI % P:
        raise _lib.DartMPCError(f"train_population: {NI} instances are not {P} learners of equal size")
    B = NI // P
    if any(p.critic_weights is None for p in policies):
        raise _lib.DartMPCError("training needs policies with critic_weights")
    cfg = _lib.ppo_config(**dict(hyper, epochs=epochs, mini_batch_size=mini_batch_size))
    tcfg = _lib.train_config(seed=0, iterations=iterations, it0=it0, steps=K, gamma=gamma, lam=lam,
                             mean_update=int(bool(mean_update)), track_best=int(bool(track_best)))
    R = K // max(int(rcfg.record_every), 1)
    weights = np.ascontiguousarray(np.stack([np.asarray(p.weights, np.float32).reshape(-1) for p in policies]))
    critic = stack_critics([p.critic_weights for p in policies])
    current_k = np.ascontiguousarray(np.concatenate([np.asarray(p.current_k, np.float64).reshape(B, 34)
                                                     for p in policies]))
    logs, clogs = _lib.loop_logs(_lib.LMPC_LOOP_LOGS, K, NI), _lib.loop_logs(_lib.LMPC_COLLECT_LOGS, K, NI)
    rec = _lib.loop_logs(_lib.LMPC_COLLECT_REC, R, NI)
    train_log = np.full((P, int(iterations), _lib.TRAIN_LOG_COLS), np.nan)
    global_log = None if global_buffer is None else np.full((P, int(iterations), _lib.GLOBAL_LOG_COLS), np.nan)
    solver.train_pop(P, seeds, target, plant_pvec, state, cstate, logs, clogs, rec, policies[0].cfg, weights, critic,
                     current_k, adam, adam_step, train_log, best["best_return"], best["best_weights"],
                     best["best_iter"], cfg, tcfg, rcfg=rcfg, prm=prm, pool=pool, global_buffer=global_buffer,
                     global_log=global_log, **({} if hyper_table is None else dict(hyper=hyper_table)))
    for l, p in enumerate(policies):
        p.weights[...] = weights[l].reshape(p.weights.shape)
        p.critic_weights[...] = critic[l, :_lib.CRITIC_NWEIGHTS].reshape(p.critic_weights.shape)
        p.current_k[...] = current_k[l * B:(l + 1) * B].reshape(p.current_k.shape)
    if out is not None:
        out.update(logs=logs, clogs=clogs, rec=rec, train_log=train_log, weights=weights, critic=critic)
    rows = [[dict(zip(_lib.TRAIN_LOG_FIELDS, (float(v) for v in row))) for row in train_log[l]] for l in range(P)]
    if global_buffer is not None:
        if out is not None:
            out.update(global_log=global_log)
        for l in range(P):
            for row, grow in zip(rows[l], global_log[l]):
                row.update(zip(_lib.GLOBAL_LOG_FIELDS, (float(v) for v in grow)))
    return rows


def evaluate_population(solver, pop, x0, targets, plant_pvec, steps, which="latest", pcfg=None, prm=None, noise=None,
                        plant=None):
    """Which learner of a population controls best: one device-resident rollout of all P (``LmpcSolver.evaluate``,
    metrics-only) on the B experiments ``x0``, ``targets`` [B, 8], ``plant_pvec`` [B, 34], the same for every learner.
    ``pop`` is a ``population_stack`` dict with ``weights``, ``current_k`` and ``state``; ``which`` = "latest" evaluates
    the members' weights, "best" the actor halves of their ``best["best_weights"]`` snapshots (every member needs one).
    The run starts from copies of the members' observation statistics, history, timestep and model_params, so ``pop``
    is not advanced.  ``noise`` None is zero noise: the policies' mean actions.  ``pcfg`` defaults to
    ``lmpc.policy_config()``.  Returns {"scores": [P, 8] (_lib.SCORE_SLOTS), "metrics": [P, B, 8], "best": the learner
    with the lowest mean steady-state error (slot 0; ties go to the lowest index)}."""
    from . import _lib
    from .lmpc import policy_config
    if which not in ("latest", "best"):
        raise _lib.DartMPCError(f"evaluate_population: which = {which!r} (\"latest\" or \"best\")")
    weights = np.asarray(pop["weights"], np.float32)
    P = weights.shape[0]
    NI = np.asarray(pop["state"]["x"]).shape[0]
    if P < 1 or NI % P:
        raise _lib.DartMPCError(f"evaluate_population: {NI} instances are not {P} learners of equal size")
    B = NI // P
    if which == "best":
        if np.any(np.asarray(pop["best"]["best_iter"]) < 0):
            raise _lib.DartMPCError("evaluate_population: a member has no best-policy snapshot yet")
        weights = np.asarray(pop["best"]["best_weights"], np.float32).reshape(P, -1)[:, :_lib.ACTOR_NWEIGHTS]
    tile = lambda a, n: np.ascontiguousarray(np.tile(np.asarray(a, np.float64).reshape(B, n), (P, 1)))
    state = {name: np.zeros(_lib._loop_shape(NI, width, nw=solver.nw), dt) for name, width, dt in _lib.LMPC_LOOP_STATE}
    state["x"][:] = tile(x0, 8)
    for name in ("obs_mean", "obs_M2", "obs_count", "history", "timestep", "model_params"):
        state[name][:] = np.asarray(pop["state"][name]).reshape(state[name].shape)
    state["metrics"] = _lib.loop_metrics(NI)
    scores = np.zeros((P, 8))
    solver.evaluate(P, 0, int(steps), tile(targets, 8), tile(plant_pvec, 34), state, None,
                    pcfg=pcfg if pcfg is not None else policy_config(), weights=np.ascontiguousarray(weights),
                    current_k=pop["current_k"], prm=None if prm is None else tile(prm, 22), noise=noise, scores=scores,
                    plant=plant)
    return {"scores": scores, "metrics": state["metrics"].reshape(P, B, 8), "best": int(np.argmin(scores[:, 0]))}


# ---- population-based training: per-learner hyper-parameters and the exploit/explore step -------------------------
# the defaults of dart_lmpc_pbt_config_default, restated so that ``pbt_plan`` needs no library
PBT_STREAM = 4                  # the generator stream of the step (streams 0-3: noise, permutations, choice, global)
PBT_DEFAULTS = dict(
    seed=0, generation=0, n_replace=0, higher_is_better=0, explore_mask=0b10101, factor_down=0.8, factor_up=1.25,
    # clip_eps, vf_coef, ent_coef, max_grad_norm, lr, beta1, beta2, adam_eps, weight_decay
    lo=(0.01, -np.inf, 0.0, 0.0, 1e-6, 0.0, 0.0, 0.0, -np.inf),
    hi=(0.5, np.inf, 0.1, np.inf, 1e-2, 0.999999, 0.999999, np.inf, np.inf))


def _pbt_settings(over):
    from . import _lib
    s = dict(PBT_DEFAULTS)
    for k, v in over.items():
        if k not in s:
            raise _lib.DartMPCError(f"pbt settings have no field {k!r} (fields: {sorted(s)})")
        s[k] = v
    for k in ("lo", "hi"):
        if isinstance(s[k], dict):
            b = list(PBT_DEFAULTS[k])
            for name, x in s[k].items():
                b[_lib.HYPER_FIELDS.index(name)] = float(x)
            s[k] = b
        s[k] = np.asarray(s[k], np.float64).reshape(-1)
        if s[k].size != _lib.HYPER_COLS:
            raise _lib.DartMPCError(f"pbt settings: {k} takes {_lib.HYPER_COLS} values")
    if not isinstance(s["explore_mask"], (int, np.integer)):
        s["explore_mask"] = sum(1 << _lib.HYPER_FIELDS.index(n) for n in set(s["explore_mask"]))
    return s


def pbt_check(P, **settings):
    """What dart_lmpc_pbt_step refuses of a config and a population size, checked on the host: raises ``DartMPCError``
    or returns the effective k (``n_replace``, 0 meaning P // 4)."""
    from . import _lib
    s = _pbt_settings(settings)
    P, k = int(P), int(s["n_replace"])
    if not 1 <= P <= _lib.POP_MAX:
        raise _lib.DartMPCError(f"pbt: 1 <= P <= {_lib.POP_MAX}, got {P}")
    if k < 0 or int(s["generation"]) < 0:
        raise _lib.DartMPCError("pbt: n_replace >= 0 and generation >= 0")
    k = k or P // 4
    if 2 * k > P:
        raise _lib.DartMPCError(f"pbt: 2 k <= P (k = {k}, P = {P}): no donor may be replaced")
    if not (s["factor_down"] > 0.0 and s["factor_up"] > 0.0):
        raise _lib.DartMPCError("pbt: the factors must be positive")
    if not np.all(s["lo"] <= s["hi"]):
        raise _lib.DartMPCError("pbt: lo[c] <= hi[c] for every column, no NaN bound")
    return k


def pbt_plan(fitness, hyper, seed=0, generation=0, fitness_stride=1, **settings):
    """The numpy statement of the exploit/explore step (dart_lmpc_pbt_step, csrc/lmpc_pbt.hip), bit for bit.
    ``fitness`` is read at ``l * fitness_stride``; ``hyper`` is the table [P, HYPER_COLS]; ``settings`` override
    PBT_DEFAULTS (``n_replace``, ``higher_is_better``, ``explore_mask``, ``factor_down``, ``factor_up``, ``lo``, ``hi``).

    Ranking: a is better than b if its fitness is strictly better in the configured direction, or the two compare
    equal and a < b; a NaN is worse than every non-NaN, NaNs are ordered by index.  Children are the learners of rank
    >= P - k, donors ranks 0 .. k - 1.  Child l's parent is the learner of rank word0 % k of the Philox block at counter
    (l, generation, 4, 0); column c of its row is the parent's, times factor_up / factor_down by the top bit of word
    c % 4 of block (l, generation, 4, 1 + c // 4) where the mask has bit c, then clamped to [lo[c], hi[c]] by
    comparisons a NaN passes through.  Returns (rank int32 [P], parent int32 [P], the new table)."""
    from . import harness
    hyper = np.array(hyper, np.float64)
    P = hyper.shape[0]
    s = _pbt_settings(dict(settings, seed=seed, generation=generation))
    k = pbt_check(P, **s)
    f = np.asarray(fitness, np.float64).reshape(-1)[::int(fitness_stride)][:P]
    higher = bool(s["higher_is_better"])

    def better(a, b):
        na, nb = np.isnan(f[a]), np.isnan(f[b])
        if na or nb:
            return (nb and a < b) if na else True
        strict = f[a] > f[b] if higher else f[a] < f[b]
        return bool(strict or (f[a] == f[b] and a < b))

    rank = np.array([sum(better(j, l) for j in range(P)) for l in range(P)], np.int32)
    by_rank = np.argsort(rank)
    parent = np.arange(P, dtype=np.int32)
    key = (int(s["seed"]) & 0xffffffff, (int(s["seed"]) >> 32) & 0xffffffff)
    gen, mask = int(s["generation"]), int(s["explore_mask"])
    out = hyper.copy()
    for l in range(P):
        if k == 0 or rank[l] < P - k:
            continue
        word0 = int(harness.philox4x32_10((l, gen, PBT_STREAM, 0), key)[0])
        parent[l] = by_rank[word0 % k]
        for c in range(hyper.shape[1]):
            v = hyper[parent[l], c]
            if (mask >> c) & 1:
                w = int(harness.philox4x32_10((l, gen, PBT_STREAM, 1 + c // 4), key)[c % 4])
                v = v * np.float64(s["factor_up"] if w >> 31 else s["factor_down"])
            lo, hi = s["lo"][c], s["hi"][c]
            out[l, c] = lo if v < lo else (hi if v > hi else v)
    return rank, parent, out


def pbt_apply(parent, weights, critic, adam, adam_step):
    """The copy half of the step on host arrays, in place: child l (``parent[l] != l``) receives its parent's actor
    row, its 37569 critic weights (the pad floats stay), both Adam moments and ``adam_step``."""
    from . import _lib
    for l, p in enumerate(np.asarray(parent)):
        if p != l:
            weights[l] = weights[p]
            critic[l, :_lib.CRITIC_NWEIGHTS] = critic[p, :_lib.CRITIC_NWEIGHTS]
            adam[l] = adam[p]
            adam_step[l] = adam_step[p]


def pbt_step(pop, hyper, fitness, seed=0, generation=0, fitness_stride=1, **settings):
    """The exploit/explore step through the host entry (dart_lmpc_pbt_step) on a ``population_stack`` dict with
    ``weights`` and ``critic``: its ``weights``, ``critic``, ``adam`` and ``adam_step`` and the table ``hyper``
    [P, HYPER_COLS] are updated in place.  Returns {"rank", "parent"} (int32 [P]); ``pbt_plan`` predicts them and
    the table."""
    from . import _lib
    s = _pbt_settings(dict(settings, seed=seed, generation=generation))
    cfg = _lib.pbt_config(**{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()})
    rank, parent = _lib.pbt_step(cfg, fitness, pop["weights"], pop["critic"], pop["adam"], pop["adam_step"], hyper,
                                 fitness_stride=fitness_stride)
    return {"rank": rank, "parent": parent}


def train_pbt(solver, policies, pop, hyper, x0, targets, plant_pvec, eval_steps, generations,
              iterations_per_generation, seeds, fitness_slot=0, steps=256, it0=0, generation0=0, rcfg=None, prm=None,
              gamma=0.99, lam=0.95, mean_update=True, track_best=True, epochs=8, mini_batch_size=64, pbt=None,
              **shared):
    """Population-based training with nothing on the host between the steps: per generation three calls are enqueued
    on one stream -- ``train_pop_hyper_dev`` for ``iterations_per_generation`` iterations of ``steps`` closed-loop
    steps, ``evaluate_dev`` (metrics only, zero noise) of every learner on the experiments ``x0``, ``targets`` [B, 8],
    ``plant_pvec`` [B, 34] from copies of the learners' policy state as ``evaluate_population`` makes them, and
    ``pbt_step_dev`` on column ``fitness_slot`` of the scores (``_lib.SCORE_SLOTS``) -- and the stream is synchronised
    once, after the last generation.

    ``policies`` is a list of P ``LmpcPolicy`` that share one config, ``pop`` a ``population_stack`` dict (``target``,
    ``plant_pvec``, ``state``, ``cstate``, ``adam``, ``adam_step``, ``best`` and optionally ``pool``) and ``hyper`` the
    table [P, HYPER_COLS] (``_lib.hyper_table``): all are updated in place, as are the policies' ``weights``,
    ``critic_weights`` and ``current_k``.  ``pbt`` overrides PBT_DEFAULTS (``seed``, ``n_replace``,
    ``higher_is_better``, ...; generation g of the call steps with ``generation0 + g``); ``shared`` overrides the shared
    fields of ``_lib.ppo_config`` (the table's columns are taken from ``hyper``).  Iteration indices run on from
    ``it0``.  Returns {"rows": per learner one ``TRAIN_LOG_FIELDS`` dict per iteration, "train_log"
    [P, generations * iterations_per_generation, 12], "rank" and "parent" [generations, P], "hyper"
    [generations, P, HYPER_COLS] (the table after each step), "scores" [generations, P, 8] (the last row: the final
    scores)}."""
    from . import _lib
    P, G, I, K = len(policies), int(generations), int(iterations_per_generation), int(steps)
    rcfg = rcfg if rcfg is not None else _lib.reward_config()
    NI = pop["state"]["x"].shape[0]
    if P < 1 or NI % P:
        raise _lib.DartMPCError(f"train_pbt: {NI} instances are not {P} learners of equal size")
    if G < 1 or I < 1 or int(eval_steps) < 1:
        raise _lib.DartMPCError("train_pbt: generations, iterations_per_generation and eval_steps must be positive")
    if not 0 <= int(fitness_slot) < 8:
        raise _lib.DartMPCError(f"train_pbt: fitness_slot in 0 .. 7 ({_lib.SCORE_SLOTS}), got {fitness_slot}")
    if any(p.critic_weights is None for p in policies):
        raise _lib.DartMPCError("training needs policies with critic_weights")
    if any(k in _lib.HYPER_FIELDS for k in shared):
        raise _lib.DartMPCError("train_pbt: the table's columns are set in hyper, not by keyword")
    B = NI // P
    hyper_h = _lib._inplace(hyper, np.float64, P * _lib.HYPER_COLS, "hyper").reshape(P, _lib.HYPER_COLS)
    seeds = np.ascontiguousarray(seeds, np.uint64).reshape(-1)
    s = _pbt_settings(dict(pbt or {}))
    pbt_check(P, **s)
    cfg = _lib.ppo_config(**dict(shared, epochs=epochs, mini_batch_size=mini_batch_size))
    R = K // max(int(rcfg.record_every), 1)
    ws_bytes = _lib.train_pop_workspace_bytes(P, B, K, int(rcfg.record_every), int(epochs), int(mini_batch_size))
    if ws_bytes == 0:
        raise _lib.DartMPCError("train_pbt: no training workspace for this shape (steps a multiple of record_every)")
    x0 = np.asarray(x0, np.float64).reshape(B, 8)
    tile = lambda a, n: np.ascontiguousarray(np.tile(np.asarray(a, np.float64).reshape(B, n), (P, 1)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()}
    # the training arrays, as train_pop_dev takes them
    weights = np.ascontiguousarray(np.stack([np.asarray(p.weights, np.float32).reshape(-1) for p in policies]))
    current_k = np.ascontiguousarray(np.concatenate([np.asarray(p.current_k, np.float64).reshape(B, 34)
                                                     for p in policies]))
    c = {k: dev(v) for k, v in dict(
        target=pop["target"], plant_pvec=pop["plant_pvec"], current_k=current_k, weights=weights,
        critic=stack_critics([p.critic_weights for p in policies]),
        prm=np.tile(_lib.LMPC_PRM_DEFAULT, (NI, 1)) if prm is None else np.asarray(prm, np.float64).reshape(NI, 22)).items()}
    st, cs = {k: dev(v) for k, v in pop["state"].items()}, {k: dev(v) for k, v in pop["cstate"].items()}
    lg = {k: dev(v) for k, v in _lib.loop_logs(_lib.LMPC_LOOP_LOGS, K, NI).items()}
    clg = {k: dev(v) for k, v in _lib.loop_logs(_lib.LMPC_COLLECT_LOGS, K, NI).items()}
    rec = {k: dev(v) for k, v in _lib.loop_logs(_lib.LMPC_COLLECT_REC, R, NI).items()}
    pool = {k: dev(v) for k, v in (pop.get("pool") or {}).items()}
    reset_rows = pop["pool"]["reset_x"].shape[0] if pool else 0
    nan64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    tlog = nan64(G, P, I, _lib.TRAIN_LOG_COLS)
    tr = dict(adam=dev(pop["adam"]), adam_step=dev(pop["adam_step"]), best_return=dev(pop["best"]["best_return"]),
              best_weights=dev(pop["best"]["best_weights"]), best_iter=dev(pop["best"]["best_iter"]),
              workspace=torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda"))
    hyper_d = dev(hyper_h)
    # the evaluation's arrays: every learner on the same B experiments, from copies of its policy state
    e_state = {name: torch.zeros(_lib._loop_shape(NI, width, nw=solver.nw), device="cuda",
                                  dtype={np.float64: torch.float64, np.float32: torch.float32,
                                         np.int32: torch.int32}[dt])
               for name, width, dt in _lib.LMPC_LOOP_STATE}
    e_state["metrics"] = torch.zeros((NI, 8), dtype=torch.float64, device="cuda")
    e_x0, e_metrics0 = dev(tile(x0, 8)), dev(_lib.loop_metrics(NI))
    e_target, e_pvec = dev(tile(targets, 8)), dev(tile(plant_pvec, 34))
    e_prm = dev(np.tile(_lib.LMPC_PRM_DEFAULT, (NI, 1)))
    scores, hyper_log = nan64(G, P, 8), nan64(G, P, _lib.HYPER_COLS)
    rank = torch.full((G, P), -1, dtype=torch.int32, device="cuda")
    parent = torch.full((G, P), -1, dtype=torch.int32, device="cuda")
    pcfg = policies[0].cfg
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()           # the uploads above ran on the current stream
    with torch.cuda.stream(stream):
        for g in range(G):
            tcfg = _lib.train_config(seed=0, iterations=I, it0=int(it0) + g * I, steps=K, gamma=gamma, lam=lam,
                                     mean_update=int(bool(mean_update)), track_best=int(bool(track_best)))
            train = dict(ptrs(tr), train_log=tlog[g].data_ptr())
            solver.train_pop_hyper_dev(P, seeds, B, reset_rows, c["target"].data_ptr(), c["prm"].data_ptr(),
                                       c["plant_pvec"].data_ptr(), c["current_k"].data_ptr(), c["weights"].data_ptr(),
                                       c["critic"].data_ptr(), ptrs(st), ptrs(cs), ptrs(lg), ptrs(clg), ptrs(rec), train,
                                       pcfg, rcfg, cfg, tcfg, gbuf=None, hyper=hyper_d.data_ptr(), pool=ptrs(pool),
                                       stream=stream.cuda_stream)
            for name, t in e_state.items():
                if name in ("obs_mean", "obs_M2", "obs_count", "history", "timestep", "model_params"):
                    t.copy_(st[name].reshape(t.shape), non_blocking=True)
                elif name == "x":
                    t.copy_(e_x0, non_blocking=True)
                elif name == "metrics":
                    t.copy_(e_metrics0, non_blocking=True)
                else:
                    t.zero_()
            solver.evaluate_dev(P, B, 0, int(eval_steps), int(eval_steps), e_target.data_ptr(), e_prm.data_ptr(),
                                e_pvec.data_ptr(), ptrs(e_state), None, pcfg=pcfg, weights=c["weights"].data_ptr(),
                                current_k=c["current_k"].data_ptr(), scores=scores[g].data_ptr(),
                                stream=stream.cuda_stream)
            pcf = _lib.pbt_config(**{k: (v.tolist() if isinstance(v, np.ndarray) else v)
                                     for k, v in dict(s, generation=int(generation0) + g).items()})
            solver.pbt_step_dev(pcf, P, scores[g].data_ptr() + 8 * int(fitness_slot), 8, c["weights"].data_ptr(),
                                c["critic"].data_ptr(), tr["adam"].data_ptr(), tr["adam_step"].data_ptr(),
                                hyper_d.data_ptr(), rank[g].data_ptr(), parent[g].data_ptr(),
                                stream=stream.cuda_stream)
            hyper_log[g].copy_(hyper_d, non_blocking=True)
    stream.synchronize()
    # everything back into the caller's arrays
    h = lambda t: t.cpu().numpy()
    pop["target"][...], pop["plant_pvec"][...] = h(c["target"]), h(c["plant_pvec"])
    for d_host, d_dev in ((pop["state"], st), (pop["cstate"], cs)):
        for k, v in d_dev.items():
            d_host[k][...] = h(v).reshape(d_host[k].shape)
    pop["adam"][...], pop["adam_step"][...] = h(tr["adam"]).reshape(pop["adam"].shape), h(tr["adam_step"])
    for k in ("best_return", "best_weights", "best_iter"):
        pop["best"][k][...] = h(tr[k]).reshape(pop["best"][k].shape)
    w_h, c_h, k_h = h(c["weights"]), h(c["critic"]), h(c["current_k"])
    for name, arr in (("weights", w_h), ("critic", c_h), ("current_k", k_h)):
        if name in pop:
            pop[name][...] = arr.reshape(pop[name].shape)
    for l, p in enumerate(policies):
        p.weights[...] = w_h[l].reshape(p.weights.shape)
        p.critic_weights[...] = c_h[l, :_lib.CRITIC_NWEIGHTS].reshape(p.critic_weights.shape)
        p.current_k[...] = k_h[l * B:(l + 1) * B].reshape(p.current_k.shape)
    hyper_h[...] = h(hyper_d)
    train_log = np.ascontiguousarray(h(tlog).transpose(1, 0, 2, 3).reshape(P, G * I, _lib.TRAIN_LOG_COLS))
    rows = [[dict(zip(_lib.TRAIN_LOG_FIELDS, (float(v) for v in row))) for row in train_log[l]] for l in range(P)]
    return {"rows": rows, "train_log": train_log, "rank": h(rank), "parent": h(parent), "hyper": h(hyper_log),
            "scores": h(scores)}


def new_population_global_buffer(P, n):
    """The global buffers of a fresh population of ``P`` learners with ``n`` samples per iteration each: zeroed
    arrays [P, G, ..] of capacity G (``_lib.global_rows``), stacked learner-major, and the one ``fill`` = 0 all
    learners share."""
    from . import _lib
    P = int(P)
    if not 1 <= P <= _lib.POP_MAX:
        raise _lib.DartMPCError(f"new_population_global_buffer: 1 <= P <= {_lib.POP_MAX}, got {P}")
    _, G = _lib.global_rows(n)
    buf = {name: np.zeros((P, G, width) if width else (P, G), dt) for name, width, dt in _lib.LMPC_GLOBAL_ARRAYS}
    buf["fill"] = 0
    return buf


def new_global_buffer(n):
    """The global buffer of a fresh training with ``n`` samples per iteration: zeroed arrays of capacity G
    (``_lib.global_rows``) and ``fill`` = 0."""
    from . import _lib
    _, G = _lib.global_rows(n)
    buf = {name: np.zeros((G, width) if width else (G,), dt) for name, width, dt in _lib.LMPC_GLOBAL_ARRAYS}
    buf["fill"] = 0
    return buf


def new_best():
    """The best-policy state of a fresh training: best_return -inf, no weights, best_iter -1."""
    return dict(best_return=np.array([-np.inf]), best_weights=np.zeros(77317, np.float32),
                best_iter=np.array([-1], np.int32))


# name -> (dtype, trailing shape; None: any) of a checkpoint's arrays
CHECKPOINT_FIELDS = {
    "actor": (np.float32, (39748,)), "critic": (np.float32, (37569,)), "adam": (np.float32, (2, 77317)),
    "adam_step": (np.int32, (1,)), "best_weights": (np.float32, (77317,)), "best_return": (np.float64, (1,)),
    "best_iter": (np.int32, (1,)), "iteration": (np.int64, (1,)), "obs_mean": (np.float64, (None, 52)),
    "obs_M2": (np.float64, (None, 52)), "obs_count": (np.int32, (None,)), "history": (np.float32, (None, 520)),
    "current_k": (np.float64, (None, 34)), "model_params": (np.float64, (None, 34)),
}


# the optional arrays of the global buffer: name -> (dtype, trailing shape; None: the buffer's capacity)
CHECKPOINT_GLOBAL_FIELDS = {
    "g_obs": (np.float32, (None, 520)), "g_action": (np.float32, (None, 34)), "g_logp": (np.float32, (None,)),
    "g_value": (np.float32, (None,)), "g_reward": (np.float64, (None,)), "g_done": (np.float32, (None,)),
    "g_fill": (np.int64, (1,)),
}


# the optional row of a population's hyper-parameter table: (dtype, shape)
CHECKPOINT_HYPER_FIELD = (np.float64, (9,))


def save_checkpoint(path, actor, critic, adam, adam_step, best, iteration, obs_mean, obs_M2, obs_count, history,
                    current_k, model_params, global_buffer=None, hyper=None):
    """One ``.npz`` of plain arrays (``CHECKPOINT_FIELDS``; readable with ``allow_pickle=False``): the packed actor
    and critic, Adam's state, the best-policy snapshot (``best`` as ``train_device`` takes it), the number of
    iterations done and the policy's Welford state, history, ``current_k`` and ``model_params`` for B controllers.
    With ``global_buffer`` (the dict of ``new_global_buffer``) the file also holds the plain arrays ``g_obs`` ..
    ``g_done`` and ``g_fill`` (``CHECKPOINT_GLOBAL_FIELDS``), so that a training can resume in the middle of a fill
    period.  With ``hyper`` (a member's row of a population's hyper-parameter table, ``_lib.HYPER_COLS`` values) the
    file also holds the plain array ``hyper``.  Returns the path written (numpy appends ``.npz`` to a path without
    it)."""
    from ._lib import DartMPCError
    B = np.asarray(obs_count).reshape(-1).size
    given = dict(actor=actor, critic=critic, adam=adam, adam_step=adam_step, best_weights=best["best_weights"],
                 best_return=best["best_return"], best_iter=best["best_iter"], iteration=[int(iteration)],
                 obs_mean=obs_mean, obs_M2=obs_M2, obs_count=obs_count, history=history, current_k=current_k,
                 model_params=model_params)
    arrays = {}
    for name, (dt, shape) in CHECKPOINT_FIELDS.items():
        want = tuple(B if d is None else d for d in shape)
        a = np.asarray(given[name])
        if a.size != int(np.prod(want)):
            raise DartMPCError(f"checkpoint field {name!r} must have shape {want}, got {a.shape}")
        arrays[name] = np.ascontiguousarray(a, dt).reshape(want)
    if global_buffer is not None:
        cap = np.asarray(global_buffer["logp"]).size
        for name, (dt, shape) in CHECKPOINT_GLOBAL_FIELDS.items():
            want = tuple(cap if d is None else d for d in shape)
            a = np.asarray(global_buffer[name[2:]])
            if a.size != int(np.prod(want)):
                raise DartMPCError(f"checkpoint field {name!r} must have shape {want}, got {a.shape}")
            arrays[name] = np.ascontiguousarray(a, dt).reshape(want)
        if not 0 <= int(arrays["g_fill"][0]) <= cap:
            raise DartMPCError(f"checkpoint field 'g_fill' must lie in [0, {cap}]")
    if hyper is not None:
        a = np.asarray(hyper)
        if a.size != CHECKPOINT_HYPER_FIELD[1][0]:
            raise DartMPCError(f"checkpoint field 'hyper' must have shape {CHECKPOINT_HYPER_FIELD[1]}, got {a.shape}")
        arrays["hyper"] = np.ascontiguousarray(a, CHECKPOINT_HYPER_FIELD[0]).reshape(CHECKPOINT_HYPER_FIELD[1])
    path = str(path)
    path = path if path.endswith(".npz") else path + ".npz"
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)
    return path


def load_checkpoint(path):
    """The arrays ``save_checkpoint`` wrote, as a dict name -> array (``allow_pickle=False``: a file that holds
    pickled objects is refused).  A missing field, a wrong dtype or a wrong shape raises ``DartMPCError``.  The
    arrays of a global buffer (``CHECKPOINT_GLOBAL_FIELDS``) are returned when the file holds them -- all of them or
    none; ``global_buffer_from_checkpoint`` turns them back into the dict ``train_device`` takes.  ``hyper`` (a
    member's hyper-parameters, float64 [9]) is returned when the file holds it; files written without it load as
    before."""
    from ._lib import DartMPCError
    try:
        with np.load(str(path), allow_pickle=False) as z:
            got = {name: z[name] for name in z.files}
    except (ValueError, OSError, KeyError) as e:
        raise DartMPCError(f"{path}: not a readable checkpoint ({e})") from e
    out = {}
    B = None
    for name, (dt, shape) in CHECKPOINT_FIELDS.items():
        if name not in got:
            raise DartMPCError(f"{path}: checkpoint field {name!r} is missing")
        a = got[name]
        if a.dtype != np.dtype(dt) or a.ndim != len(shape):
            raise DartMPCError(f"{path}: checkpoint field {name!r} must be {np.dtype(dt).name} with {len(shape)} axes")
        for have, want in zip(a.shape, shape):
            if want is None:
                B = have if B is None else B
                want = B
            if have != want:
                raise DartMPCError(f"{path}: checkpoint field {name!r} has shape {a.shape}")
        out[name] = np.ascontiguousarray(a)
    if any(name in got for name in CHECKPOINT_GLOBAL_FIELDS):
        cap = None
        for name, (dt, shape) in CHECKPOINT_GLOBAL_FIELDS.items():
            if name not in got:
                raise DartMPCError(f"{path}: checkpoint field {name!r} is missing")
            a = got[name]
            if a.dtype != np.dtype(dt) or a.ndim != len(shape):
                raise DartMPCError(f"{path}: checkpoint field {name!r} must be {np.dtype(dt).name} with {len(shape)} axes")
            for have, want in zip(a.shape, shape):
                if want is None:
                    cap = have if cap is None else cap
                    want = cap
                if have != want:
                    raise DartMPCError(f"{path}: checkpoint field {name!r} has shape {a.shape}")
            out[name] = np.ascontiguousarray(a)
    if "hyper" in got:
        a = got["hyper"]
        if a.dtype != np.dtype(CHECKPOINT_HYPER_FIELD[0]) or a.shape != CHECKPOINT_HYPER_FIELD[1]:
            raise DartMPCError(f"{path}: checkpoint field 'hyper' must be float64 with shape {CHECKPOINT_HYPER_FIELD[1]}")
        out["hyper"] = np.ascontiguousarray(a)
    return out


def global_buffer_from_checkpoint(ck):
    """The ``new_global_buffer`` dict held in a loaded checkpoint (fresh arrays), or None when it has none."""
    if "g_fill" not in ck:
        return None
    buf = {name[2:]: np.array(ck[name]) for name in CHECKPOINT_GLOBAL_FIELDS if name != "g_fill"}
    buf["fill"] = int(ck["g_fill"][0])
    return buf
