"""PPO update of the LMPC parameter policy on collected experience.

Restates the training half of RLMPC._rl_worker (LMPC/src/controller/rlmpc2.py): ``PolicyNet`` is ``Policy``
(:33-80), ``ppo_update`` the clipped-surrogate update of :783-819 in plain torch, ``ppo_update_device`` the same
update as HIP kernels (csrc/lmpc_ppo.hip, ``_lib.ppo_update``) on the packed weights and Adam state in place.  The
torch path is the reference the device path is tested against; ``make_perms`` gives both the same mini-batches.
Experience comes from ``dart_lmpc_collect`` (harness.collect_lmpc) and ``_lib.gae``; ``pack_weights`` /
``load_weights`` and ``pack_adam`` / ``load_adam`` move the weights and Adam's state between the torch objects and
the packed input-major arrays the kernels read.  The reference's ``.pth`` checkpoints are not loaded.
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
