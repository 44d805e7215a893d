"""The device PPO update, the host side (no GPU): argument checks of dart_lmpc_ppo_update that return before any
device work, the config defaults (rlmpc2.py:202-226, 561), and the helpers of dart_mpc.ppo that move Adam's state
and the permutations between torch and the packed arrays."""
import ctypes

import numpy as np
import torch


def _valid_call():
    """Arguments of dart_lmpc_ppo_update that pass every check (n = 5 samples in 8 record rows, 2 epochs)."""
    from dart_mpc import _lib
    n, total = 5, 8
    a = dict(cfg=_lib.ppo_config(epochs=2, mini_batch_size=4), n=n, total=total,
             sample=np.array([0, 2, 3, 5, 7], np.int32), perm=np.stack([np.arange(n), np.arange(n)[::-1]]).astype(np.int32),
             obs=np.zeros((total, 520), np.float32), act=np.zeros((total, 34), np.float32),
             logp=np.zeros(total, np.float32), adv=np.zeros(total), ret=np.zeros(total),
             weights=np.zeros(_lib.ACTOR_NWEIGHTS + 4, np.float32), critic=np.zeros(_lib.CRITIC_NWEIGHTS, np.float32),
             adam=np.zeros((2, _lib.PPO_NPARAMS), np.float32), step=np.zeros(1, np.int32), stats=np.zeros(3))
    assert a["weights"].ctypes.data % 16 == 0 and a["critic"].ctypes.data % 16 == 0
    return a


def _call(a, weights_offset=0):
    from dart_mpc import _lib
    p = lambda v: ctypes.c_void_p(v.ctypes.data)
    return _lib.lib().dart_lmpc_ppo_update(
        ctypes.byref(a["cfg"]), a["n"], a["total"], p(a["sample"]), p(a["perm"]), p(a["obs"]), p(a["act"]), p(a["logp"]),
        p(a["adv"]), p(a["ret"]), ctypes.c_void_p(a["weights"].ctypes.data + weights_offset), p(a["critic"]),
        p(a["adam"]), p(a["step"]), p(a["stats"]), None, None, None)


def test_update_rejects_bad_arguments_without_touching_a_gpu():
    from dart_mpc import _lib
    a = _valid_call(); a["n"] = 0
    assert _call(a) == -1
    a = _valid_call(); a["cfg"].mini_batch_size = 0
    assert _call(a) == -1
    a = _valid_call(); a["cfg"].mini_batch_size = 1025
    assert _call(a) == -1
    a = _valid_call(); a["perm"][1, 2] = a["n"]                       # a perm entry equal to n
    assert _call(a) == -1
    a = _valid_call(); a["perm"][0, 0] = -1
    assert _call(a) == -1
    a = _valid_call(); a["sample"][4] = a["total"]                    # a sample entry past the record arrays
    assert _call(a) == -1
    a = _valid_call(); a["sample"][0] = -1
    assert _call(a) == -1
    assert _call(_valid_call(), weights_offset=4) == -1               # misaligned weights
    # the device entries check what they can see: the config, the counts, the alignment
    L = _lib.lib()
    z, c = ctypes.c_void_p(256), _lib.ppo_config()
    assert L.dart_lmpc_ppo_update_dev(ctypes.byref(c), 0, 8, *([z] * 17)) == -1
    assert L.dart_lmpc_ppo_update_dev(ctypes.byref(c), 4, 8, *([z] * 7), ctypes.c_void_p(260), *([z] * 9)) == -1
    assert L.dart_lmpc_ppo_grad_dev(ctypes.byref(c), 4, 8, 1025, *([z] * 11)) == -1
    assert L.dart_lmpc_ppo_prepare_dev(0, 8, *([z] * 7)) == -1
    assert L.dart_lmpc_critic_value(-1, None, None, None) == -1 and L.dart_lmpc_critic_value(3, None, None, None) == -1
    assert L.dart_lmpc_ppo_workspace_bytes(0, 64) == 0 and L.dart_lmpc_ppo_workspace_bytes(10, 1025) == 0
    w64, w80 = _lib.ppo_workspace_bytes(150, 64), _lib.ppo_workspace_bytes(150, 80)
    # one partial gradient per tile of 16 samples and the sum (every block rounded to 256 bytes)
    assert w80 - w64 >= 4 * 77317 - 256 and w64 > 4 * 77317 * 5


def test_ppo_config_default_carries_the_reference_values():
    from dart_mpc import _lib
    c = _lib.ppo_config()
    assert (c.clip_eps, c.epochs, c.mini_batch_size, c.vf_coef, c.ent_coef, c.max_grad_norm) == (0.2, 8, 64, 0.25, 0.01, 0.5)
    assert (c.lr, c.beta1, c.beta2, c.adam_eps, c.weight_decay) == (3e-4, 0.9, 0.999, 1e-8, 1e-5)
    assert c.log_std_min == float(np.log(1e-2)) and c.log_std_max == float(np.log(2.0))
    assert _lib.PPO_NPARAMS == 77317 and ctypes.sizeof(_lib.PpoConfig) == 96
    assert _lib.ppo_config(epochs=3, lr=1e-3).epochs == 3


def _net(seed=0):
    from dart_mpc import ppo
    torch.manual_seed(seed)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return net


def test_pack_adam_load_adam_round_trip():
    from dart_mpc import ppo
    net = _net()
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)
    adam, step = ppo.pack_adam(net, opt)                              # a fresh optimizer packs to zeros
    assert adam.shape == (2, 77317) and adam.dtype == np.float32 and not adam.any()
    assert step.dtype == np.int32 and step.tolist() == [0]
    for i in range(3):
        opt.zero_grad()
        mean, std, val = net(torch.randn(8, 520, generator=torch.Generator().manual_seed(i)))
        (mean.square().mean() + val.square().mean() + std.sum()).backward()
        opt.step()
    adam, step = ppo.pack_adam(net, opt)
    assert step.tolist() == [3] and adam[0].any() and (adam[1] >= 0).all()
    # the packed order is pack_weights' order: the first moment of W1 [in, out] comes first, log_std's last of the actor
    np.testing.assert_array_equal(adam[0, :520 * 64], opt.state[net.mean_net[0].weight]["exp_avg"].numpy().T.reshape(-1))
    np.testing.assert_array_equal(adam[1, 39748 - 34:39748], opt.state[net.log_std]["exp_avg_sq"].numpy())
    other = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)
    ppo.load_adam(net, other, adam, step)
    for p in net.parameters():
        assert torch.equal(other.state[p]["exp_avg"], opt.state[p]["exp_avg"])
        assert torch.equal(other.state[p]["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
        assert float(other.state[p]["step"]) == 3.0
    a2, s2 = ppo.pack_adam(net, other)
    np.testing.assert_array_equal(a2, adam); np.testing.assert_array_equal(s2, step)
    # pack_grads follows the same order
    g = ppo.pack_grads(net)
    assert g.shape == (77317,)
    np.testing.assert_array_equal(g[39748:39748 + 520 * 64], net.value_net[0].weight.grad.numpy().T.reshape(-1))


def test_make_perms_are_the_draws_of_ppo_update():
    from dart_mpc import ppo
    n, epochs = 37, 3
    perms = ppo.make_perms(n, epochs, torch.Generator().manual_seed(5))
    assert perms.shape == (epochs, n) and perms.dtype == np.int32
    gen = torch.Generator().manual_seed(5)
    for e in range(epochs):
        np.testing.assert_array_equal(perms[e], torch.randperm(n, generator=gen).numpy())
        assert sorted(perms[e].tolist()) == list(range(n))
    assert ppo.make_perms(n, 0).shape == (0, n)
