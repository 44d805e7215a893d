"""LMPC experience collection, the host side (no GPU): harness.lmpc_reward_step, the numpy critic, the numpy GAE,
dart_mpc.ppo.  The references are restatements of LMPC/src/controller/rlmpc2.py written here, line by line.

Bars: rewards 1e-12 relative (both sides are fp64 numpy in the same operation order; only the association of sums
inside numpy's reductions could differ), done bits / counters / returns equal; the fp32 nets against torch to
np.allclose(rtol = atol = 1e-5), the bar tests/test_gpu_policy.py holds the actor to."""
import numpy as np
import torch

import lmpc_policy as lp


def _scalar_reward_loop(cfg, X, T, U, RAW, max_delta, action_scale):
    """rlmpc2.py:703-740, 771-773, 900-935 for one controller over a trajectory: X [K, 8] the states, T [K, 8] the
    targets, U [K, 2] views["control"] at every step, RAW [K, 34] the drawn actions (fp32)."""
    prev_cmd = U[0].copy()                                                      # :564
    time_penalty, episode_step, episode_return, episodes = 0.0, 0, 0.0, 0
    last_return, last_steps = 0.0, 0
    rewards, dones, damped = [], [], []
    for state, target, control, raw in zip(X, T, U, RAW):
        delta_z = raw * np.float32(max_delta * action_scale)                   # :680 (an fp32 tensor)
        delta_z_norm = np.linalg.norm(delta_z.reshape(-1))                     # :683
        per_dim_rms = float(delta_z_norm) / np.sqrt(34)                        # :684
        damped.append(per_dim_rms > cfg["max_per_dim_rms"])
        if per_dim_rms > cfg["max_per_dim_rms"]:                               # :692-694
            damp = cfg["max_per_dim_rms"] / (per_dim_rms + 1e-12)
            delta_z = delta_z * np.float32(float(damp))
        pos = np.array([state[0], state[2]])                                   # :703-711
        vel = np.array([state[1], state[3]])
        tpos = np.array([target[0], target[2]])
        tvel = np.array([0, 0])
        pos_err = np.linalg.norm(np.abs(tpos - pos))
        vel_err = np.linalg.norm(np.abs(tvel - vel))
        change_cost = float(np.linalg.norm(delta_z))
        ctrl_rate_penalty = np.sum(np.abs(control - prev_cmd))
        prev_cmd = control
        pos_term = np.exp(-(pos_err ** 2) / (2 * cfg["sigma_pos"] ** 2))       # :601-604
        vel_term = np.exp(-(vel_err ** 2) / (2 * cfg["sigma_vel"] ** 2))
        proximity_reward = cfg["w_pos"] * pos_term + cfg["w_vel"] * pos_term * vel_term
        change_penalty = cfg["w_change"] * change_cost                         # :713-717
        control_rate_penalty = cfg["w_d_ctrl"] * ctrl_rate_penalty
        reward = proximity_reward - change_penalty - control_rate_penalty - time_penalty
        if pos_err < cfg["success_tol"] and vel_err < cfg["success_tol"]:      # :720-721
            reward += cfg["success_bonus"]
        done = 0
        episode_step += 1
        if abs(state[0]) > cfg["tray_limit"][0] or abs(state[2]) > cfg["tray_limit"][1]:    # :726-730
            reward -= cfg["oob_penalty"]
            done |= 1
        if episode_step >= cfg["max_episode_steps"]:                           # :738-740
            done |= 2
        time_penalty += cfg["time_penalty_rate"]                               # :772-773
        episode_return += reward
        if done:                                                               # :900-935
            last_return, last_steps = episode_return, episode_step
            episodes += 1
            episode_return, episode_step, time_penalty = 0.0, 0, 0.0
        rewards.append(reward); dones.append(done)
    return dict(reward=np.array(rewards), done=np.array(dones), damped=np.array(damped), episodes=episodes,
                last_return=last_return, last_steps=last_steps, ep_return=episode_return, ep_step=episode_step,
                time_penalty=time_penalty, prev_cmd=prev_cmd)


def test_reward_step_matches_scalar_restatement():
    from dart_mpc import _lib, harness
    K, B = 60, 3
    cfg = dict(sigma_pos=0.02, sigma_vel=0.02, w_pos=40.0, w_vel=0.1, w_change=1e-3, w_d_ctrl=5.0, success_tol=0.01,
               success_bonus=20.0, oob_penalty=20.0, tray_limit=(0.2, 0.15), max_per_dim_rms=0.02,
               time_penalty_rate=1e-4, max_episode_steps=6)
    rcfg = _lib.reward_config(**cfg)
    rng = np.random.default_rng(11)
    T = np.zeros((K, B, 8)); T[:, :, [0, 2]] = rng.uniform(-0.1, 0.1, (1, B, 2))
    T[30:, 1, 0] += 0.03                                                       # a target jump (after a reset)
    X = T + rng.normal(0, 0.02, (K, B, 8))
    X[10, 0] = T[10, 0]; X[10, 0, [1, 3]] = [0.001, -0.002]                    # success bonus
    X[20, 1, 0] = 0.25                                                         # out of bounds in x
    X[41, 2, 2] = -0.16                                                        # out of bounds in y
    U = rng.uniform(-0.4, 0.4, (K, B, 2))
    RAW = rng.standard_normal((K, B, 34)).astype(np.float32)                   # rms of delta_z about 0.02: both sides
    cs = _lib.LmpcSolver.collect_state(U[0])
    R, Dn = np.empty((K, B)), np.empty((K, B), np.int32)
    for k in range(K):
        R[k], Dn[k] = harness.lmpc_reward_step(rcfg, cs, X[k], T[k], U[k], RAW[k], 0.02, 1.0)
    for b in range(B):
        ref = _scalar_reward_loop(cfg, X[:, b], T[:, b], U[:, b], RAW[:, b], 0.02, 1.0)
        assert ref["damped"].any() and not ref["damped"].all()
        rel = np.max(np.abs(R[:, b] - ref["reward"]) / np.maximum(1.0, np.abs(ref["reward"])))
        assert rel <= 1e-12, (b, rel)
        np.testing.assert_array_equal(Dn[:, b], ref["done"])
        for name in ("episodes", "last_steps", "ep_step"):
            assert int(cs[name][b]) == ref[name], name
        for name in ("last_return", "ep_return", "time_penalty"):
            assert abs(cs[name][b] - ref[name]) <= 1e-12 * max(1.0, abs(ref[name])), name
        np.testing.assert_array_equal(cs["prev_cmd"][b], ref["prev_cmd"])
    assert Dn[20, 1] & 1 and Dn[41, 2] & 1 and (Dn & 2).any() and (Dn == 0).any()
    assert R[10, 0] > 20.0                                                     # the success step
    assert np.all(cs["episodes"] >= K // 6)


def _reference_nets(actor, critic):
    """The reference's layers (Policy.__init__, :39-55) holding the packed weights."""
    from torch import nn

    def seq(w, n_out):
        net = nn.Sequential(nn.Linear(520, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out))
        o = 0
        with torch.no_grad():
            for m in net:
                if isinstance(m, nn.Linear):
                    no, ni = m.weight.shape
                    m.weight.copy_(torch.from_numpy(w[o:o + ni * no].reshape(ni, no).T.copy())); o += ni * no
                    m.bias.copy_(torch.from_numpy(w[o:o + no].copy())); o += no
        return net, o
    a, na = seq(np.asarray(actor, np.float32), 34)
    c, nc = seq(np.asarray(critic, np.float32), 1)
    assert na + 34 == actor.size and nc == critic.size
    return a, c


def test_numpy_critic_matches_torch_layers():
    from dart_mpc import harness
    from dart_mpc.lmpc import init_critic_weights, init_policy_weights
    rng = np.random.default_rng(3)
    critic = init_critic_weights(5)
    critic[520 * 64:520 * 64 + 64] = rng.normal(0, 0.1, 64)                    # non-zero biases
    critic[-1] = 0.3
    assert critic.size == 37569
    obs = rng.standard_normal((40, 520)).astype(np.float32)
    _, cnet = _reference_nets(init_policy_weights(0), critic)
    with torch.no_grad():
        ref = cnet(torch.from_numpy(obs)).squeeze(-1).numpy()
    got = harness.lmpc_critic_value(critic, obs)
    assert got.dtype == np.float32 and got.shape == (40,)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5), float(np.max(np.abs(got - ref)))
    # and the log-probability against torch's Normal
    actor = init_policy_weights(0)
    mean, log_std = harness.lmpc_actor_mean(actor, obs)
    raw = (mean + 0.1 * rng.standard_normal(mean.shape)).astype(np.float32)
    lo, hi = float(np.log(1e-2)), float(np.log(2.0))
    std = torch.exp(torch.clamp(torch.from_numpy(log_std.copy()), lo, hi))
    ref_lp = torch.distributions.Normal(torch.from_numpy(mean), std).log_prob(torch.from_numpy(raw)).sum(-1).numpy()
    assert np.allclose(harness.lmpc_log_prob(mean, log_std, raw, lo, hi), ref_lp, rtol=1e-5, atol=1e-5)


def test_pack_load_round_trip_and_oracle_mlp():
    from dart_mpc import ppo
    torch.manual_seed(0)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    actor, critic = ppo.pack_weights(net)
    assert actor.shape == (39748,) and critic.shape == (37569,) and actor.dtype == critic.dtype == np.float32
    other = ppo.load_weights(ppo.PolicyNet(), actor, critic)
    for (n, p), (_, q) in zip(net.named_parameters(), other.named_parameters()):
        assert torch.equal(p, q), n
    a2, c2 = ppo.pack_weights(other)
    np.testing.assert_array_equal(a2, actor); np.testing.assert_array_equal(c2, critic)
    # PolicyNet.mean_net on packed weights = the numpy MLP of the policy oracle
    W1, b1, W2, b2, W3, b3, log_std = lp.unpack(actor)
    obs = np.random.default_rng(1).standard_normal((16, 520)).astype(np.float32)
    ref = np.tanh(np.tanh(obs @ W1 + b1) @ W2 + b2) @ W3 + b3
    with torch.no_grad():
        mean, std, val = other(torch.from_numpy(obs))
    assert np.allclose(mean.numpy(), ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(log_std, net.log_std.detach().numpy())
    assert val.shape == (16,) and std.shape == (34,)


def test_numpy_gae_equals_list_recursion():
    from dart_mpc import harness

    def compute_gae(rewards, values, dones, last_value, gamma, lam):            # rlmpc2.py:592-599, verbatim logic
        adv, gae = [], 0.0
        values = values + [last_value]
        for step in reversed(range(len(rewards))):
            delta = rewards[step] + gamma * values[step + 1] * (1.0 - dones[step]) - values[step]
            gae = delta + gamma * lam * (1.0 - dones[step]) * gae
            adv.insert(0, gae)
        return adv

    rng = np.random.default_rng(2)
    rows, B = 9, 5
    nrec = np.array([0, 1, 9, 4, 7], np.int32)
    rw = rng.normal(0, 5, (rows, B))
    rv = rng.normal(0, 3, (rows, B)).astype(np.float32)
    rd = (rng.uniform(size=(rows, B)) < 0.3).astype(np.float32)
    lv = rng.normal(0, 3, B).astype(np.float32)
    adv, ret = harness.gae_numpy(nrec, rw, rv, rd, lv, 0.99, 0.95)
    for b in range(B):
        n = int(nrec[b])
        want = compute_gae(list(rw[:n, b]), [float(v) for v in rv[:n, b]], [float(d) for d in rd[:n, b]], float(lv[b]),
                           0.99, 0.95)
        np.testing.assert_array_equal(adv[:n, b], np.array(want, float))
        np.testing.assert_array_equal(ret[:n, b], np.array(want, float) + rv[:n, b].astype(float))
        assert np.isnan(adv[n:, b]).all() and np.isnan(ret[n:, b]).all()


def test_ppo_update_moves_every_parameter():
    from dart_mpc import ppo
    torch.manual_seed(1)
    net = ppo.PolicyNet()
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, weight_decay=1e-5)
    rng = np.random.default_rng(4)
    n = 96
    obs = rng.standard_normal((n, 520)).astype(np.float32)
    with torch.no_grad():
        mean, std, _ = net(torch.from_numpy(obs))
        act = mean + std * torch.randn(mean.shape, generator=torch.Generator().manual_seed(2))
        logp = torch.distributions.Normal(mean, std).log_prob(act).sum(-1)
    batch = dict(obs=obs, action=act.numpy(), logp=logp.numpy(), adv=rng.normal(0, 2, n), ret=rng.normal(5, 3, n))
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    out = ppo.ppo_update(net, opt, batch, clip_eps=0.2, epochs=2, mini_batch_size=32, vf_coef=0.25, ent_coef=0.01,
                         generator=torch.Generator().manual_seed(3))
    assert all(np.isfinite(out[k]) for k in ("policy_loss", "value_loss", "entropy"))
    for name, p in net.named_parameters():
        assert torch.isfinite(p).all(), name
        assert not torch.equal(p, before[name]), f"{name} did not move"
    # (log_std is not held to any range here: the clamp is in forward(), not on the parameter)
