"""The host side of the device-resident LMPC training (no GPU): the checkpoint format of dart_mpc.ppo, the numpy
statements of the generator and of the mean-based parameter write (harness), and the argument checks of the
training entries that return before any device work."""
import ctypes

import numpy as np
import pytest


def _state(B=3, seed=0):
    from dart_mpc import ppo
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    best = dict(best_return=np.array([rng.standard_normal()]), best_weights=f32(77317), best_iter=np.array([4], np.int32))
    return dict(actor=f32(39748), critic=f32(37569), adam=f32(2, 77317), adam_step=np.array([160], np.int32),
                best=best, iteration=7, obs_mean=rng.standard_normal((B, 52)), obs_M2=rng.random((B, 52)),
                obs_count=np.full(B, 1792, np.int32), history=f32(B, 520), current_k=rng.random((B, 34)) + 0.5,
                model_params=rng.random((B, 34)) + 0.5), ppo


def test_checkpoint_round_trip(tmp_path):
    st, ppo = _state()
    path = ppo.save_checkpoint(tmp_path / "latest", **st)
    assert path.endswith("latest.npz")
    with np.load(path, allow_pickle=False) as z:                 # plain arrays: opens without pickle
        assert sorted(z.files) == sorted(ppo.CHECKPOINT_FIELDS)
    got = ppo.load_checkpoint(path)
    flat = {**{k: v for k, v in st.items() if k != "best"}, **st["best"], "iteration": np.array([7], np.int64)}
    assert sorted(got) == sorted(flat)
    for k, v in flat.items():
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(v)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    # -inf and NaN survive (a fresh best_return)
    st["best"] = ppo.new_best()
    got = ppo.load_checkpoint(ppo.save_checkpoint(tmp_path / "fresh.npz", **st))
    assert got["best_return"].tolist() == [-np.inf] and got["best_iter"].tolist() == [-1]


def test_checkpoint_rejects_missing_wrong_and_pickled_fields(tmp_path):
    from dart_mpc._lib import DartMPCError
    st, ppo = _state()
    path = ppo.save_checkpoint(tmp_path / "c.npz", **st)
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    missing = {k: v for k, v in arrays.items() if k != "adam"}
    np.savez(tmp_path / "missing.npz", **missing)
    with pytest.raises(DartMPCError, match="adam"):
        ppo.load_checkpoint(tmp_path / "missing.npz")
    np.savez(tmp_path / "dtype.npz", **{**arrays, "critic": arrays["critic"].astype(np.float64)})
    with pytest.raises(DartMPCError, match="critic"):
        ppo.load_checkpoint(tmp_path / "dtype.npz")
    np.savez(tmp_path / "shape.npz", **{**arrays, "history": arrays["history"][:2]})
    with pytest.raises(DartMPCError, match="history"):
        ppo.load_checkpoint(tmp_path / "shape.npz")
    np.savez(tmp_path / "pickled.npz", **{**arrays, "actor": np.array([{"a": 1}], dtype=object)})
    with pytest.raises(DartMPCError):
        ppo.load_checkpoint(tmp_path / "pickled.npz")
    with pytest.raises(DartMPCError):
        ppo.load_checkpoint(tmp_path / "absent.npz")
    with pytest.raises(DartMPCError, match="actor"):
        ppo.save_checkpoint(tmp_path / "bad.npz", **{**st, "actor": st["actor"][:-1]})


def test_generator_statement_known_answers_and_keys():
    from dart_mpc import harness
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for c, k, w in kat:
        assert harness.philox4x32_10(c, k).tolist() == list(w)
    for n in (1, 5, 67, 257, 2304):
        perm, keys = harness.lmpc_train_perms(7, 0, 1, n)
        assert len(np.unique(keys[0])) == n and sorted(perm[0].tolist()) == list(range(n))
    assert harness.lmpc_train_perms(7, 0, 1, 5)[0].tolist() == [[1, 3, 2, 0, 4]]
    # ties break on the index
    assert np.lexsort((np.arange(4), np.array([5, 1, 5, 1], np.uint32))).tolist() == [1, 3, 0, 2]
    z = harness.lmpc_train_noise(7, 1, 32, 18)
    n = z.size
    assert z.shape == (32, 18, 34) and abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert abs(z.mean() + 0.0033) < 1e-4 and abs(z.var() - 1 + 0.014) < 1e-3
    # a tail uses the leading words of its block
    assert np.array_equal(harness.lmpc_train_noise(7, 1, 1, 1).reshape(-1), z.reshape(-1)[:34])


def test_mean_param_update_statement_matches_torch_restatement():
    """harness.lmpc_mean_param_update against rlmpc2.py:876-896 written with torch on the CPU (the policy module,
    torch.logit / torch.sigmoid on fp32 tensors, write_params_to_shm in numpy fp64)."""
    import torch
    from dart_mpc import harness, ppo
    from dart_mpc.lmpc import policy_config
    torch.manual_seed(3)
    net = ppo.PolicyNet()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    actor, _ = ppo.pack_weights(net)
    cfg = policy_config()
    rng = np.random.default_rng(4)
    Bn = 6
    history = rng.standard_normal((Bn, 520)).astype(np.float32)
    params = rng.uniform(cfg.min_k, cfg.k_max - cfg.k_ceiling_margin, (Bn, 34))
    params[0, :3] = [1e-4, cfg.k_max, cfg.k_max - 1e-9]                  # both clamps of the fraction
    mean, got = harness.lmpc_mean_param_update(actor, history, params, cfg)
    want = np.empty_like(params)
    with torch.no_grad():
        for b in range(Bn):
            mean_final, _, _ = net(torch.from_numpy(history[b]).unsqueeze(0))
            cur_k_t = torch.tensor(params[b], dtype=mean_final.dtype)
            frac = torch.clamp(cur_k_t / cfg.k_max, float(cfg.min_k / cfg.k_max), 1.0 - 1e-6)
            z_new = torch.logit(frac) + (mean_final * cfg.max_delta * cfg.action_scale).squeeze(0)
            k_final = (cfg.k_max * torch.sigmoid(z_new)).numpy().astype(np.float64)
            smoothed = cfg.smooth_alpha * k_final + (1 - cfg.smooth_alpha) * params[b]
            lo, hi = cfg.min_k, cfg.k_max - cfg.k_ceiling_margin
            center, scale = (hi + lo) / 2, (hi - lo) / 2 - 1e-3
            want[b] = center + scale * np.tanh((smoothed - center) / scale)
            assert np.allclose(mean[b], mean_final.numpy()[0], rtol=1e-5, atol=1e-6)
    d = float(np.max(np.abs(got - want)))
    print(f"mean parameter write, numpy against torch: max |d| {d:.3e}")
    assert d <= 1e-6 and np.max(np.abs(got - params)) > 1e-4
    assert (got > cfg.min_k).all() and (got < cfg.k_max - cfg.k_ceiling_margin).all()


def test_training_entries_validate_before_any_device_work():
    from dart_mpc import _lib
    L = _lib.lib()
    assert L.dart_lmpc_train_workspace_bytes(5, 31, 2, 2, 16) == 0          # K % record_every != 0
    assert L.dart_lmpc_train_workspace_bytes(5, 32, 2, 2, 2000) == 0
    assert L.dart_lmpc_train_workspace_bytes(0, 32, 2, 2, 16) == 0
    b = L.dart_lmpc_train_workspace_bytes(5, 32, 2, 2, 16)
    assert b > 32 * 5 * 34 * 4 + _lib.ppo_workspace_bytes(80, 16) and b % 256 == 0
    c = _lib.train_config()
    assert (c.seed, c.iterations, c.it0, c.steps, c.mean_update, c.track_best) == (0, 1, 0, 256, 1, 1)
    assert (c.gamma, c.lam) == (0.99, 0.95) and ctypes.sizeof(c) == 48
    with pytest.raises(_lib.DartMPCError):
        _lib.train_config(epochs=3)
    z = ctypes.c_void_p(0)
    assert L.dart_lmpc_train_dev(None, z, z, z, z, z, 5, 0, z, z) == -1
    assert L.dart_lmpc_train(None, z, z, z, z, z, 5, 0, z, z) == -1
    assert L.dart_lmpc_noise_dev(1, -1, 4, 4, z, z) == -1 and L.dart_lmpc_noise(1, 0, 4, 4, z) == -1
    assert L.dart_lmpc_noise_dev(1, 0, 0, 4, z, z) == 0                      # nothing to draw
    assert L.dart_lmpc_perms_dev(1, 0, 2, -1, z, z, z) == -1 and L.dart_lmpc_perms(1, 0, 2, 5, z, z) == -1
    assert L.dart_lmpc_philox_dev(3, z, z, z) == -1 and L.dart_lmpc_philox_dev(0, z, z, z) == 0
    assert L.dart_lmpc_mean_param_update_dev(z, 1, z, z, z, z, z, z) == -1
    assert L.dart_lmpc_mean_param_update(z, 1, z, z, z, z, z) == -1
    assert len(_lib.TRAIN_LOG_FIELDS) == _lib.TRAIN_LOG_COLS == 12
