"""The host side of the global-buffer update of the device-resident LMPC training (no GPU): the numpy statements of
the sequence GAE and of the choice without replacement (harness), the row arithmetic of the buffer, the argument
checks of the new entries that return before any device work, and the checkpoint format with a buffer."""
import ctypes

import numpy as np
import pytest


def _compute_gae(rewards, values, dones, last_value, gamma, lam):
    """compute_gae (rlmpc2.py:592-599) transcribed on Python lists."""
    adv = [0.0] * len(rewards)
    gae = 0.0
    vals = list(values) + [last_value]
    for t in reversed(range(len(rewards))):
        nonterminal = 1.0 - dones[t]
        delta = rewards[t] + gamma * vals[t + 1] * nonterminal - vals[t]
        gae = delta + gamma * lam * nonterminal * gae
        adv[t] = gae
    return adv, [a + v for a, v in zip(adv, values)]


@pytest.mark.parametrize("G", [1, 2, 65, 300])
def test_gae_sequence_is_compute_gae(G):
    from dart_mpc import harness
    rng = np.random.default_rng(G)
    reward = rng.standard_normal(G)
    value = rng.standard_normal(G).astype(np.float32)
    done = (rng.random(G) < 0.1).astype(np.float32)
    done[-1] = 1.0 if G % 2 else 0.0
    last = np.float32(0.37)
    adv, ret = harness.gae_sequence(reward, value, done, [last], 0.99, 0.95)
    want_adv, want_ret = _compute_gae(reward.tolist(), [float(v) for v in value], [float(d) for d in done],
                                      float(last), 0.99, 0.95)
    assert adv.tolist() == want_adv and ret.tolist() == want_ret
    mag, _ = harness.gae_sequence(reward, value, done, [last], 0.99, 0.95, magnitude=True)
    assert (mag >= np.abs(adv)).all() and (mag >= 0).all()


def test_choice_statement_is_a_prefix_of_the_stream_2_permutation():
    from dart_mpc import harness
    for n, m in ((1, 1), (3, 1), (5, 1), (67, 16), (257, 64), (2304, 576)):
        for seed, it in ((7, 0), (2 ** 40 + 3, 5)):
            keys = harness.lmpc_train_words(seed, it, 2, 0, n)
            perm = np.lexsort((np.arange(n), keys))
            got = harness.lmpc_train_choice(seed, it, n, m)
            assert got.dtype == np.int32 and got.tolist() == perm[:m].tolist()
            assert len(set(got.tolist())) == m and got.min() >= 0 and got.max() < n
    # another stream than the permutations' and the noise's
    assert not np.array_equal(harness.lmpc_train_words(7, 0, 2, 0, 8), harness.lmpc_train_words(7, 0, 1, 0, 8))
    assert not np.array_equal(harness.lmpc_train_words(7, 0, 2, 0, 8), harness.lmpc_train_words(7, 0, 3, 0, 8))
    with pytest.raises(ValueError):
        harness.lmpc_train_choice(7, 0, 4, 5)
    with pytest.raises(ValueError):
        harness.lmpc_train_choice(7, 0, 4, 0)


def test_global_rows_and_fill_arithmetic():
    from dart_mpc import _lib
    for n, m, G in ((1, 1, 1), (3, 1, 3), (80, 20, 80), (60, 15, 60), (90, 22, 110), (2304, 576, 2304)):
        assert _lib.global_rows(n) == (m, G)
        period = -(-n // m)
        assert G == period * m and G >= n
        # the fill chains: a + b iterations are a, then b; one period returns to the start
        fill, seen = 0, []
        for _ in range(2 * period + 1):
            seen.append(fill)
            nxt = fill + m
            fill = 0 if nxt >= n else nxt
            assert _lib.global_fill_after(n, seen[-1], 1) == fill
        for a in range(period + 2):
            for b in range(period + 2):
                assert _lib.global_fill_after(n, _lib.global_fill_after(n, 0, a), b) == _lib.global_fill_after(n, 0, a + b)
        assert _lib.global_fill_after(n, 0, period) == 0 and _lib.global_fill_after(n, 0, 0) == 0
    L = _lib.lib()
    assert L.dart_lmpc_global_fill_after(80, 10, 1) == -1          # not a multiple of m
    assert L.dart_lmpc_global_fill_after(80, 80, 1) == -1 and L.dart_lmpc_global_fill_after(80, -20, 1) == -1
    assert L.dart_lmpc_global_fill_after(0, 0, 1) == -1 and L.dart_lmpc_global_fill_after(80, 0, -1) == -1
    m, G = ctypes.c_int32(), ctypes.c_int32()
    assert L.dart_lmpc_global_rows(0, ctypes.byref(m), ctypes.byref(G)) == -1
    assert L.dart_lmpc_global_rows(4, None, ctypes.byref(G)) == -1
    with pytest.raises(_lib.DartMPCError):
        _lib.global_fill_after(80, 10, 1)
    # the workspace holds the update's own and the sequence's arrays
    b = L.dart_lmpc_global_workspace_bytes(90, 2, 16)
    assert b % 256 == 0 and b > _lib.ppo_workspace_bytes(110, 16) + 110 * (8 + 8 + 4 + 2 * 4) + 22 * 4
    assert L.dart_lmpc_global_workspace_bytes(0, 2, 16) == 0 and L.dart_lmpc_global_workspace_bytes(90, -1, 16) == 0
    assert L.dart_lmpc_global_workspace_bytes(90, 2, 2000) == 0
    assert len(_lib.GLOBAL_LOG_FIELDS) == _lib.GLOBAL_LOG_COLS == 6
    assert ctypes.sizeof(_lib.GlobalBuffer) == 72
    assert ctypes.sizeof(_lib.train_config()) == 48 and _lib.TRAIN_LOG_COLS == 12      # ABI 8 as it was


def test_population_of_one_has_the_single_global_workspace():
    """The single global update's workspace is the population's layout with one learner and capacity G, block for
    block: the byte counts agree on the grid of tests/test_lmpc_population_host.py (n = K / record_every B)."""
    import itertools
    from dart_mpc import _lib
    from test_lmpc_population_host import GRID
    for b, k, every, epochs, mb in itertools.product(*(GRID[q] for q in ("B", "K", "every", "epochs", "mb"))):
        n = k // every * b
        G = _lib.global_rows(n)[1]
        one = _lib.global_workspace_bytes(n, epochs, mb)
        sizes = [_lib.global_pop_workspace_bytes(p, n, G, epochs, mb) for p in GRID["P"]]
        assert one > 0 and sizes[0] == one, (n, G, epochs, mb)
        assert sizes == sorted(set(sizes)) and all(q % 256 == 0 for q in sizes), (n, G, epochs, mb)
        assert _lib.global_pop_workspace_bytes(1, n, G + 3, epochs, mb) >= one       # spare capacity never needs less


def test_global_entries_validate_before_any_device_work():
    from dart_mpc import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    one = np.zeros(8, np.int32)
    p1 = ctypes.c_void_p(one.ctypes.data)
    # choice: m < 1, m > n, null pointer, negative iteration
    for fn, tail in ((L.dart_lmpc_choice_dev, (z,)), (L.dart_lmpc_choice, ())):
        assert fn(1, 0, 5, 0, p1, *tail) == -1 and fn(1, 0, 5, 6, p1, *tail) == -1
        assert fn(1, 0, 5, 2, z, *tail) == -1 and fn(1, -1, 5, 2, p1, *tail) == -1
    assert L.dart_lmpc_perms_stream_dev(1, 0, -1, 2, 5, p1, z, z) == -1
    assert L.dart_lmpc_perms_stream_dev(1, 0, 3, 2, 5, z, z, z) == -1
    assert L.dart_lmpc_perms_stream_dev(1, 0, 3, 0, 5, z, z, z) == 0          # nothing to draw
    # sequence GAE: negative size, null pointers; nothing to do at G = 0
    for fn, tail in ((L.dart_lmpc_gae_seq_dev, (z,)), (L.dart_lmpc_gae_seq, ())):
        assert fn(-1, 0.99, 0.95, z, z, z, z, z, z, *tail) == -1
        assert fn(4, 0.99, 0.95, z, z, z, z, z, z, *tail) == -1
        assert fn(0, 0.99, 0.95, z, z, z, z, z, z, *tail) == 0
    # append: host arrays stand in for the pointers (no entry gets as far as reading them)
    cap = 8
    arr = {name: np.zeros((cap, max(w, 1)), dt) for name, w, dt in _lib.LMPC_GLOBAL_ARRAYS}
    rec = [np.zeros((4, max(w, 1)), dt) for _, w, dt in _lib.LMPC_COLLECT_REC]
    rp = [ctypes.c_void_p(a.ctypes.data) for a in rec]
    sample, choice = np.arange(4, dtype=np.int32), np.array([1, 3], np.int32)
    sp, cp = ctypes.c_void_p(sample.ctypes.data), ctypes.c_void_p(choice.ctypes.data)

    def gb(fill=0, capacity=cap, **over):
        ptrs = {k: v.ctypes.data for k, v in arr.items()}
        ptrs.update(over)
        return _lib.global_buffer(ptrs, capacity, fill)

    for fn, tail in ((L.dart_lmpc_global_append_dev, (z,)), (L.dart_lmpc_global_append, ())):
        assert fn(None, 2, 4, 4, sp, cp, *rp, *tail) == -1
        assert fn(ctypes.byref(gb(fill=7)), 2, 4, 4, sp, cp, *rp, *tail) == -1          # fill + m > capacity
        assert fn(ctypes.byref(gb(fill=-1)), 2, 4, 4, sp, cp, *rp, *tail) == -1
        assert fn(ctypes.byref(gb()), 0, 4, 4, sp, cp, *rp, *tail) == -1                # m < 1
        assert fn(ctypes.byref(gb()), 2, 4, 4, z, cp, *rp, *tail) == -1
        assert fn(ctypes.byref(gb()), 2, 4, 4, sp, cp, *rp[:3], z, *rp[4:], *tail) == -1
        assert fn(ctypes.byref(gb(reward=0)), 2, 4, 4, sp, cp, *rp, *tail) == -1
    assert L.dart_lmpc_global_append_dev(ctypes.byref(gb(obs=arr["obs"].ctypes.data + 4)), 2, 4, 4, sp, cp, *rp, z) == -1
    bad = np.array([1, 4], np.int32)                                                    # a choice outside [0, n)
    assert L.dart_lmpc_global_append(ctypes.byref(gb()), 2, 4, 4, sp, ctypes.c_void_p(bad.ctypes.data), *rp) == -1
    assert L.dart_lmpc_global_append(ctypes.byref(gb()), 2, 4, 3, sp, cp, *rp) == -1    # a sample outside the records
    assert not any(a.any() for a in arr.values())
    # the training entries: no handle
    g = gb()
    assert L.dart_lmpc_train_global_dev(None, z, z, z, z, z, 5, 0, z, ctypes.byref(g), z) == -1
    assert L.dart_lmpc_train_global(None, z, z, z, z, z, 5, 0, z, ctypes.byref(g), z) == -1


def _state(B=3, seed=0):
    from dart_mpc import ppo
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    best = dict(best_return=np.array([rng.standard_normal()]), best_weights=f32(77317), best_iter=np.array([4], np.int32))
    return dict(actor=f32(39748), critic=f32(37569), adam=f32(2, 77317), adam_step=np.array([160], np.int32),
                best=best, iteration=7, obs_mean=rng.standard_normal((B, 52)), obs_M2=rng.random((B, 52)),
                obs_count=np.full(B, 1792, np.int32), history=f32(B, 520), current_k=rng.random((B, 34)) + 0.5,
                model_params=rng.random((B, 34)) + 0.5), ppo


def test_checkpoint_round_trip_with_and_without_a_buffer(tmp_path):
    from dart_mpc._lib import DartMPCError
    st, ppo = _state()
    buf = ppo.new_global_buffer(90)
    assert buf["fill"] == 0 and buf["obs"].shape == (110, 520) and buf["reward"].dtype == np.float64
    assert sorted(buf) == ["action", "done", "fill", "logp", "obs", "reward", "value"]
    rng = np.random.default_rng(5)
    for k in ("obs", "action", "logp", "value", "reward", "done"):
        buf[k][:44] = rng.standard_normal(buf[k][:44].shape)
    buf["logp"][3] = np.nan
    buf["fill"] = 44
    path = ppo.save_checkpoint(tmp_path / "with", global_buffer=buf, **st)
    with np.load(path, allow_pickle=False) as z:                 # plain arrays: opens without pickle
        assert sorted(z.files) == sorted(list(ppo.CHECKPOINT_FIELDS) + list(ppo.CHECKPOINT_GLOBAL_FIELDS))
    got = ppo.load_checkpoint(path)
    back = ppo.global_buffer_from_checkpoint(got)
    assert back["fill"] == 44
    for k in ("obs", "action", "logp", "value", "reward", "done"):
        assert back[k].dtype == buf[k].dtype and back[k].shape == buf[k].shape and back[k].tobytes() == buf[k].tobytes()
        assert back[k].flags.writeable and back[k] is not got["g_" + k]
    assert got["actor"].tobytes() == st["actor"].tobytes()
    # without a buffer: the file and the loaded dict are what they were
    plain = ppo.save_checkpoint(tmp_path / "plain", **st)
    with np.load(plain, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(ppo.CHECKPOINT_FIELDS)
        arrays = {k: z[k] for k in z.files}
    got = ppo.load_checkpoint(plain)
    assert sorted(got) == sorted(ppo.CHECKPOINT_FIELDS) and ppo.global_buffer_from_checkpoint(got) is None
    # an old-format file (written field by field, as before the buffer existed) still loads
    np.savez(tmp_path / "old.npz", **arrays)
    old = ppo.load_checkpoint(tmp_path / "old.npz")
    assert sorted(old) == sorted(ppo.CHECKPOINT_FIELDS) and old["adam"].tobytes() == st["adam"].tobytes()
    # a buffer that is there in part, or of the wrong type, is refused
    with np.load(path, allow_pickle=False) as z:
        full = {k: z[k] for k in z.files}
    np.savez(tmp_path / "part.npz", **{k: v for k, v in full.items() if k != "g_reward"})
    with pytest.raises(DartMPCError, match="g_reward"):
        ppo.load_checkpoint(tmp_path / "part.npz")
    np.savez(tmp_path / "dtype.npz", **{**full, "g_obs": full["g_obs"].astype(np.float64)})
    with pytest.raises(DartMPCError, match="g_obs"):
        ppo.load_checkpoint(tmp_path / "dtype.npz")
    np.savez(tmp_path / "shape.npz", **{**full, "g_done": full["g_done"][:5]})
    with pytest.raises(DartMPCError, match="g_done"):
        ppo.load_checkpoint(tmp_path / "shape.npz")
    with pytest.raises(DartMPCError, match="g_fill"):
        ppo.save_checkpoint(tmp_path / "bad.npz", global_buffer={**buf, "fill": 111}, **st)
