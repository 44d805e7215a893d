"""The population training entries (dart_lmpc_train_pop*, added within ABI 8) without a GPU: symbols, workspace
sizes, the stacking helpers of dart_mpc.ppo, the sample-list formula and the stacked noise layout."""
import numpy as np
import pytest

P, B, K, EVERY, EPOCHS, MB = 3, 5, 32, 2, 2, 16


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


def test_symbols_and_abi(L):
    lib = L.lib()
    for name in ("dart_lmpc_train_pop_workspace_bytes", "dart_lmpc_train_pop_dev", "dart_lmpc_train_pop"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dart_mpc_abi_version() == 8 == L.ABI_VERSION
    assert L.POP_MAX == 32 and L.POP_CRITIC_STRIDE == 37572
    assert L.POP_CRITIC_STRIDE >= L.CRITIC_NWEIGHTS and (4 * L.POP_CRITIC_STRIDE) % 16 == 0
    assert hasattr(L.LmpcSolver, "train_pop_dev") and hasattr(L.LmpcSolver, "train_pop")


def test_workspace_bytes(L):
    bad = [(0, B, K), (L.POP_MAX + 1, B, K), (P, 0, K), (P, B, 25), (P, B, 0)]
    for p, b, k in bad:
        assert L.train_pop_workspace_bytes(p, b, k, EVERY, EPOCHS, MB) == 0, (p, b, k)
    assert L.train_pop_workspace_bytes(P, B, K, EVERY, EPOCHS, 0) == 0
    assert L.train_pop_workspace_bytes(P, B, K, EVERY, EPOCHS, 1025) == 0
    n = K // EVERY * B
    for p in (1, 2, 3, 8, L.POP_MAX):
        got = L.train_pop_workspace_bytes(p, B, K, EVERY, EPOCHS, MB)
        assert got > 0 and got % 256 == 0
        assert got >= p * L.ppo_workspace_bytes(n, MB) + 4 * K * p * B * 34
    # more learners never need less
    sizes = [L.train_pop_workspace_bytes(p, B, K, EVERY, EPOCHS, MB) for p in range(1, 9)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


# the shapes on which the layouts are compared: one instance, the tests', the benchmark's; one record row; epochs = 0
GRID = dict(B=(1, 5, 18, 72), K=(2, 24, 36, 256), every=(1, 2), epochs=(0, 1, 8), mb=(1, 16, 64), P=(1, 2, 3, 8))


def test_population_of_one_has_the_single_workspace(L):
    """The single iteration's workspace is the population's layout with one learner, block for block: the byte counts
    agree on the whole grid."""
    import itertools
    for b, k, every, epochs, mb in itertools.product(*(GRID[q] for q in ("B", "K", "every", "epochs", "mb"))):
        one = L.train_workspace_bytes(b, k, every, epochs, mb)
        sizes = [L.train_pop_workspace_bytes(p, b, k, every, epochs, mb) for p in GRID["P"]]
        assert one > 0 and sizes[0] == one, (b, k, every, epochs, mb)
        assert sizes == sorted(set(sizes)) and all(q % 256 == 0 for q in sizes), (b, k, every, epochs, mb)


def _random_member(L, rng, nw=17):
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    f64 = lambda *s: rng.standard_normal(s)
    i32 = lambda *s: rng.integers(-5, 50, s).astype(np.int32)
    gen = {np.float32: f32, np.float64: f64, np.int32: i32}
    shape = lambda w: (B, nw) if w == "nw" else ((B, w) if w else (B,))
    return dict(target=f64(B, 8), plant_pvec=f64(B, 34),
                state={n: gen[dt](*shape(w)) for n, w, dt in L.LMPC_LOOP_STATE},
                cstate={n: gen[dt](*shape(w)) for n, w, dt in L.LMPC_COLLECT_STATE},
                adam=f32(2, 77317), adam_step=i32(1), current_k=f64(B, 34), weights=f32(L.ACTOR_NWEIGHTS),
                critic=f32(L.CRITIC_NWEIGHTS),
                best=dict(best_return=f64(1), best_weights=f32(77317), best_iter=i32(1)),
                pool={n: f64(2, B, w) for n, w, _ in L.LMPC_COLLECT_POOL})


def _flat(m):
    out = {}
    for k, v in m.items():
        if isinstance(v, dict):
            out.update({k + "." + kk: vv for kk, vv in v.items()})
        else:
            out[k] = v
    return out


def test_stack_and_member_are_inverse(L):
    from dart_mpc import ppo
    rng = np.random.default_rng(5)
    members = [_random_member(L, rng) for _ in range(P)]
    pop = ppo.population_stack(members)
    assert pop["target"].shape == (P * B, 8) and pop["weights"].shape == (P, L.ACTOR_NWEIGHTS)
    assert pop["critic"].shape == (P, L.POP_CRITIC_STRIDE) and pop["critic"].dtype == np.float32
    assert (pop["critic"][:, L.CRITIC_NWEIGHTS:] == 0).all()
    assert pop["adam"].shape == (P, 2, 77317) and pop["adam_step"].shape == (P,)
    assert pop["best"]["best_weights"].shape == (P, 77317) and pop["best"]["best_return"].shape == (P,)
    assert pop["pool"]["reset_x"].shape == (2, P * B, 8)
    for v in _flat(pop).values():
        assert v.flags.c_contiguous
    for l, m in enumerate(members):
        got, want = _flat(ppo.population_member(l, P, pop)), _flat(m)
        assert set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (l, k)
    # members are views: writing a member writes the population (the pool, which is only read, is a copy)
    m1 = ppo.population_member(1, P, pop)
    m1["adam_step"][0] = 1234
    m1["critic"][3] = 7.5
    m1["state"]["x"][2, 0] = -9.0
    assert pop["adam_step"][1] == 1234 and pop["critic"][1, 3] == 7.5 and pop["state"]["x"][B + 2, 0] == -9.0
    # stacking the members again gives the population back
    again = _flat(ppo.population_stack([ppo.population_member(l, P, pop) for l in range(P)]))
    for k, v in _flat(pop).items():
        assert np.array_equal(again[k], v), k
    with pytest.raises(L.DartMPCError):
        ppo.population_member(P, P, pop)
    assert ppo.new_population_best(P)["best_return"].tolist() == [-np.inf] * P


def test_sample_lists(L):
    from dart_mpc import ppo
    R = K // EVERY
    got = ppo.population_samples(P, B, R)
    assert got.shape == (P, R * B) and got.dtype == np.int32
    rec = np.arange(R * P * B).reshape(R, P * B)                # a record array that holds its own flat index
    for l in range(P):
        want = rec[:, l * B:(l + 1) * B].reshape(-1)            # the single run's order r B + b on the learner's block
        assert np.array_equal(got[l], want)
        assert np.array_equal(rec.reshape(-1)[got[l]], want)
    assert np.array_equal(np.sort(got.reshape(-1)), np.arange(R * P * B))      # a partition of all records
    assert np.array_equal(ppo.population_samples(1, B, R)[0], np.arange(R * B))


def test_stacked_noise_layout(L):
    """P = 2, B = 3, K = 2: element (k, b, j) of learner l is flat element (k B + b) 34 + j of the generator of
    seeds[l], stored at [k][l B + b][j]."""
    from dart_mpc import harness, ppo
    seeds, p, b, k, it = (7, 2 ** 40 + 3), 2, 3, 2, 1
    got = ppo.population_noise(seeds, it, k, b)
    assert got.shape == (k, p * b, 34) and got.dtype == np.float32
    n = k * b * 34
    f = np.float32
    for l, seed in enumerate(seeds):
        blocks = np.arange((n + 3) // 4, dtype=np.uint64)
        w = harness.philox4x32_10((blocks, it, 0, 0), (seed & 0xffffffff, seed >> 32)).reshape(-1)
        u = ((w >> np.uint32(9)).astype(f) + f(0.5)) * f(2.0 ** -23)
        rad, ang = np.sqrt(f(-2.0) * np.log(u[0::2])), f(2.0 * np.pi) * u[1::2]
        z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).astype(f).reshape(-1)[:n]
        for kk in range(k):
            for bb in range(b):
                for j in (0, 1, 33):
                    assert got[kk, l * b + bb, j] == z[(kk * b + bb) * 34 + j]
        assert np.array_equal(got[:, l * b:(l + 1) * b].reshape(-1), z)
    assert not np.array_equal(got[:, :b], got[:, b:])
