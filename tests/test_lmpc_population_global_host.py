"""The population form of the global-buffer update (dart_lmpc_train_pop_global*, added within ABI 8) without a GPU:
symbols, the workspace size, the stacked buffers of dart_mpc.ppo and the training tool's option check."""
import os
import subprocess
import sys

import numpy as np
import pytest

P, B, K, EVERY, EPOCHS, MB = 3, 5, 32, 2, 2, 16
N_ = K // EVERY * B             # 80 samples per learner and iteration: m = 20, G = 80
FIELDS = ("obs", "action", "logp", "value", "reward", "done")


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


def test_symbols_and_abi(L):
    lib = L.lib()
    for name in ("dart_lmpc_global_pop_workspace_bytes", "dart_lmpc_train_pop_global_dev", "dart_lmpc_train_pop_global",
                 "dart_lmpc_choice_pop_dev", "dart_lmpc_global_append_pop_dev", "dart_lmpc_gae_seq_pop_dev"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dart_mpc_abi_version() == 8 == L.ABI_VERSION
    assert hasattr(L.LmpcSolver, "train_pop_global_dev")


def test_new_population_global_buffer(L):
    from dart_mpc import ppo
    m, G = L.global_rows(N_)
    assert (m, G) == (20, 80)
    buf = ppo.new_population_global_buffer(P, N_)
    assert set(buf) == set(FIELDS) | {"fill"} and buf["fill"] == 0
    for name, width, dt in L.LMPC_GLOBAL_ARRAYS:
        a = buf[name]
        assert a.shape == ((P, G, width) if width else (P, G)) and a.dtype == dt and a.flags.c_contiguous
        assert not a.any()
    # n = 90: G = 110 > n
    assert ppo.new_population_global_buffer(2, 90)["obs"].shape == (2, 110, 520)
    for bad in (0, L.POP_MAX + 1):
        with pytest.raises(L.DartMPCError):
            ppo.new_population_global_buffer(bad, N_)


def _members(L, rng, fills=(40, 40, 40), caps=(80, 80, 80)):
    from test_lmpc_population_host import _random_member
    out = []
    for fill, cap in zip(fills, caps):
        m = _random_member(L, rng)
        m["global_buffer"] = dict({name: (rng.standard_normal((cap, w) if w else (cap,))).astype(dt)
                                   for name, w, dt in L.LMPC_GLOBAL_ARRAYS}, fill=fill)
        out.append(m)
    return out


def test_stack_and_member_are_inverse_on_the_buffer(L):
    from dart_mpc import ppo
    rng = np.random.default_rng(11)
    members = _members(L, rng)
    pop = ppo.population_stack(members)
    gb = pop["global_buffer"]
    assert gb["fill"] == 40 and gb["obs"].shape == (P, 80, 520) and gb["reward"].dtype == np.float64
    assert all(gb[f].flags.c_contiguous for f in FIELDS)
    for l, m in enumerate(members):
        got = ppo.population_member(l, P, pop)["global_buffer"]
        assert got["fill"] == 40 and set(got) == set(m["global_buffer"])
        for name, w, dt in L.LMPC_GLOBAL_ARRAYS:
            a, b = got[name], m["global_buffer"][name]
            assert a.shape == b.shape == ((80, w) if w else (80,)) and a.dtype == dt and a.flags.c_contiguous
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (l, name)
    # the member's buffer is a view: a write through it shows in the stack
    g1 = ppo.population_member(1, P, pop)["global_buffer"]
    g1["obs"][7, 3] = -9.0
    g1["reward"][79] = 123.0
    assert gb["obs"][1, 7, 3] == -9.0 and gb["reward"][1, 79] == 123.0 and gb["obs"][0, 7, 3] != -9.0
    # stacking the members again gives the population's buffer back
    again = ppo.population_stack([ppo.population_member(l, P, pop) for l in range(P)])["global_buffer"]
    assert again["fill"] == 40 and all(np.array_equal(again[f], gb[f]) for f in FIELDS)
    # a population without buffers has no such key, in the stack or in a member
    plain = ppo.population_stack([{k: v for k, v in m.items() if k != "global_buffer"} for m in members])
    assert "global_buffer" not in plain and "global_buffer" not in ppo.population_member(0, P, plain)


def test_unequal_fill_or_capacity_is_refused(L):
    from dart_mpc import ppo
    rng = np.random.default_rng(12)
    with pytest.raises(L.DartMPCError, match="fill"):
        ppo.population_stack(_members(L, rng, fills=(40, 20, 40)))
    with pytest.raises(L.DartMPCError, match="capacity"):
        ppo.population_stack(_members(L, rng, caps=(80, 80, 83)))
    some = _members(L, rng)
    del some[2]["global_buffer"]
    with pytest.raises(L.DartMPCError):
        ppo.population_stack(some)


def test_global_pop_workspace_bytes(L):
    m, G = L.global_rows(N_)
    got = L.global_pop_workspace_bytes(P, N_, G, EPOCHS, MB)
    assert got > 0 and got % 256 == 0
    # at least: P update workspaces, adv and ret [P][capacity], the sample lists and the permutations
    assert got >= P * L.ppo_workspace_bytes(G, MB) + P * G * (8 + 8 + 4 + 4 * EPOCHS)
    for p, n, cap in ((0, N_, G), (L.POP_MAX + 1, N_, G), (P, 0, G), (P, N_, G - 1)):
        assert L.global_pop_workspace_bytes(p, n, cap, EPOCHS, MB) == 0, (p, n, cap)
    assert L.global_pop_workspace_bytes(P, N_, G, EPOCHS, 0) == 0
    assert L.global_pop_workspace_bytes(P, N_, G, EPOCHS, 1025) == 0
    sizes = [L.global_pop_workspace_bytes(p, N_, G, EPOCHS, MB) for p in range(1, 9)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)           # monotone in P
    assert L.global_pop_workspace_bytes(P, N_, G + 3, EPOCHS, MB) >= got      # and it depends on the capacity
    # n = 90: G = 110
    assert L.global_pop_workspace_bytes(P, 90, 110, EPOCHS, MB) > 0 == L.global_pop_workspace_bytes(P, 90, 109, EPOCHS, MB)


def test_training_tool_refuses_population_global_without_resident():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "lmpc_train.py"), "1", "--population", "2",
                        "--global-update", "--update", "torch"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "goes with --update resident" in r.stderr
