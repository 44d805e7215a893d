"""Argument checks of the LMPC closed-loop entries (csrc/dart_mpc_rollout.hip lmpc_loop_check / lmpc_closed_loop,
csrc/dart_mpc_train.hip train_check and the training entries): dart_lmpc_rollout, _rollout_dev, _collect,
_collect_dev, dart_lmpc_train and _train_dev on one LMPC handle with B = 2, N = 4, steps = 2, record_every = 1 and
reset_rows = 1.

Every case is a row of a table: the entry, what is wrong with the call, and the exact dart_mpc_last_error text.  The
texts and their order (which of two mistakes is reported) are those of the single-file ABI layer before it was split;
each error returns DART_MPC_EINVAL before any launch.  The two rollout entries also run once with weights == NULL and
every policy-state pointer NULL, which must succeed.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, BCAP, N, STEPS, EVERY, RESET = 2, 3, 4, 2, 1, 1
ROWS, REC = STEPS, STEPS // EVERY
EINVAL = -1

M_NULL = "null pointer"
M_POLICY = "null pointer (policy state)"
M_COLLECT = "null pointer (collection state or logs)"
M_REC = "null pointer (records)"
M_POOL = "reset_rows > 0 with a null reset pool"
M_TRAIN = "null pointer (training arrays)"
M_VARIANT = "handle is not an LMPC handle"
M_BMAX = "batch larger than B_max"
M_ROWS = "k0 + steps exceeds log_rows"
M_ALIGN = "policy and critic weights must be 16-byte aligned"
M_NOPOLICY = "experience collection needs a policy (null weights)"
M_CRITIC = "null critic weights"
M_PCFG = "bad policy config"
M_RCFG = "null reward config"
M_PLANT = "null plant config"
M_TCFG = "null training config, reward config or buffers"
M_PPO = "bad PPO config"


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _groups(L):
    """name -> (shape after the leading B or [rows, B], dtype, leading rows, group) for every array of the entries."""
    nw = 8 * (N + 1) + 2 * N
    G = {"target": ((BCAP, 8), np.float64, "loop"), "prm": ((BCAP, 22), np.float64, "loop"),
         "plant_pvec": ((BCAP, 34), np.float64, "loop"), "current_k": ((BCAP, 34), np.float64, "policy"),
         "weights": ((L.ACTOR_NWEIGHTS + 8,), np.float32, "weights"), "critic": ((L.CRITIC_NWEIGHTS,), np.float32, "critic"),
         "noise": ((ROWS, BCAP, 34), np.float32, "noise")}
    for name, w, dt in L.LMPC_LOOP_STATE:
        grp = "loop" if name in ("x", "tilt", "u_prev", "w", "model_params") else "policy"
        G[name] = ((BCAP, nw if w == "nw" else max(w, 1)), dt, grp)
    for name, w, dt in L.LMPC_COLLECT_STATE:
        G[name] = ((BCAP, max(w, 1)), dt, "collect")
    for name, w, dt in L.LMPC_COLLECT_POOL:
        G[name] = ((RESET, BCAP, w), dt, "pool")
    for name, w, dt in L.LMPC_LOOP_LOGS:
        G["log_" + name] = ((ROWS, BCAP, max(w, 1)), dt, "loop")
    for name, w, dt in L.LMPC_COLLECT_LOGS:
        G["log_" + name] = ((ROWS, BCAP, max(w, 1)), dt, "collect")
    for name, w, dt in L.LMPC_COLLECT_REC:
        G[name] = ((REC, BCAP, max(w, 1)), dt, "rec")
    G.update(adam=((2 * L.PPO_NPARAMS,), np.float32, "train"), adam_step=((1,), np.int32, "train"),
             train_log=((1, L.TRAIN_LOG_COLS), np.float64, "train"), best_return=((1,), np.float64, "train"),
             best_weights=((L.PPO_NPARAMS,), np.float32, "train"), best_iter=((1,), np.int32, "train"))
    return G


def _order(L):
    state = [n for n, _, _ in L.LMPC_LOOP_STATE]
    cstate = [n for n, _, _ in L.LMPC_COLLECT_STATE]
    pool = [n for n, _, _ in L.LMPC_COLLECT_POOL]
    logs = ["log_" + n for n, _, _ in L.LMPC_LOOP_LOGS]
    clogs = ["log_" + n for n, _, _ in L.LMPC_COLLECT_LOGS]
    rec = [n for n, _, _ in L.LMPC_COLLECT_REC]
    rollout = ["target", "prm", "plant_pvec", "current_k", "weights", "noise"] + state + logs
    collect = ["target", "prm", "plant_pvec", "current_k", "weights", "critic", "noise"] + state + cstate + pool + logs \
        + clogs + rec
    train = ["target", "prm", "plant_pvec", "current_k", "weights", "critic"] + state + cstate + pool + logs + clogs \
        + rec + ["adam", "adam_step", "train_log", "best_return", "best_weights", "best_iter", "workspace"]
    return dict(rollout=rollout, collect=collect, train=train)


class _Bench:
    """The handles, the configs and one set of host and one of device arrays, shared by every case."""

    def __init__(self, L, torch):
        from dart_mpc.lmpc import LmpcPolicy
        from dart_mpc.workload import lmpc_batch
        self.L, self.lib = L, L.lib()
        self.s = L.LmpcSolver(N=N, B_max=B)
        self.pmpc = L.Solver(N=N, B_max=B)
        self.G, self.order = _groups(L), _order(L)
        D = lmpc_batch(3)
        pol = LmpcPolicy(BCAP, seed=0)
        host = {}
        for name, (shape, dt, _) in self.G.items():
            # (16-byte aligned whatever numpy's allocator does: the alignment cases offset by 4 bytes)
            raw = np.zeros(int(np.prod(shape)) * np.dtype(dt).itemsize + 16, np.uint8)
            off = (-raw.ctypes.data) % 16
            host[name] = raw[off:off + raw.size - 16].view(dt).reshape(shape)
        host["target"][:] = D["target"][:BCAP]
        host["plant_pvec"][:] = D["pvec"][:BCAP]
        host["model_params"][:] = D["pvec"][:BCAP]
        host["x"][:] = D["state"][:BCAP]
        host["prm"][:] = L.LMPC_PRM_DEFAULT
        host["current_k"][:] = pol.current_k
        host["weights"][:L.ACTOR_NWEIGHTS] = pol.weights
        host["best_return"][:] = -np.inf
        self.host = host
        self.dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}
        ws = L.train_workspace_bytes(B, STEPS, EVERY, 1, 4)
        self.dev["workspace"] = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        self.plant = L.plant_config()
        self.pcfg = pol.cfg
        self.rcfg = L.reward_config(record_every=EVERY)
        self.ppo = L.ppo_config(epochs=1, mini_batch_size=4)
        self.tcfg = L.train_config(iterations=1, steps=STEPS)

    def ptrs(self, dev):
        if dev:
            return {k: v.data_ptr() for k, v in self.dev.items()}
        p = {k: v.ctypes.data for k, v in self.host.items()}
        p["workspace"] = 0
        return p

    def call(self, entry, dev, null=(), handle=None, nB=B, k0=0, cfgs=None, offset=None):
        """Calls `entry` ("rollout", "collect" or "train"; `dev`: its _dev form) with the pointers named in `null`
        zeroed; `cfgs` overrides config pointers by name; `offset` = (name, bytes) moves one pointer.  Returns the
        code and the handle's error text."""
        h = (handle or self.s)._h
        p = self.ptrs(dev)
        for n in null:
            p[n] = 0
        if offset:
            p[offset[0]] += offset[1]
        c = dict(plant=ctypes.addressof(self.plant), pcfg=ctypes.addressof(self.pcfg), rcfg=ctypes.addressof(self.rcfg),
                 ppo=ctypes.addressof(self.ppo), tcfg=ctypes.addressof(self.tcfg))
        c.update(cfgs or {})
        v = lambda q: ctypes.c_void_p(q) if q else None
        args = [v(p[n]) for n in self.order[entry]]
        suffix = "_dev" if dev else ""
        if entry == "rollout":
            rc = getattr(self.lib, "dart_lmpc_rollout" + suffix)(h, v(c["plant"]), v(c["pcfg"]), nB, k0, STEPS, ROWS,
                                                                  *args, None)
        elif entry == "collect":
            rc = getattr(self.lib, "dart_lmpc_collect" + suffix)(h, v(c["plant"]), v(c["pcfg"]), v(c["rcfg"]), nB, k0,
                                                                  STEPS, ROWS, REC, RESET, *args, None)
        else:
            buf = self.L._train_buffers([q.value if q is not None else 0 for q in args])
            buf = None if "buffers" in null else buf
            rc = getattr(self.lib, "dart_lmpc_train" + suffix)(h, v(c["plant"]), v(c["pcfg"]), v(c["rcfg"]), v(c["ppo"]),
                                                                v(c["tcfg"]), nB, RESET, buf, None)
        msg = self.lib.dart_mpc_last_error(h)
        return rc, msg.decode() if msg else ""


@pytest.fixture(scope="module")
def bench(L, torch):
    b = _Bench(L, torch)
    yield b
    torch.cuda.synchronize()


ENTRIES = [(e, d) for e in ("rollout", "collect", "train") for d in (False, True)]


def _null_message(entry, dev, group):
    """The text for one null array of `group`, as the entry's order of checks has it."""
    if group == "train":
        return M_TRAIN
    if entry == "train":
        if group in ("weights", "critic"):
            return M_TRAIN
        if group == "pool":
            return M_POOL
        if not dev:
            return M_NULL                               # the host entry checks the union of the groups at once
    return {"loop": M_NULL, "policy": M_POLICY, "collect": M_COLLECT, "rec": M_REC, "pool": M_POOL,
            "weights": M_NOPOLICY, "critic": M_CRITIC}[group]


@pytest.mark.parametrize("entry,dev", ENTRIES)
def test_one_null_pointer_at_a_time(bench, entry, dev):
    for name in bench.order[entry]:
        if name == "noise" or (entry == "rollout" and name == "weights"):
            continue                                    # optional: zero noise, no policy (test_rollout_without_policy)
        if name == "workspace":
            if not dev:
                continue                                # the host entry makes its own
            want = M_TRAIN
        else:
            group = bench.G[name][2]
            # training checks current_k with its own arrays, ahead of the collection's checks
            want = M_TRAIN if (entry == "train" and name == "current_k") else _null_message(entry, dev, group)
        rc, msg = bench.call(entry, dev, null=(name,))
        print(f"{entry}{'_dev' if dev else ''}: {name} = NULL -> {rc} {msg!r}")
        assert (rc, msg) == (EINVAL, want), name


@pytest.mark.parametrize("entry,dev", ENTRIES)
def test_config_pointers_and_shapes(bench, entry, dev):
    cases = [("wrong variant", dict(handle=bench.pmpc), M_VARIANT),
             ("B > B_max", dict(nB=B + 1), M_BMAX),
             ("null plant", dict(cfgs=dict(plant=0)), M_PLANT),
             ("null policy config", dict(cfgs=dict(pcfg=0)), M_PCFG)]
    if entry != "train":
        cases.append(("k0 + steps > log_rows", dict(k0=1), M_ROWS))
    if entry != "rollout":
        cases.append(("null reward config", dict(cfgs=dict(rcfg=0)), M_TCFG if entry == "train" else M_RCFG))
        cases.append(("null pool", dict(null=("reset_x", "reset_target", "reset_pvec")), M_POOL))
    if entry == "collect" or (entry == "train" and dev):
        cases.append(("misaligned weights", dict(offset=("weights", 4)), M_ALIGN))
    if entry == "train":
        cases += [("null training config", dict(cfgs=dict(tcfg=0)), M_TCFG), ("null buffers", dict(null=("buffers",)), M_TCFG),
                  ("null PPO config", dict(cfgs=dict(ppo=0)), M_PPO)]
    # two mistakes: the earlier check speaks
    cases.append(("wrong variant and a null array", dict(handle=bench.pmpc, null=("x",)),
                  M_VARIANT))
    cases.append(("B > B_max and a null array", dict(nB=B + 1, null=("x",)), M_BMAX))
    if entry == "collect":
        cases.append(("null loop array and null record", dict(null=("log_X", "rec_obs")), M_NULL))
        cases.append(("null collection array and null pool", dict(null=("nrec", "reset_x")), M_COLLECT))
        cases.append(("misaligned weights and a null array", dict(offset=("weights", 4), null=("x",)), M_ALIGN))
    for what, kw, want in cases:
        rc, msg = bench.call(entry, dev, **kw)
        print(f"{entry}{'_dev' if dev else ''}: {what} -> {rc} {msg!r}")
        assert (rc, msg) == (EINVAL, want), what


@pytest.mark.parametrize("dev", [False, True])
def test_rollout_without_policy(bench, torch, dev):
    """weights == NULL: the loop runs without a policy, and none of the policy-state pointers is looked at."""
    policy_state = [n for n, (_, _, g) in bench.G.items() if g == "policy"]
    rc, msg = bench.call("rollout", dev, null=["weights", "noise"] + policy_state, cfgs=dict(pcfg=0))
    torch.cuda.synchronize()
    print(f"rollout{'_dev' if dev else ''} without a policy -> {rc} {msg!r}")
    assert rc == 0
    log_X = bench.dev["log_X"].cpu().numpy() if dev else bench.host["log_X"]
    assert np.isfinite(log_X).all() and np.any(log_X != 0.0)           # (prefilled with zeros: the loop wrote its rows)
