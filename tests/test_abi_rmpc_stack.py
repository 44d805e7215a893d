"""The RMPC stack entries of include/dart_mpc.h (added within ABI 8): symbols, argument tables, and every argument check,
all of which return DART_MPC_EINVAL before any HIP call.  The checks that need no handle run without a GPU; a handle
exists only on a device, so the checks behind one are marked gpu -- they launch nothing: every call is refused, and the
arrays it was given are unchanged afterwards."""
import ctypes

import numpy as np
import pytest

ENTRIES = ("dart_rmpc_stack_loop_step_dev", "dart_rmpc_stack_lm_loop_step_dev", "dart_rmpc_stack_rollout_dev",
           "dart_rmpc_stack_lm_rollout_dev", "dart_rmpc_stack_rollout", "dart_rmpc_stack_lm_rollout")
EINVAL = -1


def test_symbols_and_tables():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in ENTRIES:
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    assert L.dart_mpc_abi_version() == 8 == _lib.ABI_VERSION
    assert [name for name, _, _ in _lib.RMPC_STACK_LOGS] == ["U_cmd", "quat_tray", "tilt", "tray"]
    # the binding's argument tables cover the entries' pointer arguments
    for lm in (False, True):
        step = getattr(L, "dart_rmpc_stack_lm_loop_step_dev" if lm else "dart_rmpc_stack_loop_step_dev")
        roll = getattr(L, "dart_rmpc_stack_lm_rollout_dev" if lm else "dart_rmpc_stack_rollout_dev")
        host = getattr(L, "dart_rmpc_stack_lm_rollout" if lm else "dart_rmpc_stack_rollout")
        nlog = len(_lib.RMPC_LM_LOOP_LOGS if lm else _lib.RMPC_LOOP_LOGS) + len(_lib.RMPC_STACK_LOGS)
        assert len(step.argtypes) == 4 + 7 + len(_lib.RMPC_STACK_STEP_ARGS[lm]) + nlog + 1
        assert len(roll.argtypes) == 6 + 6 + len(_lib.RMPC_STACK_ROLLOUT_ARGS[lm]) + nlog + len(_lib.ARM_LOOP_LOGS) + 1
        assert len(host.argtypes) == len(roll.argtypes) - 1
        assert ("plant_pvec" if lm else "mu") in _lib.RMPC_STACK_ROLLOUT_ARGS[lm]
    # the PMPC stack tables are as they were
    assert _lib.STACK_LOGS == (("tilt", 2, np.float64), ("tray", 7, np.float64))
    assert len(_lib.STACK_STEP_ARGS[False]) == 16 and len(_lib.STACK_ROLLOUT_ARGS[True]) == 18
    for name in ("rmpc_stack_loop_step", "rmpc_stack_loop_step_dev", "rmpc_stack_rollout", "rmpc_stack_rollout_dev"):
        assert callable(getattr(_lib.RmpcSolver, name)), name


def test_null_handle_is_einval():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in ENTRIES:
        fn = getattr(L, n)
        assert fn(*[None if t is ctypes.c_void_p else 1 for t in fn.argtypes]) == EINVAL, n


# ---- behind a handle ----------------------------------------------------------------------------------------------------
E, N_ARM, ROWS, N_HORIZON = 3, 7, 4, 20


def _valid(lm):
    """A complete, correctly sized argument set in host memory (the host entries' form)."""
    from dart_mpc import _lib
    from dart_mpc.harness import rmpc_stack_arrays, rmpc_stack_logs
    rng = np.random.default_rng(0)
    ML = _lib.lib().dart_arm_model_len(N_ARM)
    prm = {"Wimp": np.eye(6), "Wpos": np.eye(N_ARM), "Wsmooth": np.zeros((N_ARM, N_ARM)), "Qmin": -np.ones(N_ARM),
           "Qmax": np.ones(N_ARM), "Qdotmin": -np.ones(N_ARM), "Qdotmax": np.ones(N_ARM), "taumin": -np.ones(N_ARM),
           "taumax": np.ones(N_ARM), "K": np.eye(6), "K_null": np.eye(N_ARM), "dt": 0.002}
    arrays, _, _, _ = rmpc_stack_arrays(np.zeros((E, 4)), np.zeros((E, 4)), np.zeros((E, 2, N_ARM)), np.zeros((E, 2, N_ARM)),
                                        rng.uniform(0.1, 1, (2, ML)), prm, [0.0, 0.0, 0.4],
                                        plant_pvec=np.ones((E, 34)) if lm else None, N=N_HORIZON)
    return arrays, rmpc_stack_logs(ROWS, E, N_ARM, lm)


def _rollout(solver, lm, arrays, logs, k0=0, steps=2, rows=ROWS, n=N_ARM, e=E, stride=None, **cfgs):
    try:
        solver.rmpc_stack_rollout(e, n, k0, steps, rows, arrays["arm_prm"].shape[1] if stride is None else stride, arrays,
                                  *logs, lm=lm, **cfgs)
    except Exception as err:        # DartMPCError carries the return code and the handle's message
        return str(err)
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("lm", [False, True])
def test_every_einval_behind_a_handle(lm):
    import dart_mpc
    from dart_mpc import _lib
    from dart_mpc.arm import arm_config, arm_dyn_config
    arrays, logs = _valid(lm)
    before = {k: v.copy() for k, v in arrays.items()}
    refused = []

    def refuse(what, err):
        assert err is not None and "(-1)" in err, (what, err)
        refused.append(what)

    class AsRmpc(_lib.RmpcSolver):
        """RmpcSolver's methods on another solver's handle (not owned), so that a PMPC handle reaches the entries."""

        def __init__(self, solver):
            self._h = solver._h

        def close(self):
            pass

    with dart_mpc.Solver(N=N_HORIZON, Ts=0.002, B_max=4) as pm_, dart_mpc.RmpcSolver(N=N_HORIZON, Ts=0.002, B_max=4) as rm:
        pm = AsRmpc(pm_)
        refuse("variant", _rollout(pm, lm, arrays, logs))
        for name in _lib.RMPC_STACK_ROLLOUT_ARGS[lm]:
            if name == "work":
                continue            # (the host form has none)
            refuse("null " + name, _rollout(rm, lm, {**arrays, name: None}, logs, stride=arrays["arm_prm"].shape[1]))
        for g in range(3):          # a log group given in part
            part = [dict(x) for x in logs]
            part[g][next(iter(part[g]))] = None
            refuse(f"mixed log group {g}", _rollout(rm, lm, arrays, part))
        refuse("k0 + steps > log_rows", _rollout(rm, lm, arrays, logs, k0=3, steps=2))
        refuse("k0 + steps > log_rows (one group given)", _rollout(rm, lm, arrays, (None, logs[1], None), k0=3, steps=2))
        refuse("negative k0", _rollout(rm, lm, arrays, logs, k0=-1))
        refuse("E > B_max", _rollout(rm, lm, arrays, logs, e=5))
        refuse("E < 1", _rollout(rm, lm, arrays, logs, e=0))
        refuse("n > DART_ARM_NMAX", _rollout(rm, lm, arrays, logs, n=9))
        refuse("n < 1", _rollout(rm, lm, arrays, logs, n=0))
        bad = _lib.stack_config(); bad.couple = 2
        refuse("couple", _rollout(rm, lm, arrays, logs, scfg=bad))
        refuse("loop rls_lambda", _rollout(rm, lm, arrays, logs, loop=_lib.rmpc_loop_config(rls_lambda=0.0)))
        refuse("loop dr_max", _rollout(rm, lm, arrays, logs, loop=_lib.rmpc_loop_config(dr_max=-1.0)))
        refuse("loop step_fraction", _rollout(rm, lm, arrays, logs, loop=_lib.rmpc_loop_config(step_fraction=1.5)))
        refuse("arm_prm_stride", _rollout(rm, lm, arrays, logs, stride=17))
        refuse("jacdot_point", _rollout(rm, lm, arrays, logs, dcfg=arm_dyn_config(jacdot_point=5)))
        refuse("QP tol", _rollout(rm, lm, arrays, logs, qcfg=arm_config(tol=0.0)))
        neg = arrays["nlog"].copy(); neg[1] = -1
        refuse("negative nlog", _rollout(rm, lm, {**arrays, "nlog": neg}, logs))
        refuse("negative nlog (metrics only)", _rollout(rm, lm, {**arrays, "nlog": neg}, (None, None, None), rows=0))
        if not lm:
            refuse("plant v_c", _rollout(rm, lm, arrays, logs, plant=_lib.plant_config(v_c=0.0)))
        # the loop-step entries: phase, null pointers of each phase, a log group in part, k >= log_rows
        # (device memory of the right sizes throughout)
        import torch
        SL = _lib.lib().dart_arm_snapshot_len(N_ARM)
        dev = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
        z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")     # noqa: E731
        dev.update(snap=z(2 * E, SL), ee_quat=z(2 * E, 4), x0=z(E, 4), Rref=z(E, 4 * (N_HORIZON + 1)), phi=z(E, 7), y=z(E, 2),
                   tray_cmd=z(E, 7), u0=z(E, 2), f=z(E), status=z(E, dt=torch.int32), iters=z(E, dt=torch.int32))
        dlog = {k: torch.from_numpy(v).cuda() for k, v in logs[0].items()}
        dsl = {k: torch.from_numpy(v).cuda() for k, v in logs[1].items()}
        torch.cuda.synchronize()
        ptr = {k: v.data_ptr() for k, v in dev.items()}

        def step(solver, phase, arr, lg=None, sl=None, k=0, post=1, rows=ROWS, **kw):
            try:
                solver.rmpc_stack_loop_step(E, N_ARM, k, phase, post, 1, rows, arr, lg, sl, lm=lm, **kw)
            except Exception as err:
                return str(err)
            return None

        refuse("step: variant", step(pm, _lib.STACK_COUPLE, ptr))
        refuse("phase", step(rm, 2, ptr))
        for name in ("u0", "tray_pos", "tray_cmd"):
            refuse("command: null " + name, step(rm, _lib.STACK_COMMAND, {**ptr, name: None}))
        for name in _lib.RMPC_STACK_STEP_ARGS[lm]:
            if name != "tray_cmd":
                refuse("couple: null " + name, step(rm, _lib.STACK_COUPLE, {**ptr, name: None}))
        lgp = {k: v.data_ptr() for k, v in dlog.items()}
        slp = {k: v.data_ptr() for k, v in dsl.items()}
        refuse("step: mixed RMPC logs", step(rm, _lib.STACK_COUPLE, ptr, {**lgp, "x": None}))
        refuse("step: mixed stack logs", step(rm, _lib.STACK_COUPLE, ptr, None, {**slp, "U_cmd": None}))
        refuse("step: k >= log_rows", step(rm, _lib.STACK_COUPLE, ptr, lgp, slp, k=ROWS))
        refuse("step: couple", step(rm, _lib.STACK_COUPLE, ptr, scfg=bad))
        refuse("step: loop config", step(rm, _lib.STACK_COUPLE, ptr, loop=_lib.rmpc_loop_config(rls_lambda=-1.0)))
        rm.sync()
        for k, v in arrays.items():
            assert np.array_equal(dev[k].cpu().numpy(), before[k], equal_nan=True), k
        for g in (dlog, dsl):
            for k, v in g.items():
                h = v.cpu().numpy()
                assert (np.isnan(h).all() if h.dtype == np.float64 else np.all(h == _lib.LOG_INT_FILL)), k
    print(len(refused), "refusals")
    for k, v in arrays.items():
        assert np.array_equal(v, before[k], equal_nan=True), k
    for g in logs:
        for k, v in g.items():
            assert (np.isnan(v).all() if v.dtype == np.float64 else np.all(v == _lib.LOG_INT_FILL)), k
