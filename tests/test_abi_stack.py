"""The stack entries of include/dart_mpc.h (added within ABI 8): symbols, defaults, and every argument check, all of
which return DART_MPC_EINVAL before any HIP call.  The checks that need no handle run without a GPU; a handle exists only
on a device, so the checks behind one are marked gpu -- they launch nothing: every call is refused, and the arrays it was
given are unchanged afterwards."""
import ctypes

import numpy as np
import pytest

ENTRIES = ("dart_pmpc_stack_loop_step_dev", "dart_pmpc_stack_lm_loop_step_dev", "dart_pmpc_stack_rollout_dev",
           "dart_pmpc_stack_lm_rollout_dev", "dart_pmpc_stack_rollout", "dart_pmpc_stack_lm_rollout")
EINVAL = -1


def test_symbols_defaults_and_tables():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in ENTRIES + ("dart_stack_config_default", "dart_stack_work_len", "dart_tray_from_arms_dev", "dart_tray_from_arms"):
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    assert L.dart_mpc_abi_version() == 8
    c = _lib.stack_config()
    assert c.couple == _lib.STACK_ACHIEVED == 1 and list(c.reserved) == [0] * 7
    assert _lib.stack_config("ride").couple == _lib.STACK_RIDE == 0
    assert L.dart_stack_work_len(3, 7) == L.dart_dual_arm_work_len(3, 7) + 15 * 3
    assert L.dart_stack_work_len(0, 7) == EINVAL and L.dart_stack_work_len(3, 9) == EINVAL
    assert len(_lib.STACK_METRIC_SLOTS) == 8
    # the binding's argument tables cover the entries' pointer arguments
    for lm in (False, True):
        step = getattr(L, "dart_pmpc_stack_lm_loop_step_dev" if lm else "dart_pmpc_stack_loop_step_dev")
        roll = getattr(L, "dart_pmpc_stack_lm_rollout_dev" if lm else "dart_pmpc_stack_rollout_dev")
        host = getattr(L, "dart_pmpc_stack_lm_rollout" if lm else "dart_pmpc_stack_rollout")
        nlog = len(_lib.PMPC_LM_LOOP_LOGS if lm else _lib.PMPC_LOOP_LOGS) + len(_lib.STACK_LOGS)
        assert len(step.argtypes) == 3 + 7 + len(_lib.STACK_STEP_ARGS[lm]) + nlog + 1
        assert len(roll.argtypes) == 5 + 6 + len(_lib.STACK_ROLLOUT_ARGS[lm]) + nlog + len(_lib.ARM_LOOP_LOGS) + 1
        assert len(host.argtypes) == len(roll.argtypes) - 1


def test_null_handle_is_einval():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in ENTRIES:
        fn = getattr(L, n)
        assert fn(*[None if t is ctypes.c_void_p else 1 for t in fn.argtypes]) == EINVAL, n


def test_tray_from_arms_checks_need_no_device():
    from dart_mpc import _lib
    from dart_mpc.arm import tray_from_arms
    L = _lib.lib()
    a = np.zeros(64)
    p = ctypes.c_void_p(a.ctypes.data)
    ok = [p] * 6
    for E in (0, -1, (1 << 20) + 1):
        assert L.dart_tray_from_arms(E, *ok) == EINVAL
        assert L.dart_tray_from_arms_dev(E, *ok, None) == EINVAL
    for i in range(6):
        args = list(ok); args[i] = None
        assert L.dart_tray_from_arms(1, *args) == EINVAL, i
        assert L.dart_tray_from_arms_dev(1, *args, None) == EINVAL, i
    with pytest.raises(_lib.DartMPCError):
        tray_from_arms(np.zeros((2, 2, 3)), np.zeros((3, 2, 4)))
    with pytest.raises(_lib.DartMPCError):
        tray_from_arms(np.zeros((2, 2, 3)), np.zeros((2, 2, 4)), grasp=np.zeros((2, 6)))


# ---- behind a handle ----------------------------------------------------------------------------------------------------
E, N_ARM, ROWS = 3, 7, 4


def _valid(lm):
    """A complete, correctly sized argument set in host memory (the host entries' form)."""
    from dart_mpc import _lib
    from dart_mpc.harness import stack_arrays, stack_logs
    rng = np.random.default_rng(0)
    ML = _lib.lib().dart_arm_model_len(N_ARM)
    prm = {"Wimp": np.eye(6), "Wpos": np.eye(N_ARM), "Wsmooth": np.zeros((N_ARM, N_ARM)), "Qmin": -np.ones(N_ARM),
           "Qmax": np.ones(N_ARM), "Qdotmin": -np.ones(N_ARM), "Qdotmax": np.ones(N_ARM), "taumin": -np.ones(N_ARM),
           "taumax": np.ones(N_ARM), "K": np.eye(6), "K_null": np.eye(N_ARM), "dt": 0.002}
    arrays, _, _, _ = stack_arrays(np.zeros((E, 6)), np.zeros((E, 6)), np.tile([0.1, 600, 5, 0.1, -0.6, 0.6], (E, 1)),
                                   np.zeros((E, 2, N_ARM)), np.zeros((E, 2, N_ARM)), rng.uniform(0.1, 1, (2, ML)), prm,
                                   [0.0, 0.0, 0.4], plant_pvec=np.ones((E, 34)) if lm else None)
    return arrays, stack_logs(ROWS, E, N_ARM, lm)


def _rollout(solver, lm, arrays, logs, k0=0, steps=2, rows=ROWS, n=N_ARM, e=E, stride=None, **cfgs):
    try:
        solver.stack_rollout(e, n, k0, steps, rows, arrays["arm_prm"].shape[1] if stride is None else stride, arrays,
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

    with dart_mpc.Solver(N=20, Ts=0.002, B_max=4) as pm, dart_mpc.RmpcSolver(N=20, Ts=0.002, B_max=4) as rm:
        refuse("variant", _rollout(rm, lm, arrays, logs))
        for name in _lib.STACK_ROLLOUT_ARGS[lm]:
            if name == "work":
                continue            # (the host form has none)
            refuse("null " + name, _rollout(pm, lm, {**arrays, name: None}, logs, stride=arrays["arm_prm"].shape[1]))
        for g in range(3):          # a log group given in part
            part = [dict(x) for x in logs]
            part[g][next(iter(part[g]))] = None
            refuse(f"mixed log group {g}", _rollout(pm, lm, arrays, part))
        refuse("k0 + steps > log_rows", _rollout(pm, lm, arrays, logs, k0=3, steps=2))
        refuse("k0 + steps > log_rows (one group given)", _rollout(pm, lm, arrays, (None, logs[1], None), k0=3, steps=2))
        refuse("negative k0", _rollout(pm, lm, arrays, logs, k0=-1))
        refuse("E > B_max", _rollout(pm, lm, arrays, logs, e=5))
        refuse("E < 1", _rollout(pm, lm, arrays, logs, e=0))
        bad = _lib.stack_config(); bad.couple = 2
        refuse("couple", _rollout(pm, lm, arrays, logs, scfg=bad))
        refuse("n > DART_ARM_NMAX", _rollout(pm, lm, arrays, logs, n=9))
        refuse("arm_prm_stride", _rollout(pm, lm, arrays, logs, stride=17))
        refuse("jacdot_point", _rollout(pm, lm, arrays, logs, dcfg=arm_dyn_config(jacdot_point=5)))
        refuse("QP tol", _rollout(pm, lm, arrays, logs, qcfg=arm_config(tol=0.0)))
        refuse("QP max_iter", _rollout(pm, lm, arrays, logs, qcfg=arm_config(max_iter=0)))
        if not lm:
            refuse("plant v_c", _rollout(pm, lm, arrays, logs, plant=_lib.plant_config(v_c=0.0)))
        # the loop-step entries: phase, null pointers of each phase, a log group in part, k >= log_rows
        # (device memory of the right sizes throughout)
        import torch
        SL = _lib.lib().dart_arm_snapshot_len(N_ARM)
        dev = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
        dev.update(snap=torch.zeros((2 * E, SL), dtype=torch.float64, device="cuda"),
                   ee_quat=torch.zeros((2 * E, 4), dtype=torch.float64, device="cuda"),
                   x0=torch.zeros((E, 6), dtype=torch.float64, device="cuda"),
                   tray_cmd=torch.zeros((E, 7), dtype=torch.float64, device="cuda"),
                   u0=torch.zeros((E, 2), dtype=torch.float64, device="cuda"),
                   f=torch.zeros(E, dtype=torch.float64, device="cuda"),
                   status=torch.zeros(E, dtype=torch.int32, device="cuda"),
                   iters=torch.zeros(E, dtype=torch.int32, device="cuda"))
        dlog = {k: torch.from_numpy(v).cuda() for k, v in logs[0].items()}
        torch.cuda.synchronize()
        ptr = {k: v.data_ptr() for k, v in dev.items()}

        def step(phase, arr, lg=None, sl=None, k=0, post=1, rows=ROWS, **kw):
            try:
                pm.stack_loop_step_dev(E, N_ARM, k, phase, post, 1, rows, arr, lg, sl, lm=lm, **kw)
            except Exception as err:
                return str(err)
            return None

        refuse("phase", step(2, ptr))
        for name in ("u0", "tray_pos", "tray_cmd"):
            refuse("command: null " + name, step(_lib.STACK_COMMAND, {**ptr, name: None}))
        for name in _lib.STACK_STEP_ARGS[lm]:
            if name != "tray_cmd":
                refuse("couple: null " + name, step(_lib.STACK_COUPLE, {**ptr, name: None}))
        lgp = {k: v.data_ptr() for k, v in dlog.items()}
        refuse("step: mixed logs", step(_lib.STACK_COUPLE, ptr, {**lgp, "X": None}))
        refuse("step: k >= log_rows", step(_lib.STACK_COUPLE, ptr, lgp, k=ROWS))
        refuse("step: couple", step(_lib.STACK_COUPLE, ptr, scfg=bad))
        pm.sync()
        for k, v in arrays.items():
            assert np.array_equal(dev[k].cpu().numpy(), before[k], equal_nan=True), k
    print(len(refused), "refusals")
    for k, v in arrays.items():
        assert np.array_equal(v, before[k], equal_nan=True), k
    for g in logs:
        for k, v in g.items():
            assert (np.isnan(v).all() if v.dtype == np.float64 else np.all(v == _lib.LOG_INT_FILL)), k
