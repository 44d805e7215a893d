"""The closed-loop rollout entries of include/dart_mpc.h (added within ABI 8): symbols, argument checks that
need no GPU, and the defaults of the loop against those of dart_mpc.harness (no compute)."""
import inspect

import numpy as np

NEW = ("dart_rmpc_loop_step_dev", "dart_pmpc_loop_step_dev", "dart_rmpc_rollout_dev", "dart_pmpc_rollout_dev",
       "dart_rmpc_rollout", "dart_pmpc_rollout")


def test_new_symbols_exist_within_abi_8():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in NEW + ("dart_plant_config_default", "dart_rmpc_loop_config_default"):
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS
    assert L.dart_mpc_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_null_handle_is_einval():
    from dart_mpc import _lib
    L = _lib.lib()
    for n in NEW:
        fn = getattr(L, n)
        args = [None if t is _lib.ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -1, n


def test_config_defaults_equal_the_host_loop():
    from dart_mpc import _lib, harness
    p = _lib.plant_config()
    sig = inspect.signature(harness.TrayPlant.__init__).parameters
    assert (p.tau, p.mu_c, p.v_c) == (sig["tau"].default, sig["mu_c"].default, sig["v_c"].default) == (0.03, 0.02, 0.01)
    c = _lib.rmpc_loop_config()
    sig = inspect.signature(harness.run_rmpc).parameters
    assert (c.dr_max, c.alpha_rg, c.rls_lambda, c.pos_tol) == (sig["dr_max"].default, sig["alpha_rg"].default,
                                                               sig["lam"].default, sig["pos_tol"].default)
    assert (c.dr_max, c.alpha_rg, c.step_fraction, c.rls_lambda, c.pos_tol) == (0.01, 0.5, 0.2, 0.995, 0.01)
    # the rollouts take run_rmpc's / run_pmpc's arguments
    for host, dev in ((harness.run_rmpc, harness.rollout_rmpc), (harness.run_pmpc, harness.rollout_pmpc)):
        a, b = inspect.signature(host).parameters, inspect.signature(dev).parameters
        assert list(a) == list(b)[:len(a)]
        assert all(a[k].default == b[k].default for k in a)


def test_log_prefill_and_layout_tables():
    from dart_mpc import _lib
    lg = _lib.loop_logs(_lib.RMPC_LOOP_LOGS, 3, 5)
    assert lg["theta"].shape == (3, 5, 14) and lg["f"].shape == (3, 5) and np.isnan(lg["x"]).all()
    assert lg["status"].dtype == np.int32 and np.all(lg["status"] == _lib.LOG_INT_FILL)
    assert [n for n, _, _ in _lib.RMPC_LOOP_STATE] == ["x", "tilt", "prev", "u_prev", "r_v", "theta", "P", "w", "done",
                                                      "nlog"]
