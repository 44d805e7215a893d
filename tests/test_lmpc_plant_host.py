"""harness.LmpcPlant (numpy; the plant of harness.run_lmpc and the model lmpc_loop_kernel restates) against the C
oracle's RK4 step of the same model (oracle_lib.lmpc_rk4, oracle/lmpc_ipm.c).

Bar: 1e-15 absolute on 256 draws with |x_next| <= 0.25.  The numpy restatement oracle/lmpc_nlp.rk4 and the C oracle
differ by at most 5.6e-17 on 4096 such draws: both evaluate the same expressions in fp64 and only libm's sin / tanh /
exp against numpy's can differ, by an ulp of values below 1 scaled by Ts.
"""
import numpy as np

import oracle_lib

TS = 0.002


def _draws(n, seed=11):
    rng = np.random.default_rng(seed)
    lo = np.array([-0.18, -0.15, -0.13, -0.15, -0.05, -0.05, -0.05, -0.05])        # workload.lmpc_batch's state ranges
    x = rng.uniform(lo, -lo, (n, 8))
    return x, rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(0.01, 1.9, (n, 34))


def test_lmpc_plant_step_matches_c_oracle():
    from dart_mpc import harness
    x, u, pv = _draws(256)
    plant = harness.LmpcPlant(x, pv, tau=0.0, dt=TS)
    got = plant.step(u)
    want = oracle_lib.lmpc_rk4(x, u, pv, TS)
    d = float(np.max(np.abs(got - want)))
    print(f"LmpcPlant.step vs oracle_lib.lmpc_rk4: max |dx| = {d:.3e}, max |x_next| = {np.abs(want).max():.3f}")
    assert np.array_equal(plant.tilt, u)                  # tau = 0: the tilt follows the command at once
    assert got.shape == (256, 8) and d <= 1e-15
    # a second step continues from the first
    want2 = oracle_lib.lmpc_rk4(got, u, pv, TS)
    assert float(np.max(np.abs(plant.step(u) - want2))) <= 1e-15


def test_lmpc_plant_tilt_lag_is_tray_plants():
    from dart_mpc import harness
    x, u, pv = _draws(16, seed=12)
    plant = harness.LmpcPlant(x, pv, tau=0.03, dt=TS)
    tray = harness.TrayPlant(np.zeros((16, 6)), 0.1, tau=0.03, dt=TS)
    assert plant.a_lag == tray.a_lag == 1.0 - np.exp(-TS / 0.03)
    tilt = np.zeros((16, 2))
    for _ in range(3):
        plant.step(u)
        tray.step(u)
        tilt = tilt + plant.a_lag * (u - tilt)
        np.testing.assert_array_equal(plant.tilt, tray.tilt)
        np.testing.assert_array_equal(plant.tilt, tilt)
    # the model sees the lagged tilt, not the command
    ref = harness.LmpcPlant(x, pv, tau=0.0, dt=TS)
    lag = harness.LmpcPlant(x, pv, tau=0.03, dt=TS)
    first = lag.a_lag * u
    np.testing.assert_array_equal(lag.step(u), ref.step(first))
