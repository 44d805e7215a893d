"""What the tests of the device-resident closed loops share (test_gpu_rollout.py, test_gpu_cross_plant.py,
test_gpu_lmpc_rollout.py, test_gpu_lmpc_collect.py): the L / torch fixtures, device staging, the comparisons, and
the RMPC loop step's inputs and numpy expectation on either plant.  A plain module, imported by name.
"""
import numpy as np
import pytest

TS = 0.002
RMPC_PRM = np.array([80.0, 2.0, 0.02, 1.0, -0.6, 0.6, -0.06, 0.06, 0.2, 0.1])       # rob_ctrl.py:280-283
X_LO = np.array([-0.18, -0.15, -0.13, -0.15, -0.05, -0.05, -0.05, -0.05])       # workload.lmpc_batch's state ranges


@pytest.fixture(scope="module")
def L():
    from dart_mpc import _lib
    return _lib


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _to_dev(torch, arrays):
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
    torch.cuda.synchronize()
    return d


def _ptrs(d):
    return None if d is None else {k: v.data_ptr() for k, v in d.items()}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(torch, a, b):
    """Bit-for-bit equality (NaN prefill included)."""
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _shape(B, width, **sizes):
    width = sizes[width] if isinstance(width, str) else width
    return (B, width) if width else (B,)


def _nan_io(L, spec, B, **sizes):
    return {n: (np.full(_shape(B, w, **sizes), np.nan) if dt is np.float64 else np.full(B, L.LOG_INT_FILL, np.int32))
            for n, w, dt in spec}


def _close(got, want, what):
    """|got - want| <= 1e-13 with the NaN prefill in the same places (floats); equality (ints).  Returns the largest
    difference."""
    worst = 0.0
    for k in want:
        if want[k].dtype == np.float64:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{what}: {k} (prefill)"
            if np.isfinite(want[k]).any():
                worst = max(worst, float(np.nanmax(np.abs(got[k] - want[k]))))
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-13, equal_nan=True, err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    return worst


def _metrics_midrun(L, B):
    """Metrics of a fresh run (even instances) and of runs under way (odd: not yet converged; every fourth: converged
    at step 0)."""
    m = L.loop_metrics(B)
    odd = np.arange(B) % 2 == 1
    m[odd] = [0.03, -1.0, 0.2, 0.09, 2.0, 55.0, 0.02, 7.0]
    m[np.arange(B) % 4 == 3, 1] = 0.0
    return m


def _tray_step(harness, x, tilt, u, mu):
    """harness.TrayPlant.step: (next x, next tilt)."""
    plant = harness.TrayPlant(x, mu, dt=TS)
    plant.tilt = tilt.copy()
    xn = plant.step(u)
    return xn, plant.tilt


def _lm_step(harness, x8, tilt, u, pvec):
    """harness.LmpcPlant.step with the flipped command: (next x, next tilt in the PMPC / RMPC convention)."""
    plant = harness.LmpcPlant(x8, pvec, dt=TS)          # tau 0.03, as dart_plant_config's default
    plant.tilt = -tilt
    xn = plant.step(-u)
    return xn, -plant.tilt


def _rmpc_case(L, rng, B, N, lm=False):
    """Inputs of one RMPC loop step: (state, target, prm, the plant's parameters, solve I/O).  Tray plant: x [B, 6],
    mu [B]; LMPC plant (``lm``): x [B, 8], metrics under way, pvec [B, 34]."""
    if lm:
        x = rng.uniform(X_LO, -X_LO, (B, 8))
    else:
        x = np.zeros((B, 6)); x[:, :4] = rng.uniform(-0.3, 0.3, (B, 4)); x[:, 4] = 0.43
    state = dict(x=x, tilt=rng.uniform(-0.3, 0.3, (B, 2)), prev=x[:, :4] + rng.uniform(-1e-3, 1e-3, (B, 4)),
                 u_prev=rng.uniform(-0.5, 0.5, (B, 2)), r_v=rng.uniform(-0.1, 0.1, (B, 4)),
                 theta=rng.uniform(-1, 1, (B, 14)), done=(rng.uniform(size=B) < 0.3).astype(np.int32),
                 nlog=rng.integers(0, 3, B).astype(np.int32))
    if lm:
        state["metrics"] = _metrics_midrun(L, B)
    target = np.zeros((B, 4)); target[:, [0, 2]] = rng.uniform(-0.1, 0.1, (B, 2))
    near = np.arange(B) % 4 == 1            # within the tolerance: the episode closes at this step
    target[near, 0] = x[near, 0] + 1e-3; target[near, 2] = x[near, 2] - 2e-3
    io = _nan_io(L, L.RMPC_LOOP_IO, B, nref=4 * (N + 1))
    io.update(u0=rng.uniform(-0.5, 0.5, (B, 2)), f=rng.uniform(0, 1, B), status=rng.integers(-2, 3, B).astype(np.int32),
              iters=rng.integers(1, 60, B).astype(np.int32))
    plant = rng.uniform(0.01, 1.9, (B, 34)) if lm else rng.uniform(0.05, 0.3, B)
    return state, target, np.tile(RMPC_PRM, (B, 1)), plant, io


def _rmpc_expected(L, harness, state, target, prm, plant_step, io, logs, N, k, do_post, do_pre):
    """The numpy code the RMPC loop step restates.  ``plant_step(x, tilt, u)`` returns (next x, next tilt); a state
    with "metrics" is the LMPC plant's (the metrics and the rotation log); ``logs`` None is the metrics-only mode."""
    from dart_mpc.rmpc import AdaptiveNPMPCSmooth, rls_features
    s = {n: v.copy() for n, v in state.items()}
    io = {n: v.copy() for n, v in io.items()}
    lg = None if logs is None else {n: v.copy() for n, v in logs.items()}
    B = s["x"].shape[0]
    c = L.rmpc_loop_config()
    if do_post:
        xk, u = s["x"][:, :4].copy(), io["u0"]
        en = np.linalg.norm(xk[:, [0, 2]] - target[:, [0, 2]], axis=1)
        for b in np.where(s["done"] == 0)[0]:
            r = s["nlog"][b]
            if lg is not None:
                lg["pos_err"][r, b] = [target[b, 0] - xk[b, 0], target[b, 2] - xk[b, 2]]
                lg["pos_err_norm"][r, b] = float(en[b])
                lg["u_cmd"][r, b] = u[b]
                lg["timestep"][r, b] = k * TS
            s["nlog"][b] += 1
            if en[b] < c.pos_tol:
                s["done"][b] = 1
        if lg is not None:
            lg["x"][k], lg["theta"][k], lg["r_v"][k] = xk, s["theta"], s["r_v"]
            lg["f"][k], lg["status"][k], lg["iters"][k] = io["f"], io["status"], io["iters"]
            if "metrics" in s:
                lg["rot"][k] = s["x"][:, 4:]
        if "metrics" in s:
            s["metrics"] = harness.rollout_metrics(xk[None], target, u[None], io["status"][None], io["iters"][None],
                                                   s["x"][None, :, 4:], TS, metrics=s["metrics"], k0=k)
        s["prev"], s["u_prev"] = xk, u.copy()
        s["x"], s["tilt"] = plant_step(s["x"], s["tilt"], u)
    if do_pre:
        xk, prev = s["x"][:, :4].copy(), s["prev"]
        io["y"] = (xk[:, [1, 3]] - prev[:, [1, 3]]) / TS
        io["phi"] = np.stack([rls_features(p, prm[0, 9]) for p in prev])
        err = np.stack([target[:, 0] - s["r_v"][:, 0], np.zeros(B), target[:, 2] - s["r_v"][:, 2], np.zeros(B)], axis=1)
        s["r_v"] = s["r_v"] + c.alpha_rg * np.clip(err, -c.dr_max, c.dr_max) * np.array([1.0, 0.0, 1.0, 0.0])
        io["Rref"] = np.stack([AdaptiveNPMPCSmooth.build_ref_traj(xk[b], s["r_v"][b], target[b], N, 4, step_fraction=0.2)
                               for b in range(B)])
        io["x0"] = xk
    return s, io, lg
