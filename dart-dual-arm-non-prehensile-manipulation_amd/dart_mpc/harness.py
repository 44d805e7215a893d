"""Headless closed-loop harness and the reference's result formats.

The reference evaluates its controllers end to end in MuJoCo (PMPC/main_parallel_enhanced.py:290-419,
RMPC/dev_dual/rob_ctrl.py:331-420) and writes
  * PMPC / LMPC: one ``.npz`` per experiment with the per-step logs of AsyncLogger
    (PMPC/src/logger.py:90-111) plus three metrics (:158-183): steady-state error, convergence
    time (first step with error < 1 cm) and control effort (sum |U_cmd| dt);
  * RMPC: a JSON file ``{"data": {"ep1": {"pos_err", "pos_err_norm", "u_cmd", "torque",
    "timestep"}}}`` (rob_ctrl.py:51-86), one episode per run until the 1 cm tolerance is reached.

MuJoCo is not part of this package.  ``TrayPlant`` is a batched stand-in for the scene: the tray tilt
follows the commanded tilt through a first-order lag (the arms' impedance tracking), and the object
obeys the reference model (mpc_3d.py:87-97) driven by the *actual* tilt plus a Coulomb friction term
the MPC model does not have -- so the loop sees model mismatch, as the reference's does.  Many
experiments (object configs, targets) run in lock step: one batched GPU solve per simulation step.
Times in the logs are simulation time (the reference logs wall time); ``solve_time`` is the wall
time of the step's batched solve, shared by every experiment of that step.
"""
from __future__ import annotations

import json
import os
import time
from datetime import datetime
from pathlib import Path

import numpy as np

from ._lib import RmpcSolver, Solver
from .pmpc import tilt_to_quat
from .rmpc import AdaptiveNPMPCSmooth, rls_features

G_Z = -9.81
ERROR_THRESHOLD = 0.01          # logger.py:162 and rob_ctrl.py:323 (1 cm)
NPZ_KEYS = ("t", "X", "X_target", "U_cmd", "quat_tray", "loss", "solve_time", "L_torques", "R_torques", "L_qpos",
            "R_qpos", "L_qvel", "R_qvel", "L_ee_pos", "R_ee_pos", "L_ee_vel", "R_ee_vel")


class TrayPlant:
    """B objects on B tilting trays, integrated with RK4 at ``dt`` (tilt held within a step).

    state x = [px, vx, py, vy, pz, vz] (mpc_3d.py:106-113); tilt = [theta_x, theta_y] follows the
    command: tilt += (1 - exp(-dt / tau)) (u_cmd - tilt)."""

    def __init__(self, x0, mu, tau=0.03, mu_c=0.02, v_c=0.01, dt=0.002, g=G_Z):
        self.x = np.array(x0, dtype=float).reshape(-1, 6).copy()
        B = self.x.shape[0]
        self.mu = np.broadcast_to(np.asarray(mu, float), (B,)).copy()
        self.tilt = np.zeros((B, 2))
        self.a_lag = 1.0 - np.exp(-dt / tau) if tau > 0 else 1.0
        self.mu_c, self.v_c, self.dt, self.g = float(mu_c), float(v_c), float(dt), float(g)

    def _f(self, x, s):
        vx, vy = x[:, 1], x[:, 3]
        fric = self.mu_c * abs(self.g)
        ax = self.g * s[:, 0] - self.mu * vx - fric * np.tanh(vx / self.v_c)
        ay = self.g * s[:, 1] - self.mu * vy - fric * np.tanh(vy / self.v_c)
        return np.stack([vx, ax, vy, ay, np.zeros_like(vx), np.zeros_like(vx)], axis=1)

    def step(self, u_cmd):
        self.tilt += self.a_lag * (np.asarray(u_cmd, float).reshape(-1, 2) - self.tilt)
        s = np.sin(self.tilt)
        h, x = self.dt, self.x
        k1 = self._f(x, s)
        k2 = self._f(x + h / 2 * k1, s)
        k3 = self._f(x + h / 2 * k2, s)
        k4 = self._f(x + h * k3, s)
        self.x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        return self.x


# ---------------------------------------------------------------------------------------------
# formats
def logger_metrics(logs: dict, dt: float) -> dict:
    """AsyncLogger's metrics (PMPC/src/logger.py:158-183)."""
    X, Xt, t = np.asarray(logs["X"]), np.asarray(logs["X_target"]), np.asarray(logs["t"])
    if len(t) == 0:
        return {}
    sse = float(np.linalg.norm(X[-1, [0, 2]] - Xt[-1, [0, 2]]))
    errors = np.linalg.norm(X[:, [0, 2]] - Xt[:, [0, 2]], axis=1)
    idx = np.where(errors < ERROR_THRESHOLD)[0]
    conv = float(t[idx[0]]) if len(idx) > 0 else float(t[-1])
    effort = float(np.sum(np.linalg.norm(np.asarray(logs["U_cmd"]), axis=1)) * dt)
    return {"steady_state_error": sse, "convergence_time": conv, "control_effort": effort}


def rollout_metrics(X, target, U, status, iters, rot, Ts, metrics=None, k0=0):
    """The eight streaming accumulators of the cross-plant loops (csrc/loop_step.hip loop_metrics_step, _lib.METRIC_SLOTS)
    restated in numpy as a plain sequential loop over the steps: X [K, B, >= 3] the states the solves saw, target
    [B, >= 3], U [K, B, 2], status / iters [K, B], rot [K, B, 4] = [th_x, om_x, th_y, om_y] (one experiment: the same
    without the B axis).  With e_k = |X_k[[0, 2]] - target[[0, 2]]|: 0 e of the last step, 1 first k with e_k <
    ERROR_THRESHOLD (-1 while none), 2 sum |u_k| Ts, 3 max e_k, 4 steps with status != 0, 5 sum of iters, 6 max of
    |th_x|, |th_y|, 7 steps.  Slots 0 .. 2 are ``logger_metrics`` (convergence_time = Ts * slot 1, or t[-1] when slot 1
    is -1).  ``metrics`` [B, 8] / ``k0`` continue an earlier run.  Returns [B, 8] ([8] for one experiment)."""
    X, U = np.asarray(X, float), np.asarray(U, float)
    one = X.ndim == 2
    if one:
        X, U, target = X[:, None], U[:, None], np.asarray(target, float)[None]
        status, iters, rot = np.asarray(status)[:, None], np.asarray(iters)[:, None], np.asarray(rot, float)[:, None]
    target, status, iters, rot = np.asarray(target, float), np.asarray(status), np.asarray(iters), np.asarray(rot, float)
    K, B = X.shape[:2]
    if metrics is None:
        M = np.zeros((B, 8)); M[:, 1] = -1.0
    else:
        M = np.array(metrics, float).reshape(B, 8)
    for k in range(K):
        for b in range(B):
            m = M[b]
            dx, dy = X[k, b, 0] - target[b, 0], X[k, b, 2] - target[b, 2]
            e = np.sqrt(dx * dx + dy * dy)
            un = np.sqrt(U[k, b, 0] * U[k, b, 0] + U[k, b, 1] * U[k, b, 1])
            th = max(abs(rot[k, b, 0]), abs(rot[k, b, 2]))
            m[0] = e
            if m[1] < 0.0 and e < ERROR_THRESHOLD:
                m[1] = float(k0 + k)
            m[2] = m[2] + un * Ts
            if e > m[3]:
                m[3] = e
            if status[k, b] != 0:
                m[4] = m[4] + 1.0
            m[5] = m[5] + float(iters[k, b])
            if th > m[6]:
                m[6] = th
            m[7] = m[7] + 1.0
    return M[0] if one else M


def population_scores(metrics):
    """The score kernel (csrc/loop_step.hip lmpc_eval_scores_kernel, _lib.SCORE_SLOTS) restated in numpy with plain
    loops: metrics [P, B, 8] (_lib.METRIC_SLOTS per instance) -> scores [P, 8], every sum sequential over b = 0 .. B-1
    in fp64, so the kernel gives the same bits.  0 mean steady-state error, 1 converged fraction (slot 1 >= 0),
    2 mean convergence step over the converged (-1 when none), 3 mean control effort, 4 max error, 5 steps with
    status != 0, 6 iterations per solve (0 when no step was taken), 7 max rotation."""
    M = np.asarray(metrics, float)
    P, B = M.shape[:2]
    S = np.zeros((P, 8))
    for l in range(P):
        sse = conv = conv_sum = effort = bad = its = n = 0.0
        emax = rot = 0.0
        for b in range(B):
            m = M[l, b]
            sse = sse + m[0]
            if m[1] >= 0.0:
                conv = conv + 1.0
                conv_sum = conv_sum + m[1]
            effort = effort + m[2]
            if b == 0 or m[3] > emax:
                emax = m[3]
            bad = bad + m[4]
            its = its + m[5]
            if b == 0 or m[6] > rot:
                rot = m[6]
            n = n + m[7]
        S[l] = [sse / float(B), conv / float(B), conv_sum / conv if conv > 0.0 else -1.0, effort / float(B), emax, bad,
                its / n if n != 0.0 else 0.0, rot]
    return S


def save_npz(logs: dict, metrics: dict, log_dir, experiment_name: str, object_name: str, mass, friction) -> str:
    """np.savez(logs + metrics) at ``{log_dir}/{object}/mass={m}_friction={f}/{name}_{timestamp}.npz``
    (logger.py:186-196)."""
    save_dir = os.path.join(str(log_dir), object_name, f"mass={mass}_friction={friction}")
    os.makedirs(save_dir, exist_ok=True)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    path = os.path.join(save_dir, f"{experiment_name}_{stamp}.npz")
    np.savez(path, **{**logs, **metrics})
    return path


def to_jsonable(obj):
    """rob_ctrl.py:51-62."""
    if isinstance(obj, dict):
        return {k: to_jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_jsonable(v) for v in obj]
    if isinstance(obj, np.ndarray):
        return to_jsonable(obj.tolist())
    if isinstance(obj, np.generic):
        return to_jsonable(obj.item())
    if isinstance(obj, float):
        return obj if np.isfinite(obj) else None
    return obj


def add_episode(store: dict, ep_name: str, pos_err, error_norm, u_cmd, torque, timestep) -> None:
    """rob_ctrl.py:64-76."""
    store[ep_name] = {"pos_err": pos_err, "pos_err_norm": error_norm, "u_cmd": u_cmd, "torque": torque,
                      "timestep": timestep}


def save_episodes_json(path, episodes: dict, pretty: bool = True) -> None:
    """rob_ctrl.py:78-83: ``{"data": episodes}``, NaN-free."""
    with Path(path).open("w", encoding="utf-8") as f:
        json.dump({"data": to_jsonable(episodes)}, f, indent=2 if pretty else None, ensure_ascii=False,
                  allow_nan=False)


# ---------------------------------------------------------------------------------------------
# closed loops
def _cross_plant(x4, x_rot0, plant_pvec, Ts, plant_kw):
    """``LmpcPlant`` of the cross-plant loops from the translation states [B, 4] and ``x_rot0`` [B, 4] (default zeros);
    of ``plant_kw`` only ``tau`` applies (the LMPC model's Stribeck terms are its Coulomb friction)."""
    x4 = np.asarray(x4, float).reshape(-1, 4)
    B = x4.shape[0]
    x8 = np.zeros((B, 8)); x8[:, :4] = x4
    if x_rot0 is not None:
        x8[:, 4:] = np.asarray(x_rot0, float).reshape(B, 4)
    kw = {k: v for k, v in (plant_kw or {}).items() if k == "tau"}
    return LmpcPlant(x8, np.asarray(plant_pvec, float).reshape(B, 34), dt=Ts, **kw)


def run_pmpc(states0, targets, prm, steps: int, N: int = 20, Ts: float = 0.002, tol: float = 1e-8, device: int = 0,
             plant_kw: dict | None = None, plant_pvec=None, x_rot0=None):
    """B PMPC experiments in lock step (main_parallel_enhanced.py:290-419 without MuJoCo): per step the
    state of every object, one batched cold-started solve, tilt -> quaternion (:333-348), plant step.

    states0, targets [B, 6]; prm [B, 6] = [mu, Qp, Qv, R, u_lo, u_hi] (the solver's parameter rows).
    Returns a list of per-experiment log dicts in the AsyncLogger schema, metrics included, and the
    per-step solver statuses [steps, B].

    ``plant_pvec`` [B, 34]: the plant is ``LmpcPlant`` with these true parameters, started from states0[:, :4] and
    ``x_rot0`` [B, 4] (default zeros) and stepped with ``-u0`` (the LMPC model's gravity has the other sign,
    rlmpc2.py:353-357 against mpc_3d.py:91-92); the solves see [x[:4], states0[:, 4:6]].  The dicts then also hold
    ``rot`` [steps, 4] and ``metrics`` [8] (``rollout_metrics``)."""
    states0 = np.asarray(states0, float).reshape(-1, 6)
    B = states0.shape[0]
    targets = np.asarray(targets, float).reshape(B, 6)
    prm = np.asarray(prm, float).reshape(B, 6)
    cross = plant_pvec is not None
    solver = Solver(N=N, Ts=Ts, tol=tol, B_max=max(B, 1), device=device)
    plant = _cross_plant(states0[:, :4], x_rot0, plant_pvec, Ts, plant_kw) if cross \
        else TrayPlant(states0, prm[:, 0], dt=Ts, **(plant_kw or {}))
    X = np.zeros((steps, B, 6)); U = np.zeros((steps, B, 2)); Q = np.zeros((steps, B, 4))
    L = np.zeros((steps, B)); ST = np.zeros((steps, B), np.int32); TS = np.zeros(steps)
    IT = np.zeros((steps, B), np.int32); ROT = np.zeros((steps, B, 4))
    try:
        for k in range(steps):
            if cross:
                X[k] = np.concatenate([plant.x[:, :4], states0[:, 4:6]], axis=1)
                ROT[k] = plant.x[:, 4:]
            else:
                X[k] = plant.x
            t0 = time.perf_counter()
            out = solver.solve_batch(X[k], targets, prm)
            TS[k] = time.perf_counter() - t0
            U[k], L[k], ST[k], IT[k] = out["u0"], out["f"], out["status"], out["iters"]
            Q[k] = np.stack([tilt_to_quat(u) for u in out["u0"]])
            plant.step(-out["u0"] if cross else out["u0"])
    finally:
        solver.close()
    t = np.arange(steps) * Ts
    M = rollout_metrics(X, targets, U, ST, IT, ROT, Ts) if cross else None
    logs = []
    for b in range(B):
        lg = {"t": t, "X": X[:, b], "X_target": np.tile(targets[b], (steps, 1)), "U_cmd": U[:, b],
              "quat_tray": Q[:, b], "loss": L[:, b], "solve_time": TS.copy()}
        for key, w in (("torques", 7), ("qpos", 7), ("qvel", 7), ("ee_pos", 3), ("ee_vel", 6)):
            lg["L_" + key] = np.zeros((steps, w))       # arms are not simulated here
            lg["R_" + key] = np.zeros((steps, w))
        lg.update(logger_metrics(lg, Ts))
        if cross:
            lg.update(rot=ROT[:, b], metrics=M[b])
        logs.append(lg)
    return logs, ST


def run_rmpc(x0, targets, steps: int, N: int = 20, Ts: float = 0.002, prm=None, device: int = 0,
             pos_tol: float = ERROR_THRESHOLD, plant_kw: dict | None = None, mu=0.1, dr_max: float = 0.01,
             alpha_rg: float = 0.5, lam: float = 0.995, P0: float = 1e3, plant_pvec=None, x_rot0=None):
    """B RMPC experiments in lock step (rob_ctrl.py:320-420 without MuJoCo): RLS on the measured
    accelerations fused into the solve launch, reference governor, staged reference, warm-started
    solve; an experiment's episode closes when its error first drops below ``pos_tol`` (the
    reference then stops).  Returns (episodes per experiment in the rob_ctrl.py JSON layout,
    statuses [steps, B]).

    ``plant_pvec`` [B, 34]: the plant is ``LmpcPlant`` with these true parameters (``mu`` is then not used), started
    from x0 and ``x_rot0`` [B, 4] (default zeros) and stepped with ``-u`` (see ``run_pmpc``).  Each experiment's dict
    then also holds ``rot`` [steps run, 4] and ``metrics`` [8] (``rollout_metrics`` over the steps run)."""
    x0 = np.asarray(x0, float).reshape(-1, 4)
    B = x0.shape[0]
    targets = np.asarray(targets, float).reshape(B, 4)
    ctl = AdaptiveNPMPCSmooth(None, None, Ts=Ts, N=N, Qp=80.0, Qv=2.0, Ru=0.02, Rdu=1.0, u_bounds=(-0.6, 0.6),
                              du_bounds=(-0.06, 0.06), vmax=0.2, v_eps=0.1)          # rob_ctrl.py:280-283
    prm = np.tile(ctl.params(), (B, 1)) if prm is None else np.asarray(prm, float).reshape(B, 10)
    solver = RmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device)
    full = np.zeros((B, 6)); full[:, :4] = x0
    cross = plant_pvec is not None
    plant = _cross_plant(x0, x_rot0, plant_pvec, Ts, plant_kw) if cross else TrayPlant(full, mu, dt=Ts, **(plant_kw or {}))
    XS = np.zeros((steps, B, 4)); US = np.zeros((steps, B, 2)); IT = np.zeros((steps, B), np.int32)
    ROT = np.zeros((steps, B, 4))
    theta = np.zeros((B, 14)); P = np.tile(np.eye(7) * P0, (B, 2, 1, 1))
    r_v = np.zeros((B, 4)); u_prev = np.zeros((B, 2)); w = np.zeros((B, ctl.w0.shape[0]))
    prev = x0.copy()
    done = np.zeros(B, bool)
    logs = [{"pos_err": [], "pos_err_norm": [], "u_cmd": [], "torque": [], "timestep": []} for _ in range(B)]
    ST = np.zeros((steps, B), np.int32)
    try:
        for k in range(steps):
            xk = plant.x[:, :4].copy()
            y = (xk[:, [1, 3]] - prev[:, [1, 3]]) / Ts
            phi = np.stack([rls_features(p, ctl.v_eps) for p in prev])
            err = np.stack([targets[:, 0] - r_v[:, 0], np.zeros(B), targets[:, 2] - r_v[:, 2], np.zeros(B)], axis=1)
            r_v = r_v + alpha_rg * np.clip(err, -dr_max, dr_max) * np.array([1.0, 0.0, 1.0, 0.0])
            Rref = np.stack([ctl.build_ref_traj(xk[b], r_v[b], targets[b], N, 4, step_fraction=0.2) for b in range(B)])
            out = solver.solve_batch(xk, u_prev, theta, Rref, prm, w_warm=w, want_w=True, rls_P=P, rls_phi=phi,
                                     rls_y=y, rls_lambda=lam)
            theta, P, w = out["theta"], out["rls_P"], out["w"]
            u = out["u0"]
            ST[k] = out["status"]
            if cross:
                XS[k], US[k], IT[k], ROT[k] = xk, u, out["iters"], plant.x[:, 4:]
            en = np.linalg.norm(xk[:, [0, 2]] - targets[:, [0, 2]], axis=1)
            for b in np.where(~done)[0]:
                lg = logs[b]
                lg["pos_err"].append([targets[b, 0] - xk[b, 0], targets[b, 2] - xk[b, 2]])
                lg["pos_err_norm"].append(float(en[b]))
                lg["u_cmd"].append(u[b].copy())
                lg["torque"].append(np.zeros(14))                # arms are not simulated here
                lg["timestep"].append(k * Ts)
                if en[b] < pos_tol:
                    done[b] = True
            prev = xk
            u_prev = u.copy()
            plant.step(-u if cross else u)
            if done.all():
                break
    finally:
        solver.close()
    n = k + 1
    M = rollout_metrics(XS[:n], targets, US[:n], ST[:n], IT[:n], ROT[:n], Ts) if cross else None
    episodes = []
    for b in range(B):
        eps = {}
        add_episode(eps, "ep1", logs[b]["pos_err"], logs[b]["pos_err_norm"], logs[b]["u_cmd"], logs[b]["torque"],
                    logs[b]["timestep"])
        if cross:
            eps.update(rot=ROT[:n, b], metrics=M[b])
        episodes.append(eps)
    return episodes, ST[:k + 1], done


# ---------------------------------------------------------------------------------------------
# the same closed loops, resident on the device (dart_pmpc_rollout / dart_rmpc_rollout): per step one loop-step
# kernel and the solve, on one stream, no host round trip; the logs come back with one download per call
def rollout_pmpc(states0, targets, prm, steps: int, N: int = 20, Ts: float = 0.002, tol: float = 1e-8, device: int = 0,
                 plant_kw: dict | None = None, plant_pvec=None, x_rot0=None, return_logs: bool = False,
                 metrics_only: bool = False):
    """``run_pmpc`` on the device: same arguments, same return values (AsyncLogger log dicts with metrics, statuses
    [steps, B]).  ``solve_time`` is the rollout's wall time divided by the steps run.  ``return_logs``: also
    return dict(iters [steps, B], solve_time).  With ``plant_pvec`` the loop runs on the LMPC plant
    (dart_pmpc_lm_rollout); ``metrics_only`` (with ``plant_pvec``) writes and moves no log and returns only the
    metrics [B, 8] (_lib.METRIC_SLOTS)."""
    from ._lib import PMPC_LOOP_STATE, PMPC_LOOP_LOGS, PMPC_LM_LOOP_LOGS, loop_logs, loop_metrics, plant_config
    states0 = np.asarray(states0, float).reshape(-1, 6)
    B = states0.shape[0]
    targets = np.asarray(targets, float).reshape(B, 6)
    prm = np.asarray(prm, float).reshape(B, 6)
    cross = plant_pvec is not None
    if metrics_only and not cross:
        raise ValueError("metrics_only needs plant_pvec (the tray-plant rollout has no streaming metrics)")
    plant = plant_config(**{k: v for k, v in (plant_kw or {}).items()})
    if cross:
        state = {"x": _cross_plant(states0[:, :4], x_rot0, plant_pvec, Ts, None).x, "tilt": np.zeros((B, 2)),
                 "metrics": loop_metrics(B)}
        lg = None if metrics_only else loop_logs(PMPC_LM_LOOP_LOGS, steps, B)
    else:
        state = {"x": states0.copy(), "tilt": np.zeros((B, 2))}
        assert set(state) == {n for n, _, _ in PMPC_LOOP_STATE}
        lg = loop_logs(PMPC_LOOP_LOGS, steps, B)
    solver = Solver(N=N, Ts=Ts, tol=tol, B_max=max(B, 1), device=device)
    try:
        t0 = time.perf_counter()
        if cross:
            solver.rollout_lm(0, steps, targets, prm, plant_pvec, states0[:, 4:6], state, lg, plant=plant)
        else:
            solver.rollout(0, steps, targets, prm, state, lg, plant=plant)
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    if metrics_only:
        return state["metrics"]
    t = np.arange(steps) * Ts
    TS = np.full(steps, wall / max(steps, 1))
    logs = []
    for b in range(B):
        d = {"t": t, "X": lg["X"][:, b], "X_target": np.tile(targets[b], (steps, 1)), "U_cmd": lg["U_cmd"][:, b],
             "quat_tray": lg["quat_tray"][:, b], "loss": lg["loss"][:, b], "solve_time": TS.copy()}
        for key, w in (("torques", 7), ("qpos", 7), ("qvel", 7), ("ee_pos", 3), ("ee_vel", 6)):
            d["L_" + key] = np.zeros((steps, w))       # arms are not simulated here
            d["R_" + key] = np.zeros((steps, w))
        d.update(logger_metrics(d, Ts))
        if cross:
            d.update(rot=lg["rot"][:, b], metrics=state["metrics"][b])
        logs.append(d)
    if return_logs:
        return logs, lg["status"], {"iters": lg["iters"], "solve_time": wall / max(steps, 1)}
    return logs, lg["status"]


def rollout_rmpc(x0, targets, steps: int, N: int = 20, Ts: float = 0.002, prm=None, device: int = 0,
                 pos_tol: float = ERROR_THRESHOLD, plant_kw: dict | None = None, mu=0.1, dr_max: float = 0.01,
                 alpha_rg: float = 0.5, lam: float = 0.995, P0: float = 1e3, plant_pvec=None, x_rot0=None,
                 check_every: int = 0, return_logs: bool = False, metrics_only: bool = False):
    """``run_rmpc`` on the device: same arguments, same return values (episodes per experiment in the rob_ctrl.py
    JSON layout, statuses [steps run, B], done).  ``check_every`` > 0 runs the rollout in chunks of that many steps
    and stops once every experiment's episode has closed (the state stays valid between calls); 0 runs all
    ``steps`` in one call.  ``return_logs``: also return the per-step device logs (x, theta, r_v, f, status,
    iters [steps run, B, ...]), the episode rows, the final loop state and ``solve_time``.  With ``plant_pvec`` the
    loop runs on the LMPC plant (dart_rmpc_lm_rollout; ``mu`` is then not used); ``metrics_only`` (with ``plant_pvec``)
    writes and moves no log and returns only the metrics [B, 8] (_lib.METRIC_SLOTS)."""
    from ._lib import RMPC_LOOP_LOGS, RMPC_LM_LOOP_LOGS, loop_logs, plant_config, rmpc_loop_config
    x0 = np.asarray(x0, float).reshape(-1, 4)
    B = x0.shape[0]
    targets = np.asarray(targets, float).reshape(B, 4)
    ctl = AdaptiveNPMPCSmooth(None, None, Ts=Ts, N=N, Qp=80.0, Qv=2.0, Ru=0.02, Rdu=1.0, u_bounds=(-0.6, 0.6),
                              du_bounds=(-0.06, 0.06), vmax=0.2, v_eps=0.1)          # rob_ctrl.py:280-283
    prm = np.tile(ctl.params(), (B, 1)) if prm is None else np.asarray(prm, float).reshape(B, 10)
    plant = plant_config(**{k: v for k, v in (plant_kw or {}).items()})
    loop = rmpc_loop_config(dr_max=dr_max, alpha_rg=alpha_rg, rls_lambda=lam, pos_tol=pos_tol)
    cross = plant_pvec is not None
    if metrics_only and not cross:
        raise ValueError("metrics_only needs plant_pvec (the tray-plant rollout has no streaming metrics)")
    lg = None if metrics_only else loop_logs(RMPC_LM_LOOP_LOGS if cross else RMPC_LOOP_LOGS, steps, B)
    solver = RmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device)
    chunk = int(check_every) if check_every and check_every > 0 else max(steps, 1)
    k = 0
    try:
        state = solver.loop_state_lm(x0, x_rot0, P0) if cross else solver.loop_state(x0, P0)
        t0 = time.perf_counter()
        while k < steps:
            n = min(chunk, steps - k)
            if cross:
                solver.rollout_lm(k, n, targets, prm, plant_pvec, state, lg, plant=plant, loop=loop)
            else:
                solver.rollout(k, n, targets, prm, mu, state, lg, plant=plant, loop=loop)
            k += n
            if state["done"].all():
                break
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    if metrics_only:
        return state["metrics"]
    done = state["done"].astype(bool)
    episodes = []
    for b in range(B):
        n = int(state["nlog"][b])
        eps = {}
        add_episode(eps, "ep1", lg["pos_err"][:n, b].tolist(), lg["pos_err_norm"][:n, b].tolist(),
                    list(lg["u_cmd"][:n, b]), [np.zeros(14) for _ in range(n)],      # arms are not simulated here
                    lg["timestep"][:n, b].tolist())
        if cross:
            eps.update(rot=lg["rot"][:k, b], metrics=state["metrics"][b])
        episodes.append(eps)
    if return_logs:
        extra = {name: lg[name][:k] for name in ("x", "theta", "r_v", "f", "status", "iters")}
        extra.update(state=state, solve_time=wall / max(k, 1),
                     episode_rows={name: lg[name] for name in ("pos_err", "pos_err_norm", "u_cmd", "timestep")})
        return episodes, lg["status"][:k], done, extra
    return episodes, lg["status"][:k], done


# ---------------------------------------------------------------------------------------------
# LMPC: LMPC/src/run.py:256-286 without MuJoCo
LMPC_G = 9.81                  # rlmpc2.py:354


class LmpcPlant:
    """B objects on B tilting trays that obey the LMPC model itself (safe_dynamics, rlmpc2.py:260-429: translation
    with Stribeck friction and rolling, rotation with slip torque, rotational Stribeck friction, damping and
    toppling), each with its own true parameter vector ``pvec`` [B, 34] (index map :301-334; squash_param
    |p| + 1e-6), integrated with RK4 at ``dt`` (:431-436, tilt held within a step).

    state x = [px, vx, py, vy, th_x, om_x, th_y, om_y]; tilt = [a, b] follows the command through TrayPlant's
    first-order lag.  The model's Stribeck terms are its Coulomb friction, so TrayPlant's ``mu_c`` / ``v_c`` have
    no counterpart.  The driver's ``u_cmd *= -1`` and quaternion (run.py:257-261) are MuJoCo tray conventions and
    are not applied, as in TrayPlant."""

    def __init__(self, x0, pvec, tau=0.03, dt=0.002):
        self.x = np.array(x0, dtype=float).reshape(-1, 8).copy()
        B = self.x.shape[0]
        self.pvec = np.array(pvec, dtype=float).reshape(B, 34).copy()
        self.tilt = np.zeros((B, 2))
        self.a_lag = 1.0 - np.exp(-dt / tau) if tau > 0 else 1.0
        self.dt = float(dt)

    @staticmethod
    def _stribeck(v, F_s, F_c, Bv, v_s, eps):
        e = np.exp(-np.abs(v) / (v_s + 1e-12))                              # :372-376
        return np.tanh(v / eps) * (F_c + (F_s - F_c) * e) + Bv * v

    def _f(self, x, sa, sb):
        p = self.pvec
        sq = lambda i: np.abs(p[:, i]) + 1e-6                               # :296-298
        m_x, m_y, c_x, c_y, k_x, k_y = (sq(i) for i in range(6))
        sx = (p[:, 6], p[:, 7], p[:, 8], sq(9), sq(10))
        sy = (p[:, 11], p[:, 12], p[:, 13], sq(14), sq(15))
        I_x, I_y, r_x, r_y, c_rot_x, c_rot_y = (sq(i) for i in range(16, 22))
        srx = (p[:, 22], p[:, 23], p[:, 24], sq(25), sq(26))
        sry = (p[:, 27], p[:, 28], p[:, 29], sq(30), sq(31))
        h_com_x, h_com_y = sq(32), sq(33)
        px, vx, py, vy, th_x, om_x, th_y, om_y = (x[:, i] for i in range(8))
        g = LMPC_G
        Gx = m_x * (g * sa)                                                 # :353-357
        Gy = m_y * (g * sb)
        Ff_x = self._stribeck(vx, *sx)                                      # :379-380
        Ff_y = self._stribeck(vy, *sy)
        v_slip_x = vx - r_x * om_y                                          # :387-391
        v_slip_y = vy - (-r_y * om_x)
        F_roll_x = self._stribeck(v_slip_x, *sx)                            # :395-396
        F_roll_y = self._stribeck(v_slip_y, *sy)
        tau_slip_x = -r_y * F_roll_y                                        # :402-403
        tau_slip_y = -r_x * F_roll_x
        T_noslip_x = self._stribeck(om_x, *srx)
        T_noslip_y = self._stribeck(om_y, *sry)
        T_damp_x = c_rot_x * om_x                                           # :410-411
        T_damp_y = c_rot_y * om_y
        tau_topple_x = -m_y * g * h_com_x * np.sin(th_x)                    # :414-415
        tau_topple_y = -m_x * g * h_com_y * np.sin(th_y)
        tau_x = tau_slip_x - T_noslip_x - T_damp_x + tau_topple_x           # :418-419
        tau_y = tau_slip_y - T_noslip_y - T_damp_y + tau_topple_y
        al_x = tau_x / (I_x + 1e-12)                                        # :422-423
        al_y = tau_y / (I_y + 1e-12)
        rhs_x = Gx - c_x * vx - k_x * px - Ff_x - F_roll_x                  # :427
        rhs_y = Gy - c_y * vy - k_y * py - Ff_y - F_roll_y
        return np.stack([vx, rhs_x / m_x, vy, rhs_y / m_y, om_x, al_x, om_y, al_y], axis=1)       # :429

    def step(self, u_cmd):
        self.tilt += self.a_lag * (np.asarray(u_cmd, float).reshape(-1, 2) - self.tilt)
        s = np.sin(self.tilt)
        sa, sb = s[:, 0], s[:, 1]
        h, x = self.dt, self.x
        k1 = self._f(x, sa, sb)
        k2 = self._f(x + 0.5 * h * k1, sa, sb)
        k3 = self._f(x + 0.5 * h * k2, sa, sb)
        k4 = self._f(x + h * k3, sa, sb)
        self.x = x + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6
        return self.x


def lmpc_noise(noise_seed, steps: int, B: int):
    """The policy's standard-normal draws of a run, [steps, B, 34] fp32 (row k: step k); ``None`` = zero noise."""
    if noise_seed is None:
        return np.zeros((steps, B, 34), np.float32)
    return np.random.default_rng(noise_seed).standard_normal((steps, B, 34)).astype(np.float32)


def _lmpc_setup(x0, targets, plant_pvec, prm, policy_seed, model_params):
    from .lmpc import LmpcPolicy
    from ._lib import LMPC_PRM_DEFAULT
    x0 = np.asarray(x0, float).reshape(-1, 8)
    B = x0.shape[0]
    targets = np.asarray(targets, float).reshape(B, 8)
    plant_pvec = np.asarray(plant_pvec, float).reshape(B, 34)
    prm = np.tile(LMPC_PRM_DEFAULT, (B, 1)) if prm is None else np.asarray(prm, float).reshape(B, 22)
    policy = None if policy_seed is None else LmpcPolicy(B, seed=policy_seed)
    if policy is None:
        model_params = (plant_pvec if model_params is None else np.asarray(model_params, float).reshape(B, 34)).copy()
    return x0, B, targets, plant_pvec, prm, policy, model_params


def _lmpc_result(B, steps, Ts, targets, lg, final_x, state, wall, return_logs):
    after = np.concatenate([lg["X"][1:], final_x[None]], axis=0) if steps else lg["X"]     # run.py:286: after the step
    t = np.arange(steps) * Ts
    logs = [{"pos_error": lg["pos_error"][:, b], "u_cmd": lg["U_cmd"][:, b], "timestep": t.copy(), "state": after[:, b],
             "loss": lg["loss"][:, b]} for b in range(B)]
    if return_logs:
        return logs, lg["status"], {"iters": lg["iters"], "pvec": lg["pvec"], "X": lg["X"], "state": state,
                                    "solve_time": wall / max(steps, 1)}
    return logs, lg["status"]


def run_lmpc(x0, targets, plant_pvec, steps: int, N: int = 30, policy_seed=0, noise_seed=None, Ts: float = 0.002,
             prm=None, device: int = 0, plant_kw: dict | None = None, model_params=None, return_logs: bool = False):
    """B LMPC experiments in lock step (LMPC/src/run.py:256-286 without MuJoCo): per step one fused policy step +
    solve (``policy_solve_batch``), warm-started from the previous optimum (rlmpc2.py:494-524), then ``LmpcPlant``
    with the true parameters ``plant_pvec`` [B, 34].  x0, targets [B, 8].  ``policy_seed`` seeds a fresh
    ``LmpcPolicy``; None runs without a policy, every solve using ``model_params`` (default ``plant_pvec``).
    ``noise_seed`` seeds the policy's draws (``lmpc_noise``; None: zero noise).

    Returns per-experiment dicts with run.py's logged keys (pos_error, u_cmd, timestep, state -- the state after
    the step, :286 -- plus loss) and the solver statuses [steps, B]; ``return_logs`` adds dict(iters, pvec
    [steps, B, 34], X [steps, B, 8] the states the solves saw, state = the final loop state, solve_time)."""
    from ._lib import LMPC_LOOP_LOGS, LmpcSolver, loop_logs
    from .lmpc import policy_solve_batch
    x0, B, targets, plant_pvec, prm, policy, model_params = _lmpc_setup(x0, targets, plant_pvec, prm, policy_seed,
                                                                        model_params)
    noise = lmpc_noise(noise_seed, steps, B)
    lg = loop_logs(LMPC_LOOP_LOGS, steps, B)
    plant = LmpcPlant(x0, plant_pvec, dt=Ts, **(plant_kw or {}))
    solver = LmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device)
    u_prev, w = np.zeros((B, 2)), np.zeros((B, solver.nw))
    wall = 0.0
    try:
        for k in range(steps):
            lg["X"][k] = plant.x
            t0 = time.perf_counter()
            if policy is not None:
                out = policy_solve_batch(solver, policy, plant.x, u_prev, targets, prm, w_warm=w, want_w=True,
                                         noise=noise[k])
                lg["pvec"][k] = policy.model_params
            else:
                out = solver.solve_batch(plant.x, u_prev, model_params, targets, prm, w_warm=w, want_w=True)
                lg["pvec"][k] = model_params
            wall += time.perf_counter() - t0
            w, u_prev = out["w"], out["u0"].copy()
            lg["U_cmd"][k], lg["loss"][k], lg["status"][k], lg["iters"][k] = out["u0"], out["f"], out["status"], out["iters"]
            xn = plant.step(out["u0"])
            dx, dy = xn[:, 0] - targets[:, 0], xn[:, 2] - targets[:, 2]
            lg["pos_error"][k] = np.sqrt(dx * dx + dy * dy)                 # run.py:274
    finally:
        solver.close()
    state = {"x": plant.x.copy(), "tilt": plant.tilt.copy(), "u_prev": u_prev, "w": w,
             "model_params": policy.model_params.copy() if policy is not None else model_params}
    if policy is not None:
        state.update(obs_mean=policy.obs_mean, obs_M2=policy.obs_M2, obs_count=policy.obs_count,
                     history=policy.history.reshape(B, 520), timestep=policy.timestep)
    return _lmpc_result(B, steps, Ts, targets, lg, plant.x, state, wall, return_logs)


def rollout_lmpc(x0, targets, plant_pvec, steps: int, N: int = 30, policy_seed=0, noise_seed=None, Ts: float = 0.002,
                 prm=None, device: int = 0, plant_kw: dict | None = None, model_params=None,
                 return_logs: bool = False):
    """``run_lmpc`` on the device (dart_lmpc_rollout): same arguments, same return values.  ``solve_time`` is the
    rollout's wall time divided by the steps run."""
    from ._lib import LMPC_LOOP_LOGS, LmpcSolver, loop_logs, plant_config
    x0, B, targets, plant_pvec, prm, policy, model_params = _lmpc_setup(x0, targets, plant_pvec, prm, policy_seed,
                                                                        model_params)
    noise = lmpc_noise(noise_seed, steps, B) if (policy is not None and noise_seed is not None) else None
    lg = loop_logs(LMPC_LOOP_LOGS, steps, B)
    plant = plant_config(**{k: v for k, v in (plant_kw or {}).items()})
    solver = LmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device)
    try:
        state = solver.loop_state(x0, policy=policy, model_params=model_params)
        t0 = time.perf_counter()
        solver.rollout(0, steps, targets, plant_pvec, state, lg, policy=policy, prm=prm, noise=noise, plant=plant)
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    return _lmpc_result(B, steps, Ts, targets, lg, state["x"], state, wall, return_logs)


def evaluate_lmpc(x0, targets, plant_pvec, steps: int, policies, N: int = 30, noise_seed=None,
                  metrics_only: bool = True, Ts: float = 0.002, prm=None, device: int = 0,
                  plant_kw: dict | None = None, model_params=None):
    """P LMPC policies on the same B experiments in one device-resident rollout (dart_lmpc_eval): ``policies`` is a
    list of P ``LmpcPolicy(B)`` (sharing one policy config), or one, or None for the loop without a policy (every solve
    uses ``model_params``, default ``plant_pvec``).  ``x0``, ``targets`` [B, 8] and ``plant_pvec`` [B, 34] are one
    learner's and are used for every learner.  The evaluation runs on copies of the policies' state (observation
    statistics, history, timestep, model_params): a policy passed in is not advanced.  ``noise_seed`` None is zero
    noise -- the policy's mean action, the deterministic evaluation; otherwise every learner sees the draws of
    ``lmpc_noise(noise_seed, steps, B)``.

    Returns {"metrics": [P, B, 8] (_lib.METRIC_SLOTS), "scores": [P, 8] (_lib.SCORE_SLOTS)}; ``metrics_only`` False
    also logs every step and adds "logs" and "status": per learner what ``rollout_lmpc`` returns."""
    from . import _lib
    if policies is not None and not isinstance(policies, (list, tuple)):
        policies = [policies]
    x0, B, targets, plant_pvec, prm, _, model_params = _lmpc_setup(x0, targets, plant_pvec, prm, None, model_params)
    P = len(policies) if policies is not None else 1
    if policies is not None:
        if P < 1 or any(p.B != B for p in policies):
            raise ValueError(f"policies: a list of LmpcPolicy({B})")
        if any(bytes(p.cfg) != bytes(policies[0].cfg) for p in policies):
            raise ValueError("policies: one policy config for the whole population")
    tile = lambda a: np.ascontiguousarray(np.tile(a, (P,) + (1,) * (a.ndim - 1)))
    noise = None
    if policies is not None and noise_seed is not None:
        noise = np.ascontiguousarray(np.tile(lmpc_noise(noise_seed, steps, B), (1, P, 1)))
    plant = _lib.plant_config(**{k: v for k, v in (plant_kw or {}).items()})
    solver = _lib.LmpcSolver(N=N, Ts=Ts, B_max=max(P * B, 1), device=device)
    try:
        members = [solver.loop_state(x0, policy=p) for p in policies] if policies is not None \
            else [solver.loop_state(x0, model_params=model_params)]
        state = {name: np.concatenate([m[name] for m in members], axis=0) for name in members[0]}
        state["metrics"] = _lib.loop_metrics(P * B)
        lg = None if metrics_only else _lib.loop_logs(_lib.LMPC_LOOP_LOGS, steps, P * B)
        scores = np.zeros((P, 8))
        t0 = time.perf_counter()
        solver.evaluate(P, 0, steps, tile(targets), tile(plant_pvec), state, lg,
                        pcfg=policies[0].cfg if policies is not None else None,
                        weights=np.stack([p.weights for p in policies]) if policies is not None else None,
                        current_k=np.concatenate([p.current_k for p in policies]) if policies is not None else None,
                        prm=tile(prm), noise=noise, scores=scores, plant=plant)
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    out = {"metrics": state["metrics"].reshape(P, B, 8), "scores": scores}
    if not metrics_only:
        out["logs"], out["status"] = [], []
        for l in range(P):
            sl = slice(l * B, (l + 1) * B)
            logs, st = _lmpc_result(B, steps, Ts, targets, {k: v[:, sl] for k, v in lg.items()}, state["x"][sl], None, wall,
                                    False)
            out["logs"].append(logs); out["status"].append(st)
    return out


def compare_controllers(x0, target_xy, plant_pvec, steps: int, N: int = 20, lmpc_N: int = 30, Ts: float = 0.002,
                        pmpc_prm=None, pz_vz=(0.4, 0.0), lmpc_policy_seed=None, device: int = 0,
                        plant_kw: dict | None = None, lmpc_policies=None):
    """PMPC, RMPC and LMPC on the same objects: B experiments from the states ``x0`` [B, 8] (LmpcPlant's layout) to the
    targets ``target_xy`` [B, 2] on ``LmpcPlant`` with the true parameters ``plant_pvec`` [B, 34], ``steps`` steps each.
    PMPC and RMPC run through the cross-plant rollouts in metrics-only mode; LMPC runs through ``rollout_lmpc``
    (``lmpc_policy_seed`` None: every solve uses ``plant_pvec`` as its model) and ``rollout_metrics`` of its logs.
    ``pmpc_prm`` [B, 6]: PMPC's parameter rows, default [c_x / m_x of the plant, 600, 5, 0.1, -0.6, 0.6] (the cube's
    weights, main_parallel_enhanced.py:171-179).  Returns {"PMPC", "RMPC", "LMPC"}: metrics [B, 8] each
    (_lib.METRIC_SLOTS).  ``lmpc_policies`` (one ``LmpcPolicy(B)`` or a list of P) routes LMPC through
    ``evaluate_lmpc`` instead, its metrics made on the device and no log moved: "LMPC" is then [B, 8] for one policy and
    [P, B, 8] for a list."""
    x0 = np.asarray(x0, float).reshape(-1, 8)
    B = x0.shape[0]
    txy = np.asarray(target_xy, float).reshape(B, 2)
    plant_pvec = np.asarray(plant_pvec, float).reshape(B, 34)
    zz = np.broadcast_to(np.asarray(pz_vz, float), (B, 2))
    if pmpc_prm is None:
        pmpc_prm = np.tile([0.0, 600.0, 5.0, 0.1, -0.6, 0.6], (B, 1))
        pmpc_prm[:, 0] = (np.abs(plant_pvec[:, 2]) + 1e-6) / (np.abs(plant_pvec[:, 0]) + 1e-6)
    s6 = np.concatenate([x0[:, :4], zz], axis=1)
    t6 = np.stack([txy[:, 0], np.zeros(B), txy[:, 1], np.zeros(B), zz[:, 0], np.zeros(B)], axis=1)
    t4, t8 = t6[:, :4], np.concatenate([t6[:, :4], np.zeros((B, 4))], axis=1)
    out = {"PMPC": rollout_pmpc(s6, t6, pmpc_prm, steps, N=N, Ts=Ts, device=device, plant_kw=plant_kw,
                                plant_pvec=plant_pvec, x_rot0=x0[:, 4:], metrics_only=True),
           "RMPC": rollout_rmpc(x0[:, :4], t4, steps, N=N, Ts=Ts, device=device, plant_kw=plant_kw, pos_tol=0.0,
                                plant_pvec=plant_pvec, x_rot0=x0[:, 4:], metrics_only=True)}
    if lmpc_policies is not None:
        m = evaluate_lmpc(x0, t8, plant_pvec, steps, lmpc_policies, N=lmpc_N, Ts=Ts, device=device,
                          plant_kw={k: v for k, v in (plant_kw or {}).items() if k == "tau"})["metrics"]
        out["LMPC"] = m if isinstance(lmpc_policies, (list, tuple)) else m[0]
        return out
    logs, st, X = rollout_lmpc(x0, t8, plant_pvec, steps, N=lmpc_N, policy_seed=lmpc_policy_seed, Ts=Ts, device=device,
                               plant_kw={k: v for k, v in (plant_kw or {}).items() if k == "tau"}, return_logs=True)
    U = np.stack([lg["u_cmd"] for lg in logs], axis=1)
    out["LMPC"] = rollout_metrics(X["X"], t8, U, st, X["iters"], X["X"][:, :, 4:], Ts)
    return out


# ---------------------------------------------------------------------------------------------
# LMPC experience collection: the training half of RLMPC._rl_worker (rlmpc2.py:537-938) up to the PPO update
LOG_SQRT_2PI = np.float32(0.91893853320467274178)


def _unpack_f32(w, shapes):
    w = np.asarray(w, np.float32)
    out, o = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(w[o:o + n].reshape(shape)); o += n
    return out


def lmpc_actor_mean(weights, obs):
    """Policy.mean_net (:39-46) on obs [B, 520] in fp32; returns (mean [B, 34], the unclamped log_std [34])."""
    W1, b1, W2, b2, W3, b3, log_std = _unpack_f32(weights, ((520, 64), (64,), (64, 64), (64,), (64, 34), (34,), (34,)))
    obs = np.asarray(obs, np.float32)
    h1 = np.tanh(obs @ W1 + b1).astype(np.float32)
    h2 = np.tanh(h1 @ W2 + b2).astype(np.float32)
    return (h2 @ W3 + b3).astype(np.float32), log_std


def lmpc_critic_value(critic, obs):
    """Policy.value_net (:48-55) on obs [B, 520] in fp32: value [B]."""
    V1, c1, V2, c2, V3, c3 = _unpack_f32(critic, ((520, 64), (64,), (64, 64), (64,), (64,), (1,)))
    obs = np.asarray(obs, np.float32)
    g1 = np.tanh(obs @ V1 + c1).astype(np.float32)
    g2 = np.tanh(g1 @ V2 + c2).astype(np.float32)
    return (g2 @ V3 + c3[0]).astype(np.float32)


def lmpc_log_prob(mean, log_std, raw, log_std_min, log_std_max):
    """Normal(mean, exp(clamp(log_std))).log_prob(raw).sum(-1) (:699) in fp32: [B]."""
    lsd = np.clip(np.asarray(log_std, np.float32), np.float32(log_std_min), np.float32(log_std_max))
    sd = np.exp(lsd).astype(np.float32)
    z = (np.asarray(raw, np.float32) - np.asarray(mean, np.float32)).astype(np.float32)
    lp = -(z * z) / (np.float32(2) * (sd * sd)) - lsd - LOG_SQRT_2PI
    return lp.astype(np.float32).sum(axis=-1, dtype=np.float32)


def lmpc_change_cost(raw, max_delta, action_scale, max_per_dim_rms):
    """|delta_z| of :680-709 per instance, on fp32 values as the reference's tensors: delta_z = raw (max_delta
    action_scale), damped by max_per_dim_rms / (rms + 1e-12) when rms = |delta_z| / sqrt(34) exceeds it."""
    raw = np.asarray(raw, np.float32).reshape(-1, 34)
    out = np.empty(raw.shape[0])
    for b, r in enumerate(raw):
        dz = r * np.float32(max_delta * action_scale)
        rms = float(np.linalg.norm(dz)) / np.sqrt(34)
        if rms > max_per_dim_rms:
            dz = dz * np.float32(max_per_dim_rms / (rms + 1e-12))
        out[b] = float(np.linalg.norm(dz))
    return out


def lmpc_reward_step(rcfg, cs, x, target, control, raw, max_delta=0.02, action_scale=1.0):
    """Reward, done and the episode bookkeeping of one step for B controllers (:703-740, :771-773, :900-935), the
    batched numpy statement of what lmpc_experience_kernel computes: fp64, except change_cost (fp32, :680-709).

    ``x`` [B, 8] is the state the solve saw, ``control`` [B, 2] the u_prev policy step k observed, ``raw`` [B, 34]
    the drawn action.  ``cs`` (``LmpcSolver.collect_state``) is advanced in place: prev_cmd, ep_step, ep_return,
    time_penalty and, at an episode end, episodes, last_return, last_steps.  The in_contact penalty (:735) is left
    out (LmpcPlant has no contact model).  Returns (reward [B] float64, done [B] int32: bit 1 out of bounds, bit 2
    max_episode_steps)."""
    x, target, control = (np.asarray(a, float) for a in (x, target, control))
    pos_err = np.sqrt(np.abs(target[:, 0] - x[:, 0]) ** 2 + np.abs(target[:, 2] - x[:, 2]) ** 2)
    vel_err = np.sqrt(x[:, 1] ** 2 + x[:, 3] ** 2)
    e_p = np.exp(-(pos_err ** 2) / (2 * rcfg.sigma_pos ** 2))
    e_v = np.exp(-(vel_err ** 2) / (2 * rcfg.sigma_vel ** 2))
    prox = rcfg.w_pos * e_p + rcfg.w_vel * e_p * e_v
    change = lmpc_change_cost(raw, max_delta, action_scale, rcfg.max_per_dim_rms)
    rate = np.abs(control[:, 0] - cs["prev_cmd"][:, 0]) + np.abs(control[:, 1] - cs["prev_cmd"][:, 1])
    cs["prev_cmd"][:] = control
    reward = prox - rcfg.w_change * change - rcfg.w_d_ctrl * rate - cs["time_penalty"]
    reward = np.where((pos_err < rcfg.success_tol) & (vel_err < rcfg.success_tol), reward + rcfg.success_bonus, reward)
    cs["ep_step"] += 1
    oob = (np.abs(x[:, 0]) > rcfg.tray_limit[0]) | (np.abs(x[:, 2]) > rcfg.tray_limit[1])
    reward = np.where(oob, reward - rcfg.oob_penalty, reward)
    done = (oob * 1 + (cs["ep_step"] >= rcfg.max_episode_steps) * 2).astype(np.int32)
    cs["time_penalty"] += rcfg.time_penalty_rate
    cs["ep_return"] += reward
    end = done != 0
    cs["last_return"][end] = cs["ep_return"][end]
    cs["last_steps"][end] = cs["ep_step"][end]
    cs["episodes"][end] += 1
    cs["ep_return"][end] = 0.0
    cs["ep_step"][end] = 0
    cs["time_penalty"][end] = 0.0
    return reward, done


def lmpc_mean_param_update(weights, history, model_params, pcfg=None):
    """The mean-based parameter write after an update (:876-896) for B controllers, the batched numpy statement of
    what lmpc_mean_update_kernel computes: the actor's mean on the current ``history`` [B, 520] (fp32; nothing of the
    policy's state changes), k <- k_max sigmoid(logit(clamp(k / k_max, min_k / k_max, 1 - 1e-6)) + mean max_delta
    action_scale) on fp32 tensors (:888-893), then the EMA and the tanh soft clip of write_params_to_shm (:606-616)
    in fp64.  ``pcfg``: a ``dart_mpc.lmpc.PolicyConfig`` (default: the library's).  Returns (mean float32 [B, 34],
    the new model_params float64 [B, 34], which the worker also takes as its current_k, :896)."""
    if pcfg is None:
        from .lmpc import policy_config
        pcfg = policy_config()
    mean, _ = lmpc_actor_mean(weights, np.asarray(history, np.float32).reshape(-1, 520))
    prev = np.asarray(model_params, np.float64).reshape(-1, 34)
    f32 = np.float32
    kmax = f32(pcfg.k_max)
    frac = np.clip(prev.astype(f32) / kmax, f32(pcfg.min_k / pcfg.k_max), f32(1.0) - f32(1e-6)).astype(f32)
    z_prev = np.log(frac / (f32(1.0) - frac)).astype(f32)
    z_new = (z_prev + mean * f32(pcfg.max_delta) * f32(pcfg.action_scale)).astype(f32)
    k_new = (kmax * (f32(1.0) / (f32(1.0) + np.exp(-z_new).astype(f32)))).astype(f32)
    smoothed = pcfg.smooth_alpha * k_new.astype(np.float64) + (1.0 - pcfg.smooth_alpha) * prev
    lo, hi = pcfg.min_k, pcfg.k_max - pcfg.k_ceiling_margin
    center, scale = 0.5 * (hi + lo), 0.5 * (hi - lo) - 1e-3
    return mean, center + scale * np.tanh((smoothed - center) / scale)


def philox4x32_10(counter, key):
    """Philox4x32-10 with the standard constants on broadcastable counter words (c0, c1, c2, c3) and key words
    (k0, k1): uint32 [..., 4].  The numpy statement of the generator of csrc/lmpc_train.hip."""
    u64, m = np.uint64, np.uint64(0xffffffff)
    c = [np.asarray(x, u64) & m for x in counter]
    k0, k1 = (np.asarray(x, u64) & m for x in key)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c[0], u64(0xCD9E8D57) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> u64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + u64(0x9E3779B9)) & m, (k1 + u64(0xBB67AE85)) & m
    return np.stack([x.astype(np.uint32) for x in np.broadcast_arrays(*c)], axis=-1)


def lmpc_train_words(seed, iteration, stream, epoch, n):
    """The n 32-bit words of (seed, iteration, stream, epoch): element e is word e % 4 of block e / 4, key
    (seed & 0xffffffff, seed >> 32), counter (block, iteration, stream, epoch); stream 0 = noise, 1 = permutations."""
    seed = int(seed)
    blocks = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    return philox4x32_10((blocks, int(iteration), int(stream), int(epoch)),
                         (seed & 0xffffffff, (seed >> 32) & 0xffffffff)).reshape(-1)[:int(n)]


def lmpc_train_noise(seed, iteration, steps, B, dtype=np.float64):
    """The exploration noise of dart_lmpc_noise restated in numpy, [steps, B, 34] in ``dtype`` arithmetic: u =
    ((word >> 9) + 0.5) 2^-23, words 0, 1 and 2, 3 of a block give one Box-Muller pair sqrt(-2 ln u0) (cos, sin)(2 pi
    u1) each; a tail uses the leading words of its block."""
    n = int(steps) * int(B) * 34
    w = lmpc_train_words(seed, iteration, 0, 0, 4 * ((n + 3) // 4))
    f = np.dtype(dtype).type
    u = ((w >> np.uint32(9)).astype(dtype) + f(0.5)) * f(2.0 ** -23)
    u0, u1 = u[0::2], u[1::2]
    rad, ang = np.sqrt(f(-2.0) * np.log(u0)), f(2.0 * np.pi) * u1
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).astype(dtype)
    return z.reshape(-1)[:n].reshape(int(steps), int(B), 34)


def lmpc_train_perms(seed, iteration, epochs, n):
    """The mini-batch permutations of dart_lmpc_perms restated in numpy: (perm int32 [epochs, n], keys uint32
    [epochs, n]); a permutation is the argsort of (key, index)."""
    keys = np.stack([lmpc_train_words(seed, iteration, 1, e, n) for e in range(int(epochs))]) if int(epochs) > 0 \
        else np.zeros((0, int(n)), np.uint32)
    idx = np.arange(int(n))
    perm = np.stack([np.lexsort((idx, k)) for k in keys]).astype(np.int32) if int(epochs) > 0 \
        else np.zeros((0, int(n)), np.int32)
    return perm, keys


def lmpc_train_choice(seed, iteration, n, m):
    """dart_lmpc_choice restated in numpy: ``m`` of ``n`` without replacement, int32 [m] -- the first m entries of
    the argsort of (key, index) over the n words of (seed, iteration, stream 2, epoch 0).  Stands in for the
    reference's ``rng.choice(len(buf), max(1, len(buf) // 4), replace=False)`` (rlmpc2.py:823-827)."""
    n, m = int(n), int(m)
    if not 1 <= m <= n:
        raise ValueError(f"a choice of m = {m} out of n = {n}")
    keys = lmpc_train_words(seed, iteration, 2, 0, n)
    return np.lexsort((np.arange(n), keys))[:m].astype(np.int32)


def gae_sequence(reward, value, done, last_value, gamma=0.99, lam=0.95, magnitude=False):
    """compute_gae (:592-599) over one sequence, the sequential recursion in fp64: (adv, ret = adv + value), [G].
    With ``magnitude`` the same recursion on |delta_t| (the bootstrap value enters through delta_{G-1} alone): the
    scale A_t = sum_k |c_t .. c_{t+k-1} delta_{t+k}| that the error of a reassociated evaluation is measured
    against; returns (A, A + |value|)."""
    rw = np.asarray(reward, np.float64).reshape(-1)
    rv, rd = np.asarray(value, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    G = rw.size
    adv = np.zeros(G)
    g, v_next = 0.0, float(np.asarray(last_value, np.float64).reshape(-1)[0])
    for s in reversed(range(G)):
        nd = 1.0 - rd[s]
        delta = rw[s] + gamma * v_next * nd - rv[s]
        if magnitude:
            delta = abs(delta)
        g = delta + gamma * lam * nd * g
        adv[s] = g
        v_next = rv[s]
    return adv, adv + (np.abs(rv) if magnitude else rv)


def gae_numpy(nrec, rec_reward, rec_value, rec_done, last_value, gamma=0.99, lam=0.95):
    """compute_gae (:592-599) per instance over its first nrec[b] records [rec_rows, B], fp64: (adv, ret = adv +
    value), NaN in the rows an instance has not recorded."""
    rw = np.asarray(rec_reward, float)
    rv, rd = np.asarray(rec_value, float), np.asarray(rec_done, float)
    rows, B = rw.shape
    adv, ret = np.full((rows, B), np.nan), np.full((rows, B), np.nan)
    for b in range(B):
        n = int(min(max(int(nrec[b]), 0), rows))
        g, v_next = 0.0, float(last_value[b])
        for s in reversed(range(n)):
            delta = rw[s, b] + gamma * v_next * (1.0 - rd[s, b]) - rv[s, b]
            g = delta + gamma * lam * (1.0 - rd[s, b]) * g
            adv[s, b], ret[s, b] = g, g + rv[s, b]
            v_next = rv[s, b]
    return adv, ret


def _collect_setup(B, steps, policy_seed, critic_seed, reset_pool, rec_rows, rcfg):
    from ._lib import LMPC_COLLECT_LOGS, LMPC_COLLECT_REC, LmpcSolver, loop_logs, reward_config
    from .lmpc import LmpcPolicy, init_critic_weights
    policy = LmpcPolicy(B, seed=policy_seed, critic_weights=init_critic_weights(critic_seed))
    rcfg = rcfg if rcfg is not None else reward_config()
    if rec_rows is None:
        rec_rows = steps // int(rcfg.record_every) + 1
    pool = None
    if reset_pool is not None:
        pool = {k: np.ascontiguousarray(reset_pool[k], np.float64) for k in ("reset_x", "reset_target", "reset_pvec")}
    cs = LmpcSolver.collect_state(np.zeros((B, 2)))
    return policy, rcfg, pool, cs, loop_logs(LMPC_COLLECT_LOGS, steps, B), loop_logs(LMPC_COLLECT_REC, rec_rows, B)


def _collect_result(res, cs, clogs, rec, targets, plant_pvec):
    exp = dict(rec)
    exp.update(clogs)
    exp.update(cs)
    exp.update(target=targets, plant_pvec=plant_pvec)
    return res + (exp,)


def run_lmpc_collect(x0, targets, plant_pvec, steps: int, N: int = 30, policy_seed=0, critic_seed=1, noise_seed=None,
                     Ts: float = 0.002, prm=None, device: int = 0, plant_kw: dict | None = None, rcfg=None,
                     reset_pool=None, rec_rows=None, policy=None, restoration: bool = True):
    """``run_lmpc`` with experience collection on the host, the loop a user would otherwise write: per step the fused
    policy step + solve, then in numpy the critic, the log-probability, ``lmpc_reward_step``, the record and the
    reset into the next episode from ``reset_pool`` (dict reset_x / reset_target [R, B, 8], reset_pvec [R, B, 34];
    None: episode ends only reset the counters).  ``rcfg`` is a ``reward_config()``; ``rec_rows`` defaults to what
    ``steps`` can fill.  Returns ``run_lmpc``'s (logs, statuses, extra) plus a dict of the records (rec_*), the
    per-step logs (reward, done, value, logp), the collection state and the final target / plant_pvec.
    ``policy`` (an ``LmpcPolicy`` with ``critic_weights``) replaces the seeded one; ``restoration`` is the solver's."""
    from ._lib import LMPC_LOOP_LOGS, LmpcSolver, loop_logs
    from .lmpc import policy_solve_batch
    x0, B, targets, plant_pvec, prm, _, _ = _lmpc_setup(x0, targets, plant_pvec, prm, None, None)
    targets, plant_pvec = targets.copy(), plant_pvec.copy()
    pol, rcfg, pool, cs, clogs, rec = _collect_setup(B, steps, policy_seed, critic_seed, reset_pool, rec_rows, rcfg)
    policy = policy if policy is not None else pol
    noise = lmpc_noise(noise_seed, steps, B)
    lg = loop_logs(LMPC_LOOP_LOGS, steps, B)
    plant = LmpcPlant(x0, plant_pvec, dt=Ts, **(plant_kw or {}))
    solver = LmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device, restoration=restoration)
    u_prev, w = np.zeros((B, 2)), np.zeros((B, solver.nw))
    every, rows = int(rcfg.record_every), rec["rec_reward"].shape[0]
    wall = 0.0
    try:
        for k in range(steps):
            xk = plant.x.copy()
            lg["X"][k] = xk
            t0 = time.perf_counter()
            out = policy_solve_batch(solver, policy, xk, u_prev, targets, prm, w_warm=w, want_w=True, noise=noise[k])
            obs = policy.history.reshape(B, 520)
            mean, log_std = lmpc_actor_mean(policy.weights, obs)
            value = lmpc_critic_value(policy.critic_weights, obs)
            logp = lmpc_log_prob(mean, log_std, out["action"], policy.cfg.log_std_min, policy.cfg.log_std_max)
            reward, done = lmpc_reward_step(rcfg, cs, xk, targets, u_prev, out["action"], policy.cfg.max_delta,
                                            policy.cfg.action_scale)
            clogs["reward"][k], clogs["done"][k], clogs["value"][k], clogs["logp"][k] = reward, done, value, logp
            cs["sticky"] |= done
            for b in np.where((policy.timestep - 1) % every == 0)[0]:
                n = int(cs["nrec"][b])
                if n < rows:
                    rec["rec_obs"][n, b], rec["rec_action"][n, b] = obs[b], out["action"][b]
                    rec["rec_logp"][n, b], rec["rec_value"][n, b], rec["rec_reward"][n, b] = logp[b], value[b], reward[b]
                    rec["rec_done"][n, b] = float((cs["sticky"][b] if rcfg.done_sticky else done[b]) != 0)
                    cs["nrec"][b] = n + 1
                cs["sticky"][b] = 0
            wall += time.perf_counter() - t0
            lg["pvec"][k] = policy.model_params
            w, u_prev = out["w"], out["u0"].copy()
            cs["control_seen"][:] = u_prev
            lg["U_cmd"][k], lg["loss"][k], lg["status"][k], lg["iters"][k] = out["u0"], out["f"], out["status"], out["iters"]
            xn = plant.step(out["u0"])
            dx, dy = xn[:, 0] - targets[:, 0], xn[:, 2] - targets[:, 2]
            lg["pos_error"][k] = np.sqrt(dx * dx + dy * dy)
            if pool is not None:
                for b in np.where(done != 0)[0]:
                    e = (int(cs["episodes"][b]) - 1) % pool["reset_x"].shape[0]
                    plant.x[b], plant.tilt[b] = pool["reset_x"][e, b], 0.0
                    targets[b], plant.pvec[b] = pool["reset_target"][e, b], pool["reset_pvec"][e, b]
    finally:
        solver.close()
    state = {"x": plant.x.copy(), "tilt": plant.tilt.copy(), "u_prev": u_prev, "w": w,
             "model_params": policy.model_params.copy(), "obs_mean": policy.obs_mean, "obs_M2": policy.obs_M2,
             "obs_count": policy.obs_count, "history": policy.history.reshape(B, 520), "timestep": policy.timestep}
    res = _lmpc_result(B, steps, Ts, targets, lg, plant.x, state, wall, True)
    return _collect_result(res, cs, clogs, rec, targets, plant.pvec.copy())


def collect_lmpc(x0, targets, plant_pvec, steps: int, N: int = 30, policy_seed=0, critic_seed=1, noise_seed=None,
                 Ts: float = 0.002, prm=None, device: int = 0, plant_kw: dict | None = None, rcfg=None,
                 reset_pool=None, rec_rows=None, policy=None, restoration: bool = True):
    """``run_lmpc_collect`` on the device (dart_lmpc_collect): same arguments, same return values."""
    from ._lib import LMPC_LOOP_LOGS, LmpcSolver, loop_logs, plant_config
    x0, B, targets, plant_pvec, prm, _, _ = _lmpc_setup(x0, targets, plant_pvec, prm, None, None)
    targets, plant_pvec = np.ascontiguousarray(targets.copy()), np.ascontiguousarray(plant_pvec.copy())
    pol, rcfg, pool, cs, clogs, rec = _collect_setup(B, steps, policy_seed, critic_seed, reset_pool, rec_rows, rcfg)
    policy = policy if policy is not None else pol
    noise = lmpc_noise(noise_seed, steps, B) if noise_seed is not None else None
    lg = loop_logs(LMPC_LOOP_LOGS, steps, B)
    plant = plant_config(**{k: v for k, v in (plant_kw or {}).items()})
    solver = LmpcSolver(N=N, Ts=Ts, B_max=max(B, 1), device=device, restoration=restoration)
    try:
        state = solver.loop_state(x0, policy=policy)
        t0 = time.perf_counter()
        solver.collect(0, steps, targets, plant_pvec, state, cs, lg, clogs, rec, policy, rcfg=rcfg, prm=prm, noise=noise,
                       pool=pool, plant=plant)
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    res = _lmpc_result(B, steps, Ts, targets, lg, state["x"], state, wall, True)
    return _collect_result(res, cs, clogs, rec, targets, plant_pvec)


# ---- the arm layer's closed loop (dart_dual_arm_rollout) ------------------------------------------------------------
def tray_poses_from_tilt(u_log, tray_pos):
    """Tray poses [K, E, 7] (pos | quat wxyz) from a tilt log ``u_log`` [K, E, 2] of the MPC rollouts and the tray
    position(s) ``tray_pos`` [3] or [E, 3]: the tilt -> quaternion step of PMPC/main.py:106-116 (``tilt_to_quat``)."""
    u = np.asarray(u_log, dtype=np.float64)
    K, E = u.shape[:2]
    out = np.empty((K, E, 7))
    out[..., :3] = np.broadcast_to(np.asarray(tray_pos, dtype=np.float64), (E, 3))
    for k in range(K):
        for e in range(E):
            out[k, e, 3:] = tilt_to_quat(u[k, e])
    return out


def rollout_dual_arm(q0, qd0, tray_poses, models, params, steps: int, plant_models=None, metrics_only: bool = False,
                     qdd_prev0=None, metrics0=None, grasp=None, jacdot_point: int = 0, **cfg):
    """``steps`` steps of E dual-arm experiments resident on the device (``dart_dual_arm_rollout``): per step the tray
    pose -> mocap targets, the dynamics of ``models`` (ArmModels or rows, left and right), the impedance QP and one
    step of the plant ``plant_models`` (default: the controller's models; a heavier last link is a payload).

    q0, qd0 [E, 2, n]; tray_poses [steps, E, 7] or [1, E, 7] (held); params: the reference's parameter dict for both
    arms, or a pair (left, right).  ``qdd_prev0`` / ``metrics0`` continue an earlier call.  Returns dict(q, qd,
    qdd_prev, metrics [2 E, 6] (arm.ARM_METRIC_SLOTS), logs (None with ``metrics_only``), wall_s)."""
    import ctypes

    from . import arm as A
    from ._lib import _ptr, lib
    q = np.ascontiguousarray(q0, dtype=np.float64).copy()
    qd = np.ascontiguousarray(qd0, dtype=np.float64).copy()
    if q.ndim != 3 or q.shape[1] != 2 or qd.shape != q.shape:
        raise A.DartMPCError("q0 and qd0 are [E, 2, n]")
    E, _, n = q.shape
    tray = np.ascontiguousarray(tray_poses, dtype=np.float64)
    if tray.ndim != 3 or tray.shape[1:] != (E, 7) or tray.shape[0] not in (1, steps):
        raise A.DartMPCError(f"tray_poses are [{steps} or 1, {E}, 7]")
    rows = A._model_rows(models, n, 2)
    plant = rows if plant_models is None else A._model_rows(plant_models, n, 2)
    pl, pr = params if isinstance(params, (tuple, list)) else (params, params)
    prm = np.ascontiguousarray(np.tile(np.stack([A.pack_params(pl), A.pack_params(pr)]), (E, 1)))
    g = np.ascontiguousarray(A.DACTL_GRASP if grasp is None else grasp, dtype=np.float64)
    qp = np.zeros_like(q) if qdd_prev0 is None else np.ascontiguousarray(qdd_prev0, dtype=np.float64).copy()
    met = np.zeros((2 * E, A.NMETRIC)) if metrics0 is None else np.ascontiguousarray(metrics0, dtype=np.float64).copy()
    B = 2 * E
    logs = None
    if not metrics_only:
        logs = {"q": np.full((steps, B, n), np.nan), "qd": np.full((steps, B, n), np.nan),
                "tau": np.full((steps, B, n), np.nan), "ee_pos": np.full((steps, B, 3), np.nan),
                "loss": np.full((steps, B), np.nan), "status": np.zeros((steps, B), dtype=np.int32)}
    lp = [None] * 6 if logs is None else [_ptr(logs[k]) for k in ("q", "qd", "tau", "ee_pos", "loss", "status")]
    dcfg, qcfg = A.arm_dyn_config(jacdot_point=int(jacdot_point)), A.arm_config(**cfg)
    t0 = time.perf_counter()
    rc = lib().dart_dual_arm_rollout(ctypes.byref(dcfg), ctypes.byref(qcfg), E, n, int(steps), tray.shape[0], _ptr(tray),
                                     _ptr(g), _ptr(rows), _ptr(plant), _ptr(prm), prm.shape[1], _ptr(q), _ptr(qd),
                                     _ptr(qp), _ptr(met), *lp)
    wall = time.perf_counter() - t0
    if rc != 0:
        raise A.DartMPCError(f"dart_dual_arm_rollout failed ({rc})")
    return {"q": q, "qd": qd, "qdd_prev": qp, "metrics": met, "logs": logs, "wall_s": wall}


# ---- the PMPC loop closed through the dual-arm layer (dart_pmpc_stack_rollout) --------------------------------------
def stack_arrays(states0, targets, prm, q0, qd0, models, params, tray_pos, plant_models=None, plant_pvec=None,
                 x_rot0=None, grasp=None, Ts: float = 0.002):
    """The host arrays of a fresh stack run in the names of ``_lib.STACK_ROLLOUT_ARGS`` (without ``work``): inputs and
    the in/out state and metrics (metrics zeros with slot 1 = -1; stack and arm metrics zeros).  Returns
    (arrays, E, n, lm)."""
    from . import arm as A
    from ._lib import loop_metrics
    states0 = np.asarray(states0, float).reshape(-1, 6)
    E = states0.shape[0]
    q = np.ascontiguousarray(q0, dtype=np.float64).copy()
    qd = np.ascontiguousarray(qd0, dtype=np.float64).copy()
    if q.ndim != 3 or q.shape[:2] != (E, 2) or qd.shape != q.shape:
        raise A.DartMPCError(f"q0 and qd0 are [{E}, 2, n]")
    n = q.shape[2]
    rows = A._model_rows(models, n, 2)
    pl, pr = params if isinstance(params, (tuple, list)) else (params, params)
    lm = plant_pvec is not None
    arrays = {
        "target": np.ascontiguousarray(np.asarray(targets, float).reshape(E, 6)),
        "prm": np.ascontiguousarray(np.asarray(prm, float).reshape(E, 6)),
        "x": _cross_plant(states0[:, :4], x_rot0, plant_pvec, Ts, None).x if lm else states0.copy(),
        "tilt": np.zeros((E, 2)), "metrics": loop_metrics(E),
        "grasp": np.ascontiguousarray(A.DACTL_GRASP if grasp is None else grasp, dtype=np.float64),
        "models": rows, "plant_models": rows if plant_models is None else A._model_rows(plant_models, n, 2),
        "arm_prm": np.ascontiguousarray(np.tile(np.stack([A.pack_params(pl), A.pack_params(pr)]), (E, 1))),
        "q": q.reshape(2 * E, n), "qd": qd.reshape(2 * E, n), "qdd_prev": np.zeros((2 * E, n)),
        "arm_metrics": np.zeros((2 * E, A.NMETRIC)),
        "tray_pos": np.ascontiguousarray(np.broadcast_to(np.asarray(tray_pos, dtype=np.float64), (E, 3))),
        "stack_metrics": np.zeros((E, 8)),
    }
    if lm:
        arrays["plant_pvec"] = np.ascontiguousarray(np.asarray(plant_pvec, float).reshape(E, 34))
        arrays["pz_vz"] = np.ascontiguousarray(states0[:, 4:6])
    if arrays["grasp"].shape != (2, 7):
        raise A.DartMPCError("grasp transforms are [2, 7] (pos | quat)")
    return arrays, E, n, lm


def stack_logs(rows, E, n, lm):
    """The three log groups of a stack run, prefilled: (PMPC logs, stack logs, arm logs)."""
    from ._lib import PMPC_LOOP_LOGS, PMPC_LM_LOOP_LOGS, STACK_LOGS, LOG_INT_FILL, loop_logs
    B = 2 * E
    arm = {"q": np.full((rows, B, n), np.nan), "qd": np.full((rows, B, n), np.nan), "tau": np.full((rows, B, n), np.nan),
           "ee_pos": np.full((rows, B, 3), np.nan), "loss": np.full((rows, B), np.nan),
           "status": np.full((rows, B), LOG_INT_FILL, dtype=np.int32)}
    return loop_logs(PMPC_LM_LOOP_LOGS if lm else PMPC_LOOP_LOGS, rows, E), loop_logs(STACK_LOGS, rows, E), arm


def rollout_stack(states0, targets, prm, q0, qd0, models, params, steps: int, tray_pos, couple="achieved",
                  plant_models=None, plant_pvec=None, metrics_only: bool = False, x_rot0=None, settle_steps: int = 0,
                  N: int = 20, Ts: float = 0.002, tol: float = 1e-8, device: int = 0, plant_kw: dict | None = None,
                  grasp=None, jacdot_point: int = 0, **cfg):
    """E PMPC experiments closed through two arms each, resident on the device (``dart_pmpc_stack_rollout``): per step
    the solve, the tray pose commanded by its tilt, both arms' dynamics, impedance QP and plant step, the tray the arms
    then hold, and the object's plant step -- with ``couple="achieved"`` on the achieved tilt (the arms are the lag),
    with ``"ride"`` on the lagged command as in ``rollout_pmpc`` (the arms are measured only).

    states0, targets, prm, ``plant_pvec`` / ``x_rot0`` as ``rollout_pmpc``; q0, qd0 [E, 2, n], models, params,
    ``plant_models`` (a heavier last link is a payload) as ``rollout_dual_arm``; ``tray_pos`` [3] or [E, 3].  The arms
    should start near the grasp pose of a level tray: ``settle_steps`` > 0 first runs ``rollout_dual_arm`` for that many
    steps against the level pose at ``tray_pos`` and starts from where it ends.

    Returns dict(logs: the per-experiment log dicts of ``rollout_pmpc`` (None with ``metrics_only``), status, iters
    [steps, E], metrics [E, 8] (_lib.METRIC_SLOTS), x, tilt (the final state), arm: what ``rollout_dual_arm`` returns,
    stack_metrics [E, 8] (_lib.STACK_METRIC_SLOTS), tilt_log [steps, E, 2], tray_log [steps, E, 7], wall_s)."""
    from . import arm as A
    from ._lib import plant_config, stack_config
    if settle_steps:
        E0 = np.asarray(q0).shape[0]
        level = np.zeros((1, E0, 7))
        level[0, :, :3] = np.broadcast_to(np.asarray(tray_pos, dtype=np.float64), (E0, 3))
        level[0, :, 3] = 1.0
        st = rollout_dual_arm(q0, qd0, level, models, params, int(settle_steps), plant_models=plant_models,
                              metrics_only=True, grasp=grasp, jacdot_point=jacdot_point, **cfg)
        q0, qd0 = st["q"], st["qd"]
    arrays, E, n, lm = stack_arrays(states0, targets, prm, q0, qd0, models, params, tray_pos, plant_models, plant_pvec,
                                    x_rot0, grasp, Ts)
    lg, sl, al = (None, None, None) if metrics_only else stack_logs(steps, E, n, lm)
    solver = Solver(N=N, Ts=Ts, tol=tol, B_max=max(E, 1), device=device)
    try:
        t0 = time.perf_counter()
        solver.stack_rollout(E, n, 0, steps, 0 if metrics_only else steps, arrays["arm_prm"].shape[1], arrays, lg, sl, al,
                             plant=plant_config(**(plant_kw or {})), scfg=stack_config(couple),
                             dcfg=A.arm_dyn_config(jacdot_point=int(jacdot_point)), qcfg=A.arm_config(**cfg), lm=lm)
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    out = {"logs": None, "status": None, "iters": None, "metrics": arrays["metrics"], "x": arrays["x"],
           "tilt": arrays["tilt"], "stack_metrics": arrays["stack_metrics"], "tilt_log": None, "tray_log": None,
           "arm": {"q": arrays["q"].reshape(E, 2, n), "qd": arrays["qd"].reshape(E, 2, n),
                   "qdd_prev": arrays["qdd_prev"].reshape(E, 2, n), "metrics": arrays["arm_metrics"], "logs": al,
                   "wall_s": wall},
           "wall_s": wall}
    if metrics_only:
        return out
    t = np.arange(steps) * Ts
    tg = arrays["target"]
    logs = []
    for b in range(E):
        d = {"t": t, "X": lg["X"][:, b], "X_target": np.tile(tg[b], (steps, 1)), "U_cmd": lg["U_cmd"][:, b],
             "quat_tray": lg["quat_tray"][:, b], "loss": lg["loss"][:, b], "solve_time": np.full(steps, wall / max(steps, 1))}
        for a, side in enumerate("LR"):
            d[side + "_torques"], d[side + "_qpos"] = al["tau"][:, 2 * b + a], al["q"][:, 2 * b + a]
            d[side + "_qvel"], d[side + "_ee_pos"] = al["qd"][:, 2 * b + a], al["ee_pos"][:, 2 * b + a]
            d[side + "_ee_vel"] = np.zeros((steps, 6))      # (not kept by the arm loop)
        d.update(logger_metrics(d, Ts))
        d["metrics"] = arrays["metrics"][b]
        if lm:
            d["rot"] = lg["rot"][:, b]
        logs.append(d)
    out.update(logs=logs, status=lg["status"], iters=lg["iters"], tilt_log=sl["tilt"], tray_log=sl["tray"])
    return out


# ---- the RMPC loop closed through the dual-arm layer (dart_rmpc_stack_rollout) --------------------------------------
def rmpc_stack_arrays(x0, targets, q0, qd0, models, params, tray_pos, mu=0.1, prm=None, plant_models=None,
                      plant_pvec=None, x_rot0=None, grasp=None, N: int = 20, Ts: float = 0.002, P0: float = 1e3):
    """The host arrays of a fresh RMPC stack run in the names of ``_lib.RMPC_STACK_ROLLOUT_ARGS`` (without ``work``):
    inputs, the RMPC loop state of ``RmpcSolver.loop_state`` (``loop_state_lm`` with ``plant_pvec``), the arm state and
    the in/out metrics (metrics zeros with slot 1 = -1; stack and arm metrics zeros).  x0, targets [E, 4]; q0, qd0
    [E, 2, n]; ``prm`` [E, 10] (default: rob_ctrl.py's parameter row).  Returns (arrays, E, n, lm)."""
    from . import arm as A
    from ._lib import RMPC_LOOP_STATE, RMPC_LM_LOOP_STATE, _loop_shape, lib, loop_metrics
    x0 = np.asarray(x0, float).reshape(-1, 4)
    E = x0.shape[0]
    q = np.ascontiguousarray(q0, dtype=np.float64).copy()
    qd = np.ascontiguousarray(qd0, dtype=np.float64).copy()
    if q.ndim != 3 or q.shape[:2] != (E, 2) or qd.shape != q.shape:
        raise A.DartMPCError(f"q0 and qd0 are [{E}, 2, n]")
    n = q.shape[2]
    rows = A._model_rows(models, n, 2)
    pl, pr = params if isinstance(params, (tuple, list)) else (params, params)
    lm = plant_pvec is not None
    if prm is None:
        ctl = AdaptiveNPMPCSmooth(None, None, Ts=Ts, N=N, Qp=80.0, Qv=2.0, Ru=0.02, Rdu=1.0, u_bounds=(-0.6, 0.6),
                                  du_bounds=(-0.06, 0.06), vmax=0.2, v_eps=0.1)          # rob_ctrl.py:280-283
        prm = np.tile(ctl.params(), (E, 1))
    nw = lib().dart_rmpc_nw(int(N))
    arrays = {name: np.zeros(_loop_shape(E, width, nw=nw), dt) for name, width, dt in (RMPC_LM_LOOP_STATE if lm else RMPC_LOOP_STATE)}
    arrays["x"][:, :4] = x0
    if lm and x_rot0 is not None:
        arrays["x"][:, 4:] = np.asarray(x_rot0, float).reshape(E, 4)
    arrays["prev"][:] = x0
    arrays["P"][:] = np.tile(np.eye(7) * float(P0), (2, 1, 1)).reshape(98)
    arrays.update({
        "target": np.ascontiguousarray(np.asarray(targets, float).reshape(E, 4)),
        "prm": np.ascontiguousarray(np.asarray(prm, float).reshape(E, 10)),
        "metrics": loop_metrics(E),
        "grasp": np.ascontiguousarray(A.DACTL_GRASP if grasp is None else grasp, dtype=np.float64),
        "models": rows, "plant_models": rows if plant_models is None else A._model_rows(plant_models, n, 2),
        "arm_prm": np.ascontiguousarray(np.tile(np.stack([A.pack_params(pl), A.pack_params(pr)]), (E, 1))),
        "q": q.reshape(2 * E, n), "qd": qd.reshape(2 * E, n), "qdd_prev": np.zeros((2 * E, n)),
        "arm_metrics": np.zeros((2 * E, A.NMETRIC)),
        "tray_pos": np.ascontiguousarray(np.broadcast_to(np.asarray(tray_pos, dtype=np.float64), (E, 3))),
        "stack_metrics": np.zeros((E, 8)),
    })
    if lm:
        arrays["plant_pvec"] = np.ascontiguousarray(np.asarray(plant_pvec, float).reshape(E, 34))
    else:
        arrays["mu"] = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, np.float64), (E,)))
    if arrays["grasp"].shape != (2, 7):
        raise A.DartMPCError("grasp transforms are [2, 7] (pos | quat)")
    return arrays, E, n, lm


def rmpc_stack_logs(rows, E, n, lm):
    """The three log groups of an RMPC stack run, prefilled: (RMPC logs, stack logs, arm logs)."""
    from ._lib import RMPC_LOOP_LOGS, RMPC_LM_LOOP_LOGS, RMPC_STACK_LOGS, loop_logs
    return (loop_logs(RMPC_LM_LOOP_LOGS if lm else RMPC_LOOP_LOGS, rows, E), loop_logs(RMPC_STACK_LOGS, rows, E),
            stack_logs(rows, E, n, lm)[2])


def rollout_stack_rmpc(x0, targets, q0, qd0, models, params, steps: int, tray_pos, couple="achieved", mu=0.1, prm=None,
                       plant_models=None, plant_pvec=None, x_rot0=None, metrics_only: bool = False,
                       settle_steps: int = 0, check_every: int = 0, N: int = 20, Ts: float = 0.002, device: int = 0,
                       pos_tol: float = ERROR_THRESHOLD, plant_kw: dict | None = None, dr_max: float = 0.01,
                       alpha_rg: float = 0.5, lam: float = 0.995, P0: float = 1e3, grasp=None, jacdot_point: int = 0,
                       **cfg):
    """E RMPC experiments closed through two arms each, resident on the device (``dart_rmpc_stack_rollout``;
    rob_ctrl.py:331-416): per step the RLS update fused into the warm-started solve, the tray pose commanded by its tilt,
    both arms' dynamics, impedance QP and plant step, the tray the arms then hold, and the object's plant step -- with
    ``couple="achieved"`` on the achieved tilt, with ``"ride"`` on the lagged command as in ``rollout_rmpc`` (the arms are
    measured only) -- then the governor and the staged reference of the next solve.

    x0, targets, ``mu``, ``prm``, ``plant_pvec`` / ``x_rot0``, ``check_every`` and the loop's keywords as
    ``rollout_rmpc``; q0, qd0, models, params, ``plant_models``, ``tray_pos``, ``settle_steps`` as ``rollout_stack``.
    ``check_every`` > 0 runs chunks of that many steps and stops once every episode has closed; state and metrics are
    in/out, so the chunks are the bits of one call.

    Returns dict(episodes, status [steps run, E], done, extra: what ``rollout_rmpc(..., return_logs=True)`` returns, each
    episode row's ``torque`` being the 2 n torques [L | R] the arms applied in that step (the reference's torques_log);
    metrics [E, 8], stack_metrics [E, 8], arm: what ``rollout_dual_arm`` returns, tilt_log, tray_log, U_log
    [steps run, E, .], steps, wall_s).  ``metrics_only``: no log is written or moved; episodes, status, extra and the
    three logs are None."""
    from . import arm as A
    from ._lib import plant_config, rmpc_loop_config, stack_config
    if settle_steps:
        E0 = np.asarray(q0).shape[0]
        level = np.zeros((1, E0, 7))
        level[0, :, :3] = np.broadcast_to(np.asarray(tray_pos, dtype=np.float64), (E0, 3))
        level[0, :, 3] = 1.0
        st = rollout_dual_arm(q0, qd0, level, models, params, int(settle_steps), plant_models=plant_models,
                              metrics_only=True, grasp=grasp, jacdot_point=jacdot_point, **cfg)
        q0, qd0 = st["q"], st["qd"]
    arrays, E, n, lm = rmpc_stack_arrays(x0, targets, q0, qd0, models, params, tray_pos, mu, prm, plant_models, plant_pvec,
                                         x_rot0, grasp, N, Ts, P0)
    lg, sl, al = (None, None, None) if metrics_only else rmpc_stack_logs(steps, E, n, lm)
    loop = rmpc_loop_config(dr_max=dr_max, alpha_rg=alpha_rg, rls_lambda=lam, pos_tol=pos_tol)
    solver = RmpcSolver(N=N, Ts=Ts, B_max=max(E, 1), device=device)
    chunk = int(check_every) if check_every and check_every > 0 else max(steps, 1)
    k = 0
    try:
        t0 = time.perf_counter()
        while k < steps:
            m = min(chunk, steps - k)
            solver.rmpc_stack_rollout(E, n, k, m, 0 if metrics_only else steps, arrays["arm_prm"].shape[1], arrays, lg, sl,
                                      al, plant=plant_config(**(plant_kw or {})), loop=loop, scfg=stack_config(couple),
                                      dcfg=A.arm_dyn_config(jacdot_point=int(jacdot_point)), qcfg=A.arm_config(**cfg), lm=lm)
            k += m
            if arrays["done"].all():
                break
        wall = time.perf_counter() - t0
    finally:
        solver.close()
    out = {"episodes": None, "status": None, "done": arrays["done"].astype(bool), "extra": None,
           "metrics": arrays["metrics"], "stack_metrics": arrays["stack_metrics"],
           "arm": {"q": arrays["q"].reshape(E, 2, n), "qd": arrays["qd"].reshape(E, 2, n),
                   "qdd_prev": arrays["qdd_prev"].reshape(E, 2, n), "metrics": arrays["arm_metrics"],
                   "logs": None if al is None else {name: a[:k] for name, a in al.items()}, "wall_s": wall},
           "tilt_log": None, "tray_log": None, "U_log": None, "steps": k, "wall_s": wall}
    if metrics_only:
        return out
    episodes = []
    for b in range(E):
        nl = min(int(arrays["nlog"][b]), steps)
        # a fresh run's open episode logs one row per step from step 0: row j's torques are step j's tau
        eps = {}
        add_episode(eps, "ep1", lg["pos_err"][:nl, b].tolist(), lg["pos_err_norm"][:nl, b].tolist(),
                    list(lg["u_cmd"][:nl, b]), [al["tau"][j, 2 * b:2 * b + 2].reshape(2 * n).copy() for j in range(nl)],
                    lg["timestep"][:nl, b].tolist())
        eps["metrics"] = arrays["metrics"][b]
        if lm:
            eps["rot"] = lg["rot"][:k, b]
        episodes.append(eps)
    state = {name: arrays[name] for name in ("x", "tilt", "prev", "u_prev", "r_v", "theta", "P", "w", "done", "nlog",
                                             "metrics")}
    extra = {name: lg[name][:k] for name in ("x", "theta", "r_v", "f", "status", "iters")}
    extra.update(state=state, solve_time=wall / max(k, 1),
                 episode_rows={name: lg[name] for name in ("pos_err", "pos_err_norm", "u_cmd", "timestep")})
    out.update(episodes=episodes, status=lg["status"][:k], extra=extra, tilt_log=sl["tilt"][:k], tray_log=sl["tray"][:k],
               U_log=sl["U_cmd"][:k])
    return out
