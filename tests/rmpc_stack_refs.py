"""CPU reference for the RMPC loop through the dual-arm layer (csrc/rmpc_stack_step.hip) -- TEST INFRASTRUCTURE ONLY,
numpy, never imported by the product.  One couple + object launch (post / pre): the RMPC glue of ``harness.run_rmpc``
(episode rows, done, the step rows, RLS features / targets, governor, staged reference), the coupling and the stack
metrics of ``stack_refs``, ``harness.rollout_metrics``, and ``harness.TrayPlant`` / ``harness.LmpcPlant``.
"""
from __future__ import annotations

import numpy as np

import stack_refs as S
from arm_dyn_refs import DACTL_GRASP
from dart_mpc import harness
from dart_mpc.pmpc import tilt_to_quat
from dart_mpc.rmpc import AdaptiveNPMPCSmooth, rls_features

RIDE, ACHIEVED = S.RIDE, S.ACHIEVED


def _plant_step(lm, Ts, x, tilt, up, plant):
    """(next x, next tilt) of the object plant with the tilt state ``tilt`` driven by ``up``; ``plant``: mu [E] (tray
    plant) or pvec [E, 34] (LMPC plant, stepped with the flipped command as ``harness.run_rmpc`` does)."""
    if lm:
        p = harness.LmpcPlant(x, plant, dt=Ts)
        p.tilt = -tilt
        xn = p.step(-up)
        return xn, -p.tilt
    p = harness.TrayPlant(x, plant, dt=Ts)
    p.tilt = tilt.copy()
    xn = p.step(up)
    return xn, p.tilt


def rmpc_stack_step(lm, couple, N, k, do_post, do_pre, Ts, cfg, state, target, prm, plant, io, logs, stack_logs, tray_pos,
                    ee_pos, ee_quat, grasp=DACTL_GRASP):
    """One launch of rmpc_stack_step_kernel<lm> for E experiments.  ``state``: x [E, 6 | 8], tilt, prev, u_prev, r_v,
    theta, done, nlog, metrics, stack_metrics; ``io``: the solve's per-step arrays (RMPC_LOOP_IO); ``logs`` /
    ``stack_logs``: the RMPC and the stack log groups [rows, E, .] or None; ``cfg``: the loop config (dr_max, alpha_rg,
    step_fraction, pos_tol).  Returns copies (state, io, logs, stack_logs)."""
    s = {n: np.array(v) for n, v in state.items()}
    io = {n: np.array(v) for n, v in io.items()}
    lg = None if logs is None else {n: v.copy() for n, v in logs.items()}
    sl = None if stack_logs is None else {n: v.copy() for n, v in stack_logs.items()}
    E = s["x"].shape[0]
    if do_post:
        xk, u = s["x"][:, :4].copy(), io["u0"]
        rot = s["x"][:, 4:] if lm else np.zeros((E, 4))
        en = np.linalg.norm(xk[:, [0, 2]] - target[:, [0, 2]], axis=1)
        for b in np.where(s["done"] == 0)[0]:
            r = s["nlog"][b]
            if lg is not None and 0 <= r < lg["pos_err"].shape[0]:
                lg["pos_err"][r, b] = [target[b, 0] - xk[b, 0], target[b, 2] - xk[b, 2]]
                lg["pos_err_norm"][r, b] = float(en[b])
                lg["u_cmd"][r, b] = u[b]
                lg["timestep"][r, b] = k * Ts
            s["nlog"][b] += 1
            if en[b] < cfg.pos_tol:
                s["done"][b] = 1
        if lg is not None:
            lg["x"][k], lg["theta"][k], lg["r_v"][k] = xk, s["theta"], s["r_v"]
            lg["f"][k], lg["status"][k], lg["iters"][k] = io["f"], io["status"], io["iters"]
            if lm:
                lg["rot"][k] = rot
        s["metrics"] = harness.rollout_metrics(xk[None], target, u[None], io["status"][None], io["iters"][None], rot[None],
                                               Ts, metrics=s["metrics"], k0=k)
        meas = S.tray_from_arms_batch(np.asarray(ee_pos).reshape(E, 2, 3), np.asarray(ee_quat).reshape(E, 2, 4), grasp)
        held = S.stack_metrics_step(s["stack_metrics"], meas, u, np.asarray(tray_pos, dtype=float))
        if sl is not None:
            sl["U_cmd"][k], sl["quat_tray"][k] = u, np.stack([tilt_to_quat(v) for v in u])
            sl["tilt"][k], sl["tray"][k] = meas["tilt"], meas["tray"]
        s["prev"], s["u_prev"] = xk, u.copy()
        tilt, up = s["tilt"], u
        if couple == ACHIEVED:
            tilt = np.where(held[:, None], tilt, meas["tilt"])
            up = tilt.copy()
        s["x"], s["tilt"] = _plant_step(lm, Ts, s["x"], tilt, up, plant)
    if do_pre:
        xk, prev = s["x"][:, :4].copy(), s["prev"]
        io["y"] = (xk[:, [1, 3]] - prev[:, [1, 3]]) / Ts
        io["phi"] = np.stack([rls_features(p, prm[b, 9]) for b, p in enumerate(prev)])
        err = np.stack([target[:, 0] - s["r_v"][:, 0], np.zeros(E), target[:, 2] - s["r_v"][:, 2], np.zeros(E)], axis=1)
        s["r_v"] = s["r_v"] + cfg.alpha_rg * np.clip(err, -cfg.dr_max, cfg.dr_max) * np.array([1.0, 0.0, 1.0, 0.0])
        io["Rref"] = np.stack([AdaptiveNPMPCSmooth.build_ref_traj(xk[b], s["r_v"][b], target[b], N, 4,
                                                                  step_fraction=cfg.step_fraction) for b in range(E)])
        io["x0"] = xk
    return s, io, lg, sl
