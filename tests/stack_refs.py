"""CPU references for the PMPC loop through the dual-arm layer (csrc/stack_step.hip) -- TEST INFRASTRUCTURE ONLY, numpy,
never imported by the product.  The coupling (the tray two arms hold), the command pose, and one couple + object step
(post / pre) on ``harness.TrayPlant`` / ``harness.LmpcPlant`` with ``harness.rollout_metrics``; quaternion algebra from
``arm_dyn_refs``, the command quaternion ``pmpc.tilt_to_quat``.
"""
from __future__ import annotations

import numpy as np

from arm_dyn_refs import DACTL_GRASP, qmat, qmul
from dart_mpc import harness
from dart_mpc.pmpc import tilt_to_quat

RIDE, ACHIEVED = 0, 1


def _conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def _unit(q):
    return q / np.sqrt(q @ q)


def tray_from_arms(ee_pos, ee_quat, grasp=DACTL_GRASP):
    """ee_pos [2, 3], ee_quat [2, 4] (left, right) -> dict(tray [7], tilt [2], yaw, gap, angle)."""
    ee_pos, ee_quat, grasp = (np.asarray(a, dtype=float) for a in (ee_pos, ee_quat, grasp))
    with np.errstate(all="ignore"):
        qL = _unit(qmul(ee_quat[0], _conj(grasp[0, 3:])))
        qR = _unit(qmul(ee_quat[1], _conj(grasp[1, 3:])))
        if qL @ qR < 0.0:
            qR = -qR
        qt = _unit(qL + qR)
        if qt[0] < 0.0:
            qt = -qt
        w, x, y, z = qt
        if np.all(np.isfinite(qt)):
            R = qmat(qt)
            p = 0.5 * ((ee_pos[0] - R @ grasp[0, :3]) + (ee_pos[1] - R @ grasp[1, :3]))
        else:
            p = np.full(3, np.nan)
        roll = np.arctan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y))
        sp = 2.0 * (w * y - z * x)
        pitch = np.arcsin(1.0 if sp > 1.0 else -1.0 if sp < -1.0 else sp)
        yaw = np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
        gap = abs(np.linalg.norm(ee_pos[1] - ee_pos[0]) - np.linalg.norm(grasp[1, :3] - grasp[0, :3]))
        d = qmul(qL, _conj(qR))
        angle = 2.0 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0]))
    return {"tray": np.concatenate([p, qt]), "tilt": np.array([-pitch, roll]), "yaw": float(yaw), "gap": float(gap),
            "angle": float(angle)}


def tray_from_arms_batch(ee_pos, ee_quat, grasp=DACTL_GRASP):
    """ee_pos [E, 2, 3], ee_quat [E, 2, 4] -> dict of stacked fields."""
    outs = [tray_from_arms(p, q, grasp) for p, q in zip(np.asarray(ee_pos), np.asarray(ee_quat))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("tray", "tilt", "yaw", "gap", "angle")}


def command_pose(u0, tray_pos):
    """[E, 7] (pos | quat wxyz) from u0 [E, 2] and tray_pos [E, 3]."""
    u0 = np.asarray(u0, dtype=float)
    return np.concatenate([np.asarray(tray_pos, dtype=float), np.stack([tilt_to_quat(u) for u in u0])], axis=1)


def stack_metrics_step(sm, meas, u0, tray_pos):
    """One step of the stack metrics, sm [E, 8] in place: meas from ``tray_from_arms_batch``.  Returns held [E]."""
    E = sm.shape[0]
    held = ~np.all(np.isfinite(meas["tilt"]), axis=1)
    with np.errstate(all="ignore"):
        for e in range(E):
            s = sm[e]
            d0, d1 = abs(meas["tilt"][e, 0] - u0[e, 0]), abs(meas["tilt"][e, 1] - u0[e, 1])
            dev = d0 if d0 > d1 else d1
            pe = np.linalg.norm(meas["tray"][e, :3] - tray_pos[e])
            if not held[e]:
                s[0] = dev
                if dev > s[1]:
                    s[1] = dev
            for slot, v in ((2, abs(meas["yaw"][e])), (3, meas["gap"][e]), (4, meas["angle"][e]), (5, pe)):
                if v > s[slot]:
                    s[slot] = v
            if held[e]:
                s[6] += 1.0
            s[7] += 1.0
    return held


def stack_step(lm, couple, k, do_post, do_pre, Ts, target, prm, tray_pos, ee_pos, ee_quat, x, tilt, metrics, stack_metrics,
               u0, f, status, iters, plant_pvec=None, pz_vz=None, grasp=DACTL_GRASP, plant_kw=None, gravity=-9.81):
    """One couple + object launch (stack_step_kernel<lm>): post(k) and / or pre, for E experiments.  x [E, 6] (tray
    plant) or [E, 8] (LMPC plant); returns dict(x, tilt, metrics, stack_metrics, x0 (pre), and post's log rows X, U_cmd,
    quat_tray, loss, status, iters, rot (lm), tilt_log, tray_log)."""
    x, tilt = np.array(x, dtype=float), np.array(tilt, dtype=float)
    metrics, sm = np.array(metrics, dtype=float), np.array(stack_metrics, dtype=float)
    E = x.shape[0]
    out = {}
    pzvz = np.asarray(pz_vz, dtype=float) if lm else x[:, 4:6].copy()
    if do_post:
        u0 = np.asarray(u0, dtype=float)
        X = np.concatenate([x[:, :4], pzvz], axis=1)
        rot = x[:, 4:] if lm else np.zeros((E, 4))
        metrics = harness.rollout_metrics(X[None], target, u0[None], np.asarray(status)[None], np.asarray(iters)[None],
                                          rot[None], Ts, metrics=metrics, k0=k)
        meas = tray_from_arms_batch(np.asarray(ee_pos).reshape(E, 2, 3), np.asarray(ee_quat).reshape(E, 2, 4), grasp)
        held = stack_metrics_step(sm, meas, u0, np.asarray(tray_pos, dtype=float))
        out.update(X=X, U_cmd=u0.copy(), quat_tray=np.stack([tilt_to_quat(u) for u in u0]), loss=np.asarray(f, dtype=float),
                   status=np.asarray(status), iters=np.asarray(iters), tilt_log=meas["tilt"], tray_log=meas["tray"])
        if lm:
            out["rot"] = x[:, 4:].copy()
        if couple == ACHIEVED:
            tilt = np.where(held[:, None], tilt, meas["tilt"])
            up = tilt.copy()
        else:
            up = u0
        kw = dict(plant_kw or {})
        if lm:
            plant = harness.LmpcPlant(x, plant_pvec, dt=Ts, **{k_: v for k_, v in kw.items() if k_ == "tau"})
            plant.tilt = -tilt
            plant.step(-up)
            x, tilt = plant.x, -plant.tilt
        else:
            plant = harness.TrayPlant(x, np.asarray(prm)[:, 0], dt=Ts, g=gravity, **kw)
            plant.tilt = tilt.copy()
            plant.step(up)
            x, tilt = plant.x, plant.tilt
    if do_pre:
        out["x0"] = np.concatenate([x[:, :4], pzvz], axis=1)
    out.update(x=x, tilt=tilt, metrics=metrics, stack_metrics=sm)
    return out
