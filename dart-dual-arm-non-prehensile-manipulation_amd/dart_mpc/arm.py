"""Drop-in per-arm impedance controller backed by the MI355X arm-QP kernel.

Mirrors ARMCONTROL (PMPC/src/controller/arm.py; the same class lives in
RMPC/dev_dual/controller/parallel.py and LMPC/src/controller/parallel.py):

  - ``ArmSolver``: the batched C ABI ``dart_arm_solve_batch(_dev)`` -- the body of
    ``ARMCONTROL.solver_worker`` (:266-457) for B arm snapshots per launch.
  - ``ArmControl``: ``ARMCONTROL.compute_torque`` (:201-231) with the solver run in-process:
    feed it the dict ``compute_dynamics`` (:111-199) returns, get ``(torque_cmd, loss)``; the
    solution is kept as the next ``qdd_prev`` exactly as the worker writes ``views["qdd_prev"]``
    (:431).  The dynamics dict is an input here; ``ArmDynamics`` makes it on the device from the joint state.
  - ``ArmDynamics``: ``compute_dynamics`` (:111-199) without MuJoCo -- ``dart_arm_dynamics_batch(_dev)`` from a model
    row (``dart_mpc.arm_model.ArmModel``) and (q, qd); ``control_batch`` runs dynamics and QP in one call.
  - ``DualArmControl``: ``DACTL.control`` (PMPC/src/dualctl.py:22-66), tray pose -> both arms' torques.

Snapshot / parameter row layouts are those of include/dart_mpc.h (``pack_snapshot``,
``pack_params``).  The kernel cold-starts the bound multipliers and warm-starts qdd from
qdd_prev; the QP is strictly convex, so the answer does not depend on the reference's IPOPT
warm-start duals (:401-417).

Non-finite input: a NaN or inf in a snapshot or in the parameter row (a NaN bound aside, which is an absent bound)
returns ``BREAKDOWN`` (-2) with ``iters`` 0 and a NaN ``loss``, never a status >= 0; ``qdd`` and ``tau`` are then not
meaningful (``ArmControl`` keeps them as they come: check ``last_status``).  The reference worker would raise in ``np.linalg.pinv`` on such a snapshot.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import DartMPCError, _ptr, lib

SOLVED, ACCEPTABLE, MAXITER, BREAKDOWN, INFEASIBLE = 0, 1, -1, -2, -3
SNAP_FIELDS = (("q", "n"), ("qd", "n"), ("qdd_prev", "n"), ("mocap_pos", 3), ("ee_pos", 3), ("rotvec", 3),
               ("jac", "6n"), ("jacDot", "6n"), ("M", "nn"), ("h", "n"), ("Mx_inv", 36))
PARAM_FIELDS = (("Wimp", 36), ("Wpos", "nn"), ("Wsmooth", "nn"), ("Qmin", "n"), ("Qmax", "n"), ("Qdotmin", "n"),
                ("Qdotmax", "n"), ("taumin", "n"), ("taumax", "n"), ("K", 36), ("K_null", "nn"), ("dt", 1))


class ArmConfig(ctypes.Structure):
    """Mirror of ``struct dart_arm_config``."""
    _fields_ = [("tol", ctypes.c_double), ("acceptable_tol", ctypes.c_double), ("max_iter", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def _width(w, n):
    return {"n": n, "6n": 6 * n, "nn": n * n}.get(w, w)


def pack_snapshot(snaps: dict) -> np.ndarray:
    """[B, snapshot_len] rows from a dict of [B, ...] arrays (or one snapshot of unbatched arrays)."""
    one = np.ndim(snaps["q"]) == 1
    n = np.shape(snaps["q"])[-1]
    cols = [np.reshape(np.asarray(snaps[k], dtype=np.float64), (1 if one else -1, _width(w, n)))
            for k, w in SNAP_FIELDS]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def pack_params(prm: dict) -> np.ndarray:
    """One parameter row (dict of arrays, the reference's params) or [B, param_len] when batched."""
    n = np.shape(prm["Qmin"])[-1]
    batched = np.ndim(prm["Qmin"]) == 2
    cols = []
    for k, w in PARAM_FIELDS:
        v = np.asarray(prm[k], dtype=np.float64)
        cols.append(np.reshape(v, (-1 if batched else 1, _width(w, n))))
    out = np.concatenate(cols, axis=1)
    return np.ascontiguousarray(out if batched else out[0])


def arm_config(**over) -> ArmConfig:
    c = ArmConfig()
    lib().dart_arm_config_default(ctypes.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


class ArmSolver:
    """Batched ``dart_arm_solve_batch``: B arm QPs per call (n joints, one shared or per-instance
    parameter row)."""

    def __init__(self, n: int = 7, **cfg):
        self.n = int(n)
        self.cfg = arm_config(**cfg)
        L = lib()
        self.snap_len = L.dart_arm_snapshot_len(self.n)
        self.param_len = L.dart_arm_param_len(self.n)
        if self.snap_len < 0:
            raise DartMPCError(f"unsupported joint count n={n}")

    def solve_batch(self, snap_rows: np.ndarray, prm_rows: np.ndarray):
        """Host arrays: snap_rows [B, snapshot_len], prm_rows [param_len] (shared) or [B, param_len]."""
        snap_rows = np.ascontiguousarray(snap_rows, dtype=np.float64)
        prm_rows = np.ascontiguousarray(prm_rows, dtype=np.float64)
        B = snap_rows.shape[0]
        if snap_rows.shape[1] != self.snap_len:
            raise DartMPCError(f"snapshot rows must have {self.snap_len} entries")
        stride = 0 if prm_rows.ndim == 1 else self.param_len
        if prm_rows.shape[-1] != self.param_len or (stride and prm_rows.shape[0] != B):
            raise DartMPCError(f"parameter rows must have {self.param_len} entries")
        out = {"qdd": np.zeros((B, self.n)), "tau": np.zeros((B, self.n)), "loss": np.zeros(B),
               "status": np.zeros(B, dtype=np.int32), "iters": np.zeros(B, dtype=np.int32)}
        rc = lib().dart_arm_solve_batch(ctypes.byref(self.cfg), B, self.n, _ptr(snap_rows), _ptr(prm_rows), stride,
                                        _ptr(out["qdd"]), _ptr(out["tau"]), _ptr(out["loss"]), _ptr(out["status"]),
                                        _ptr(out["iters"]))
        if rc != 0:
            raise DartMPCError(f"dart_arm_solve_batch failed ({rc})")
        return out

    def solve_batch_dev(self, B, snap_ptr, prm_ptr, prm_shared, qdd_ptr, tau_ptr, loss_ptr, status_ptr, iters_ptr,
                        stream=None):
        """Device pointers (ints), asynchronous on ``stream`` (a hipStream_t as int, None = default)."""
        rc = lib().dart_arm_solve_batch_dev(ctypes.byref(self.cfg), B, self.n, ctypes.c_void_p(snap_ptr),
                                            ctypes.c_void_p(prm_ptr), 0 if prm_shared else self.param_len,
                                            ctypes.c_void_p(qdd_ptr), ctypes.c_void_p(tau_ptr),
                                            ctypes.c_void_p(loss_ptr), ctypes.c_void_p(status_ptr),
                                            ctypes.c_void_p(iters_ptr), ctypes.c_void_p(stream or 0))
        if rc != 0:
            raise DartMPCError(f"dart_arm_solve_batch_dev failed ({rc})")


class ArmControl:
    """ARMCONTROL.compute_torque with the solve in-process on the GPU.

    ``params`` is the reference's parameter dict (Wimp, Wpos, Wsmooth, Qmin, Qmax, Qdotmin, Qdotmax,
    taumin, taumax, K, K_null, dt; joint/actuator/body names are MuJoCo bindings and not needed).
    """

    def __init__(self, params: dict, n: int = 7):
        self.params = params
        self.solver = ArmSolver(n)
        self.prm_row = pack_params(params)
        self.qdd_prev = np.zeros(n)          # views["qdd_prev"], zero-initialised (arm.py:95)
        self.last_status = None

    def compute_torque(self, dynamics: dict):
        """dynamics: the dict of compute_dynamics (arm.py:185-199); qdd_prev is taken from this
        controller (the worker's own last solution) unless the dict carries one."""
        snap = dict(dynamics)
        snap.setdefault("qdd_prev", self.qdd_prev)
        out = self.solver.solve_batch(pack_snapshot(snap), self.prm_row)
        self.last_status = int(out["status"][0])
        self.qdd_prev = out["qdd"][0].copy()
        return out["tau"][0].copy(), float(out["loss"][0])

    def compute_torque_from_state(self, dynamics: "ArmDynamics", q, qd, mocap_pos, mocap_quat):
        """compute_dynamics + compute_torque from the joint state alone: the snapshot is taken on the device
        (``dart_arm_control_batch``), no MuJoCo.  Keeps qdd_prev as ``compute_torque`` does."""
        out = dynamics.control_batch(dynamics.pack_state(q, qd, self.qdd_prev, mocap_pos, mocap_quat), self.prm_row,
                                     cfg=self.solver.cfg)
        self.last_status = int(out["status"][0])
        self.qdd_prev = out["qdd"][0].copy()
        return out["tau"][0].copy(), float(out["loss"][0])


# ---- arm dynamics on the device (dart_arm_dynamics_batch and the entries built on it) -----------------------------
JACDOT_REFERENCE, JACDOT_BODY = 0, 1
NMETRIC = 6
ARM_METRIC_SLOTS = ("final_pos_error", "max_pos_error", "final_rot_error", "status_nonzero", "iters", "max_tau_ratio")
# the grasp transforms of DACTL._resolve_ee_pos (dualctl.py:32-33): (pos | quat wxyz) in the tray frame, left then right
DACTL_GRASP = np.array([[-0.175, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5], [0.175, 0.0, 0.0, 0.5, -0.5, -0.5, 0.5]])


class ArmDynConfig(ctypes.Structure):
    """Mirror of ``struct dart_arm_dyn_config``."""
    _fields_ = [("jacdot_point", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


def arm_dyn_config(**over) -> ArmDynConfig:
    c = ArmDynConfig()
    lib().dart_arm_dyn_config_default(ctypes.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _model_rows(model, n, count=None):
    """Model rows as a contiguous array: one ArmModel / row (shared) or a sequence of them ([count, model_len])."""
    def one(m):
        return m.row() if hasattr(m, "row") else np.asarray(m, dtype=np.float64)
    rows = np.stack([one(m) for m in model]) if isinstance(model, (list, tuple)) else one(model)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    ML = lib().dart_arm_model_len(n)
    if rows.shape[-1] != ML or (count is not None and rows.shape != (count, ML)):
        raise DartMPCError(f"model rows of {n} joints have {ML} entries" + (f" ({count} rows)" if count else ""))
    return rows


def _check(rc, what):
    if rc != 0:
        raise DartMPCError(f"{what} failed ({rc})")


class ArmDynamics:
    """``ARMCONTROL.compute_dynamics`` on the device: joint state -> the snapshot the QP reads.

    ``model``: an ``ArmModel`` (or its row), shared by the batch, or one per instance."""

    def __init__(self, model, n: int = None, jacdot_point: int = JACDOT_REFERENCE):
        self.n = int(n if n is not None else model.n)
        L = lib()
        self.state_len, self.snap_len = L.dart_arm_state_len(self.n), L.dart_arm_snapshot_len(self.n)
        if self.state_len < 0:
            raise DartMPCError(f"unsupported joint count n={n}")
        self.model_len = L.dart_arm_model_len(self.n)
        self.rows = _model_rows(model, self.n)
        self.cfg = arm_dyn_config(jacdot_point=int(jacdot_point))

    def pack_state(self, q, qd, qdd_prev, mocap_pos, mocap_quat) -> np.ndarray:
        """[B, state_len] rows from [B, .] arrays (or one state of unbatched arrays)."""
        cols = [np.reshape(np.asarray(v, dtype=np.float64), (-1 if np.ndim(q) == 2 else 1, w))
                for v, w in ((q, self.n), (qd, self.n), (qdd_prev, self.n), (mocap_pos, 3), (mocap_quat, 4))]
        return np.ascontiguousarray(np.concatenate(cols, axis=1))

    def _stride(self, B):
        if self.rows.ndim == 2 and self.rows.shape[0] != B:
            raise DartMPCError(f"{self.rows.shape[0]} model rows for {B} instances")
        return 0 if self.rows.ndim == 1 else self.model_len

    def dynamics_batch(self, state_rows, want_ee_quat=False):
        """state_rows [B, state_len] -> snapshot rows [B, snapshot_len] (and ee_quat [B, 4])."""
        state_rows = np.ascontiguousarray(state_rows, dtype=np.float64)
        B = state_rows.shape[0]
        if state_rows.ndim != 2 or state_rows.shape[1] != self.state_len:
            raise DartMPCError(f"state rows must have {self.state_len} entries")
        snap = np.zeros((B, self.snap_len))
        eq = np.zeros((B, 4)) if want_ee_quat else None
        _check(lib().dart_arm_dynamics_batch(ctypes.byref(self.cfg), B, self.n, _ptr(self.rows), self._stride(B),
                                             _ptr(state_rows), _ptr(snap), _ptr(eq)), "dart_arm_dynamics_batch")
        return (snap, eq) if want_ee_quat else snap

    def dynamics_batch_dev(self, B, model_ptr, model_shared, state_ptr, snap_ptr, ee_quat_ptr=None, stream=None):
        """Device pointers (ints), asynchronous on ``stream``."""
        _check(lib().dart_arm_dynamics_batch_dev(ctypes.byref(self.cfg), B, self.n, ctypes.c_void_p(model_ptr),
                                                 0 if model_shared else self.model_len, ctypes.c_void_p(state_ptr),
                                                 ctypes.c_void_p(snap_ptr), ctypes.c_void_p(ee_quat_ptr or 0),
                                                 ctypes.c_void_p(stream or 0)), "dart_arm_dynamics_batch_dev")

    def snapshot(self, q, qd, qdd_prev, mocap_pos, mocap_quat) -> dict:
        """The dict ``pack_snapshot`` takes (arm.py:185-199 without the MuJoCo calls), plus ``ee_quat`` and
        ``mocap_quat``; batched when q is [B, n]."""
        one = np.ndim(q) == 1
        rows, eq = self.dynamics_batch(self.pack_state(q, qd, qdd_prev, mocap_pos, mocap_quat), want_ee_quat=True)
        out = unpack_snapshot(rows, self.n)
        out["ee_quat"], out["mocap_quat"] = eq, np.reshape(np.asarray(mocap_quat, dtype=np.float64), (-1, 4))
        return {k: v[0] for k, v in out.items()} if one else out

    def control_batch(self, state_rows, prm_rows, cfg=None, want_snap=False):
        """Dynamics, then the QP, in one call: dict(qdd, tau, loss, status, iters[, snap])."""
        state_rows = np.ascontiguousarray(state_rows, dtype=np.float64)
        prm_rows = np.ascontiguousarray(prm_rows, dtype=np.float64)
        B, n = state_rows.shape[0], self.n
        PL = lib().dart_arm_param_len(n)
        if state_rows.ndim != 2 or state_rows.shape[1] != self.state_len:
            raise DartMPCError(f"state rows must have {self.state_len} entries")
        stride = 0 if prm_rows.ndim == 1 else PL
        if prm_rows.shape[-1] != PL or (stride and prm_rows.shape[0] != B):
            raise DartMPCError(f"parameter rows must have {PL} entries")
        cfg = cfg if cfg is not None else arm_config()
        out = {"qdd": np.zeros((B, n)), "tau": np.zeros((B, n)), "loss": np.zeros(B),
               "status": np.zeros(B, dtype=np.int32), "iters": np.zeros(B, dtype=np.int32)}
        snap = np.zeros((B, self.snap_len)) if want_snap else None
        _check(lib().dart_arm_control_batch(ctypes.byref(self.cfg), ctypes.byref(cfg), B, n, _ptr(self.rows),
                                            self._stride(B), _ptr(state_rows), _ptr(prm_rows), stride, _ptr(snap),
                                            _ptr(out["qdd"]), _ptr(out["tau"]), _ptr(out["loss"]), _ptr(out["status"]),
                                            _ptr(out["iters"])), "dart_arm_control_batch")
        if want_snap:
            out["snap"] = snap
        return out

    def control_batch_dev(self, cfg, B, model_ptr, model_shared, state_ptr, prm_ptr, prm_shared, snap_ptr, qdd_ptr,
                          tau_ptr, loss_ptr, status_ptr, iters_ptr, stream=None):
        vp = ctypes.c_void_p
        _check(lib().dart_arm_control_batch_dev(ctypes.byref(self.cfg), ctypes.byref(cfg), B, self.n, vp(model_ptr),
                                                0 if model_shared else self.model_len, vp(state_ptr), vp(prm_ptr),
                                                0 if prm_shared else lib().dart_arm_param_len(self.n), vp(snap_ptr),
                                                vp(qdd_ptr), vp(tau_ptr), vp(loss_ptr), vp(status_ptr), vp(iters_ptr),
                                                vp(stream or 0)), "dart_arm_control_batch_dev")


def unpack_snapshot(rows, n) -> dict:
    """The inverse of ``pack_snapshot``: dict of [B, ...] arrays from [B, snapshot_len] rows."""
    rows = np.asarray(rows)
    out, o = {}, 0
    for k, w in SNAP_FIELDS:
        w = _width(w, n)
        shape = {"jac": (6, n), "jacDot": (6, n), "M": (n, n), "Mx_inv": (6, 6)}.get(k, (w,))
        out[k] = rows[:, o:o + w].reshape((rows.shape[0],) + shape).copy()
        o += w
    return out


def tray_from_arms(ee_pos, ee_quat, grasp=None) -> dict:
    """The tray two arms hold (``dart_tray_from_arms``, the coupling of the loop through the arms): ee_pos [E, 2, 3] the
    EE points, ee_quat [E, 2, 4] the EE orientations (wxyz, either sign), ``grasp`` [2, 7] (default ``DACTL_GRASP``).
    Returns dict(tray [E, 7] pos | quat, tilt [E, 2] = [-pitch, roll], yaw, gap, angle [E]); one experiment ([2, 3],
    [2, 4]) gives the same without the E axis."""
    one = np.ndim(ee_pos) == 2
    pos = np.ascontiguousarray(np.reshape(np.asarray(ee_pos, dtype=np.float64), (-1, 2, 3)))
    quat = np.ascontiguousarray(np.reshape(np.asarray(ee_quat, dtype=np.float64), (-1, 2, 4)))
    E = pos.shape[0]
    if quat.shape[0] != E:
        raise DartMPCError("ee_pos [E, 2, 3] and ee_quat [E, 2, 4] differ in E")
    g = np.ascontiguousarray(DACTL_GRASP if grasp is None else grasp, dtype=np.float64)
    if g.shape != (2, 7):
        raise DartMPCError("grasp transforms are [2, 7] (pos | quat)")
    tray, tilt, diag = np.zeros((E, 7)), np.zeros((E, 2)), np.zeros((E, 3))
    _check(lib().dart_tray_from_arms(E, _ptr(pos), _ptr(quat), _ptr(g), _ptr(tray), _ptr(tilt), _ptr(diag)),
           "dart_tray_from_arms")
    out = {"tray": tray, "tilt": tilt, "yaw": diag[:, 0].copy(), "gap": diag[:, 1].copy(), "angle": diag[:, 2].copy()}
    return {k: v[0] for k, v in out.items()} if one else out


class DualArmControl:
    """``DACTL.control`` (PMPC/src/dualctl.py) with dynamics and solve on the device: tray pose -> both arms' torques.

    ``control(pos, quat, q, qd)``: q, qd [2, n] (left, right) -> ((tau_L, tau_R), (loss_L, loss_R)); with a leading
    experiment axis ([E, 3], [E, 4], [E, 2, n]) the results are (tau [E, 2, n], loss [E, 2]).  qdd_prev is kept between
    calls as ``ArmControl`` does."""

    def __init__(self, model_L, model_R, params_L: dict, params_R: dict, n: int = None, grasp=None,
                 jacdot_point: int = JACDOT_REFERENCE, **cfg):
        self.n = int(n if n is not None else model_L.n)
        self.models = _model_rows([model_L, model_R], self.n, 2)
        self.prm = np.ascontiguousarray(np.stack([pack_params(params_L), pack_params(params_R)]))
        self.grasp = np.ascontiguousarray(DACTL_GRASP if grasp is None else grasp, dtype=np.float64)
        if self.grasp.shape != (2, 7):
            raise DartMPCError("grasp transforms are [2, 7] (pos | quat)")
        self.dcfg = arm_dyn_config(jacdot_point=int(jacdot_point))
        self.cfg = arm_config(**cfg)
        self.qdd_prev = None
        self.last_status = None
        self.last_mocap = None

    def control(self, pos, quat, q, qd):
        one = np.ndim(q) == 2
        n = self.n
        q = np.ascontiguousarray(np.reshape(np.asarray(q, dtype=np.float64), (-1, 2, n)))
        qd = np.ascontiguousarray(np.reshape(np.asarray(qd, dtype=np.float64), (-1, 2, n)))
        E = q.shape[0]
        tray = np.ascontiguousarray(np.concatenate([np.reshape(np.asarray(pos, dtype=np.float64), (E, 3)),
                                                    np.reshape(np.asarray(quat, dtype=np.float64), (E, 4))], axis=1))
        if self.qdd_prev is None or self.qdd_prev.shape != q.shape:
            self.qdd_prev = np.zeros_like(q)
        prm = np.ascontiguousarray(np.tile(self.prm, (E, 1)))
        B = 2 * E
        qdd, tau, loss = np.zeros((B, n)), np.zeros((B, n)), np.zeros(B)
        status, iters, mocap = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 7))
        _check(lib().dart_dual_arm_control(ctypes.byref(self.dcfg), ctypes.byref(self.cfg), E, n, _ptr(tray),
                                           _ptr(self.grasp), _ptr(q), _ptr(qd), _ptr(self.qdd_prev), _ptr(self.models),
                                           _ptr(prm), prm.shape[1], None, _ptr(mocap), _ptr(qdd), _ptr(tau), _ptr(loss),
                                           _ptr(status), _ptr(iters)), "dart_dual_arm_control")
        self.qdd_prev = qdd.reshape(E, 2, n).copy()
        self.last_status, self.last_mocap = status.reshape(E, 2), mocap.reshape(E, 2, 7)
        tau, loss = tau.reshape(E, 2, n), loss.reshape(E, 2)
        if one:
            return (tau[0, 0], tau[0, 1]), (float(loss[0, 0]), float(loss[0, 1]))
        return tau, loss
