"""Rate of the arm layer on the device: 36 arms (18 experiments x 2 xArm7 arms from tests/golden/xarm7_arm_models.npz) per
step, arrays resident, median and min - max over ``rounds`` rounds after one untimed round (the cases alternate).
  (a) dart_arm_dynamics_batch_dev alone: state -> snapshot;
  (b) dart_arm_control_batch_dev: dynamics + QP;
  (c) dart_arm_solve_batch_dev on the same snapshots: the QP alone (beside it the QP-only figure of the parent commit's
      README, 36 synthetic snapshots per launch);
  (d) dart_dual_arm_rollout_dev per step (K steps in one call, metrics only) against the same steps sequenced from the
      host: K calls of the host entry dart_dual_arm_rollout with one step each (copies and a synchronisation per step).
(a)-(c) time ``reps`` launches back to back and one synchronisation.  Also recorded, because DESIGN.md states them: the QP's
statuses and iteration counts on these xArm7 snapshots and in the loop, and what the two jacDot modes change in a 20-step loop.
Usage: python tools/arm_control_rate.py [out.json] [steps] [rounds]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import arm_qp  # noqa: E402  (the reference's parameter set only)
from dart_mpc import harness, lib  # noqa: E402
from dart_mpc import arm as A  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "arm_dyn", "control_rate.json")
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
E, n, reps = 18, 7, 200
HOME = np.array([0.0, -0.247, 0.0, 0.909, 0.0, 1.15644, 0.0])
PARENT_QP_ONLY = {"solves_per_s": 408.3e3, "us_per_launch": 36 / 408.3e3 * 1e6,
                  "source": "README of the parent commit: arm QP, 36 synthetic snapshots per launch"}


def summary(walls, per):
    w = np.asarray(walls) / per * 1e6
    return {"us": float(np.median(w)), "us_min": float(w.min()), "us_max": float(w.max()), "rounds": len(walls)}


def main():
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "xarm7_arm_models.npz"))
    rows, lim = g["rows"], g["limits"][0]
    rng = np.random.default_rng(0)
    prm = arm_qp.default_params()
    prow = A.pack_params(prm)
    B = 2 * E
    q0 = np.clip(HOME + rng.uniform(-0.3, 0.3, (E, 2, n)), lim[:, 0], lim[:, 1])
    qd0 = rng.uniform(-0.2, 0.2, (E, 2, n))
    u = 0.1 * np.sin(np.arange(steps)[:, None, None] * 0.05 + np.arange(E)[None, :, None] + np.array([0.0, 1.0]))
    tray = harness.tray_poses_from_tilt(u, [0.0, 0.0, 0.55])
    dyn = A.ArmDynamics(np.tile(rows, (E, 1)), n)
    targets = np.array([[A.DACTL_GRASP[a, :3] + [0, 0, 0.55] for a in range(2)] for _ in range(E)]).reshape(B, 3)
    state = dyn.pack_state(q0.reshape(B, n), qd0.reshape(B, n), np.zeros((B, n)), targets,
                           np.tile(A.DACTL_GRASP[:, 3:], (E, 1)))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    d_rows, d_state, d_prm = cu(np.tile(rows, (E, 1))), cu(state), cu(prow)
    d_snap = torch.zeros((B, dyn.snap_len), dtype=torch.float64, device="cuda")
    d_qdd, d_tau = torch.zeros((B, n), dtype=torch.float64, device="cuda"), torch.zeros((B, n), dtype=torch.float64, device="cuda")
    d_loss = torch.zeros(B, dtype=torch.float64, device="cuda")
    d_st, d_it = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    solver, qcfg = A.ArmSolver(n), A.arm_config()
    outs = (d_qdd.data_ptr(), d_tau.data_ptr(), d_loss.data_ptr(), d_st.data_ptr(), d_it.data_ptr())

    def timed(launch, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            launch()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def dynamics():
        return timed(lambda: dyn.dynamics_batch_dev(B, d_rows.data_ptr(), False, d_state.data_ptr(), d_snap.data_ptr()), reps)

    def control():
        return timed(lambda: dyn.control_batch_dev(qcfg, B, d_rows.data_ptr(), False, d_state.data_ptr(), d_prm.data_ptr(),
                                                   True, d_snap.data_ptr(), *outs), reps)

    def solve():
        return timed(lambda: solver.solve_batch_dev(B, d_snap.data_ptr(), d_prm.data_ptr(), True, *outs), reps)

    L, vp = lib(), ctypes.c_void_p
    dcfg = A.arm_dyn_config()
    d_tray, d_grasp, d_models = cu(tray), cu(A.DACTL_GRASP), cu(rows)
    d_prm2 = cu(np.tile(prow, (B, 1)))
    d_work = torch.zeros(L.dart_dual_arm_work_len(E, n), dtype=torch.float64, device="cuda")
    last = {}

    def rollout_dev():
        q, qd, qp, met = cu(q0), cu(qd0), cu(np.zeros_like(q0)), cu(np.zeros((B, A.NMETRIC)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.dart_dual_arm_rollout_dev(ctypes.byref(dcfg), ctypes.byref(qcfg), E, n, steps, steps, vp(d_tray.data_ptr()),
                                         vp(d_grasp.data_ptr()), vp(d_models.data_ptr()), vp(d_models.data_ptr()),
                                         vp(d_prm2.data_ptr()), d_prm2.shape[1], vp(q.data_ptr()), vp(qd.data_ptr()),
                                         vp(qp.data_ptr()), vp(met.data_ptr()), vp(d_work.data_ptr()), *([None] * 6), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        last["dev"] = (q.cpu().numpy(), met.cpu().numpy())
        return wall

    def rollout_host_steps():
        q, qd, qp, met = q0, qd0, None, None
        t0 = time.perf_counter()
        for k in range(steps):
            r = harness.rollout_dual_arm(q, qd, tray[k:k + 1], rows, prm, 1, metrics_only=True, qdd_prev0=qp, metrics0=met)
            q, qd, qp, met = r["q"], r["qd"], r["qdd_prev"], r["metrics"]
        wall = time.perf_counter() - t0
        last["host"] = (q, met)
        return wall

    cases = {"dynamics_batch_dev": (dynamics, reps), "control_batch_dev": (control, reps), "solve_batch_dev": (solve, reps),
             "rollout_dual_arm_dev": (rollout_dev, steps), "rollout_host_sequenced": (rollout_host_steps, steps)}
    walls = {k: [] for k in cases}
    for fn, _ in cases.values():
        fn()
    for _ in range(rounds):
        for k, (fn, _) in cases.items():
            walls[k].append(fn())
    result = {"tool": "tools/arm_control_rate.py", "arms_per_step": B, "n": n, "reps": reps, "steps": steps, "rounds": rounds}
    for k, (_, per) in cases.items():
        result[k] = summary(walls[k], per)
        result[k]["unit"] = "us per step of 36 arms" if k.startswith("rollout") else "us per launch of 36 arms"
    result["solve_batch_dev"]["parent_qp_only"] = PARENT_QP_ONLY
    result["rollout_dual_arm_dev"]["speedup_over_host_sequenced"] = (result["rollout_host_sequenced"]["us"]
                                                                     / result["rollout_dual_arm_dev"]["us"])
    result["rollout_bits_agree"] = bool(np.array_equal(last["dev"][0], last["host"][0])
                                        and np.array_equal(last["dev"][1], last["host"][1]))
    # what the QP does on real xArm7 snapshots
    st, it = d_st.cpu().numpy(), d_it.cpu().numpy()
    met = last["dev"][1]
    result["xarm7_qp"] = {"snapshot_statuses": {int(s): int(c) for s, c in zip(*np.unique(st, return_counts=True))},
                          "snapshot_iters_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())],
                          "loop_status_nonzero_steps": int(met[:, 3].sum()),
                          "loop_iters_per_solve": float(met[:, 4].sum() / (B * steps)),
                          "loop_final_pos_error_m_min_max": [float(met[:, 0].min()), float(met[:, 0].max())],
                          "loop_max_tau_ratio": float(met[:, 5].max())}
    lg = harness.rollout_dual_arm(q0, qd0, tray, rows, prm, steps)["logs"]["status"]
    result["xarm7_qp"]["loop_statuses"] = {int(s): int(c) for s, c in zip(*np.unique(lg, return_counts=True))}
    # the two jacDot modes in a 20-step loop (E = 2)
    two = {m: harness.rollout_dual_arm(q0[:2], qd0[:2], tray[:20, :2], rows, prm, 20, jacdot_point=m) for m in (0, 1)}
    dif = lambda k: float(np.max(np.abs(two[0]["logs"][k] - two[1]["logs"][k])))     # noqa: E731
    s0 = A.unpack_snapshot(A.ArmDynamics(rows[0], n, jacdot_point=0).dynamics_batch(state[:2]), n)
    s1 = A.unpack_snapshot(A.ArmDynamics(rows[0], n, jacdot_point=1).dynamics_batch(state[:2]), n)
    result["jacdot_modes_20_steps"] = {
        "max_abs_diff_tau": dif("tau"), "max_abs_diff_q": dif("q"), "max_abs_diff_ee_pos": dif("ee_pos"),
        "statuses_equal": bool(np.array_equal(two[0]["logs"]["status"], two[1]["logs"]["status"])),
        "max_abs_jacDot_qd_reference": float(np.max(np.abs(np.einsum("bij,bj->bi", s0["jacDot"], s0["qd"])))),
        "max_abs_jacDot_qd_body": float(np.max(np.abs(np.einsum("bij,bj->bi", s1["jacDot"], s1["qd"])))),
        "max_abs_diff_jacDot": float(np.max(np.abs(s0["jacDot"] - s1["jacDot"])))}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
