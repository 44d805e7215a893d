"""Rate of the PMPC loop closed through the dual-arm layer: E = 18 experiments (the 18 object configurations of
workload.pmpc_batch, 36 xArm7 arms from tests/golden/xarm7_arm_models.npz started at the level grasp pose), N = 20, arrays
resident, median and min - max over ``rounds`` rounds after one untimed round (the cases alternate).  Per step:
  (a) stack_rollout_dev          the resident loop (dart_pmpc_stack_rollout_dev, K steps in one call, metrics only), in
                                 both couple modes;
  (b) stack_host_sequenced       the same launches sequenced from the host: K calls of the host entry
                                 dart_pmpc_stack_rollout with one step each (copies and a synchronisation per step);
  (c) pmpc_rollout_dev + dual_arm_rollout_dev   the two loops the stack is made of, each alone (dart_pmpc_rollout_dev with
                                 its logs; dart_dual_arm_rollout_dev, metrics only, fed the poses that run commands, which
                                 makes it the arm half of the ride-mode stack loop bit for bit): their sum is what the
                                 ride-mode stack loop costs without its two small launches;
  (d) command / couple launches alone (dart_pmpc_stack_loop_step_dev, ``reps`` launches back to back, one synchronisation).
Every timing is a host clock around work that ends in a device synchronisation.
Usage: python tools/stack_rate.py [--controller pmpc|rmpc] [out.json] [steps] [rounds]

--controller rmpc measures the RMPC loop through the arms instead (dart_rmpc_stack_*; the object's start state and
target of workload.pmpc_batch, mu of the configuration as the plant's viscous friction) and writes
profiles/stack/rmpc_stack_rate.json by default: (a) the resident loop in both couple modes, metrics only; (b) the same
steps sequenced from the host, K calls of the host entry dart_rmpc_stack_rollout with one step each, their bits checked
against (a); (c) dart_rmpc_rollout_dev alone (with its logs) and dart_dual_arm_rollout_dev alone, fed the poses the
ride-mode run commands, and their sum.
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
import dart_mpc  # noqa: E402
from dart_mpc import _lib as L  # noqa: E402
from dart_mpc import arm as A  # noqa: E402
from dart_mpc import harness  # noqa: E402
from dart_mpc.workload import pmpc_batch  # noqa: E402

argv = list(sys.argv)
controller = "pmpc"
if "--controller" in argv:
    controller = argv[argv.index("--controller") + 1]
    del argv[argv.index("--controller"):argv.index("--controller") + 2]
if controller not in ("pmpc", "rmpc"):
    sys.exit("--controller is pmpc or rmpc")
out_path = argv[1] if len(argv) > 1 else os.path.join(
    ROOT, "profiles", "stack", "rmpc_stack_rate.json" if controller == "rmpc" else "stack_rate.json")
steps = int(argv[2]) if len(argv) > 2 else 200
rounds = int(argv[3]) if len(argv) > 3 else 5
E, n, N, Ts, reps = 18, 7, 20, 0.002, 200


def summary(walls, per):
    w = np.asarray(walls) / per * 1e6
    return {"us": float(np.median(w)), "us_min": float(w.min()), "us_max": float(w.max()), "rounds": len(walls)}


def main():
    import torch
    gold = os.path.join(ROOT, "tests", "golden")
    rows = np.load(os.path.join(gold, "xarm7_arm_models.npz"))["rows"]
    g = np.load(os.path.join(gold, "xarm7_grasp_q.npz"))
    S0, T, P = pmpc_batch(1)
    q0 = np.tile(g["q"], (E, 1, 1))
    qd0 = np.zeros_like(q0)
    prm = arm_qp.default_params()
    B = 2 * E
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    solver = dart_mpc.Solver(N=N, Ts=Ts, tol=1e-8, B_max=E, device=0)
    lib, vp = L.lib(), ctypes.c_void_p
    work = torch.zeros(lib.dart_stack_work_len(E, n), dtype=torch.float64, device="cuda")
    last = {}

    def fresh():
        return harness.stack_arrays(S0, T, P, q0, qd0, rows, prm, g["tray_pos"], Ts=Ts)[0]

    def stack_dev(couple):
        d = {k: cu(v) for k, v in fresh().items()}
        d["work"] = work
        ptrs = {k: v.data_ptr() for k, v in d.items()}
        scfg = L.stack_config(couple)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.stack_rollout_dev(E, n, 0, steps, 0, d["arm_prm"].shape[1], ptrs, scfg=scfg)
        solver.sync()
        wall = time.perf_counter() - t0
        last["dev_" + couple] = {k: d[k].cpu().numpy() for k in ("x", "q", "metrics", "stack_metrics", "arm_metrics")}
        return wall

    def stack_host_steps():
        a = fresh()
        scfg = L.stack_config("achieved")
        t0 = time.perf_counter()
        for k in range(steps):
            solver.stack_rollout(E, n, k, 1, 0, a["arm_prm"].shape[1], a, scfg=scfg)
        wall = time.perf_counter() - t0
        last["host"] = {k: a[k] for k in ("x", "q", "metrics", "stack_metrics", "arm_metrics")}
        return wall

    d_logs = {k: cu(v) for k, v in L.loop_logs(L.PMPC_LOOP_LOGS, steps, E).items()}
    d_T, d_P = cu(T), cu(P)

    def pmpc_dev():
        st = {"x": cu(S0), "tilt": cu(np.zeros((E, 2)))}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.rollout_dev(E, 0, steps, steps, d_T.data_ptr(), d_P.data_ptr(), {k: v.data_ptr() for k, v in st.items()},
                           {k: v.data_ptr() for k, v in d_logs.items()})
        solver.sync()
        return time.perf_counter() - t0

    # the poses that run commands (tray_pos | its log_quat): fed these, the arm loop does the arm half of the ride-mode
    # stack loop bit for bit, so the two parts and the ride-mode stack loop do the same arithmetic
    pmpc_dev()
    d_tray = torch.cat([cu(np.broadcast_to(g["tray_pos"], (steps, E, 3))), d_logs["quat_tray"]], dim=2).contiguous()
    d_grasp, d_models = cu(A.DACTL_GRASP), cu(rows)
    d_aprm = cu(np.tile(A.pack_params(prm), (B, 1)))
    dcfg, qcfg = A.arm_dyn_config(), A.arm_config()

    def arm_dev():
        q, qd, qp, met = cu(q0), cu(qd0), cu(np.zeros_like(q0)), cu(np.zeros((B, A.NMETRIC)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.dart_dual_arm_rollout_dev(ctypes.byref(dcfg), ctypes.byref(qcfg), E, n, steps, steps, vp(d_tray.data_ptr()),
                                           vp(d_grasp.data_ptr()), vp(d_models.data_ptr()), vp(d_models.data_ptr()),
                                           vp(d_aprm.data_ptr()), d_aprm.shape[1], vp(q.data_ptr()), vp(qd.data_ptr()),
                                           vp(qp.data_ptr()), vp(met.data_ptr()), vp(work.data_ptr()), *([None] * 6), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        last["arm"] = {"q": q.cpu().numpy().reshape(B, n), "arm_metrics": met.cpu().numpy()}
        return wall

    # the two small launches alone, on the arrays one resident step leaves behind
    step_d = {k: cu(v) for k, v in fresh().items()}
    SL = lib.dart_arm_snapshot_len(n)
    step_d.update(snap=work, ee_quat=work[lib.dart_dual_arm_work_len(E, n):], tray_cmd=cu(np.zeros((E, 7))),
                  x0=cu(np.zeros((E, 6))), u0=cu(np.zeros((E, 2))), f=cu(np.zeros(E)), status=cu(np.zeros(E, np.int32)),
                  iters=cu(np.zeros(E, np.int32)))
    step_p = {k: v.data_ptr() for k, v in step_d.items()}
    assert work.numel() >= B * SL

    def launches(phase):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            solver.stack_loop_step_dev(E, n, 0, phase, 1, 1, 0, step_p)
        solver.sync()
        return time.perf_counter() - t0

    cases = {"stack_rollout_dev_achieved": (lambda: stack_dev("achieved"), steps),
             "stack_rollout_dev_ride": (lambda: stack_dev("ride"), steps),
             "stack_host_sequenced": (stack_host_steps, steps),
             "pmpc_rollout_dev": (pmpc_dev, steps), "dual_arm_rollout_dev": (arm_dev, steps),
             "command_launch": (lambda: launches(L.STACK_COMMAND), reps),
             "couple_object_launch": (lambda: launches(L.STACK_COUPLE), reps)}
    walls = {k: [] for k in cases}
    for fn, _ in cases.values():
        fn()
    for _ in range(rounds):
        for k, (fn, _) in cases.items():
            walls[k].append(fn())
    res = {"tool": "tools/stack_rate.py", "experiments": E, "arms_per_step": B, "n": n, "N": N, "steps": steps, "reps": reps,
           "rounds": rounds, "launches_per_step": 6}
    for k, (_, per) in cases.items():
        res[k] = summary(walls[k], per)
        res[k]["unit"] = "us per launch" if k.endswith("_launch") else "us per step of 18 experiments"
    parts = res["pmpc_rollout_dev"]["us"] + res["dual_arm_rollout_dev"]["us"]
    small = res["command_launch"]["us"] + res["couple_object_launch"]["us"]
    res["sum_of_the_two_loops_us"] = parts
    res["sum_plus_the_two_small_launches_us"] = parts + small
    res["ride_stack_over_sum_of_parts"] = res["stack_rollout_dev_ride"]["us"] / (parts + small)
    res["ride_stack_minus_the_two_loops_us"] = res["stack_rollout_dev_ride"]["us"] - parts
    res["arm_loop_bits_equal_ride_stack"] = bool(all(np.array_equal(last["arm"][k], last["dev_ride"][k])
                                                     for k in ("q", "arm_metrics")))
    res["speedup_over_host_sequenced"] = res["stack_host_sequenced"]["us"] / res["stack_rollout_dev_achieved"]["us"]
    res["host_sequenced_bits_agree"] = bool(all(np.array_equal(last["host"][k].reshape(-1), last["dev_achieved"][k].reshape(-1))
                                                for k in last["host"]))
    for c in ("achieved", "ride"):
        m = last["dev_" + c]
        res["run_" + c] = {"stack_metrics_max": dict(zip(L.STACK_METRIC_SLOTS, m["stack_metrics"].max(axis=0).tolist())),
                           "object_final_error_mean": float(m["metrics"][:, 0].mean()),
                           "pmpc_status_nonzero_steps": float(m["metrics"][:, 4].sum()),
                           "pmpc_iters_per_solve": float(m["metrics"][:, 5].sum() / (E * steps)),
                           "arm_qp_iters_per_solve": float(m["arm_metrics"][:, 4].sum() / (B * steps))}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    solver.close()


def main_rmpc():
    import torch
    gold = os.path.join(ROOT, "tests", "golden")
    rows = np.load(os.path.join(gold, "xarm7_arm_models.npz"))["rows"]
    g = np.load(os.path.join(gold, "xarm7_grasp_q.npz"))
    S0, T, P = pmpc_batch(1)
    x0, tg, mu = S0[:, :4], T[:, :4], np.ascontiguousarray(P[:, 0])
    q0 = np.tile(g["q"], (E, 1, 1))
    qd0 = np.zeros_like(q0)
    prm = arm_qp.default_params()
    B = 2 * E
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    solver = dart_mpc.RmpcSolver(N=N, Ts=Ts, B_max=E, device=0)
    lib, vp = L.lib(), ctypes.c_void_p
    work = torch.zeros(lib.dart_stack_work_len(E, n), dtype=torch.float64, device="cuda")
    keep = ("x", "theta", "w", "q", "metrics", "stack_metrics", "arm_metrics")
    last = {}

    def fresh():
        return harness.rmpc_stack_arrays(x0, tg, q0, qd0, rows, prm, g["tray_pos"], mu=mu, N=N, Ts=Ts)[0]

    rprm = fresh()["prm"]
    d_slogs = {k: cu(v) for k, v in L.loop_logs(L.RMPC_STACK_LOGS, steps, E).items()}

    def stack_dev(couple, logs=None):
        d = {k: cu(v) for k, v in fresh().items()}
        d["work"] = work
        ptrs = {k: v.data_ptr() for k, v in d.items()}
        scfg = L.stack_config(couple)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.rmpc_stack_rollout_dev(E, n, 0, steps, steps if logs else 0, d["arm_prm"].shape[1], ptrs, None, logs, None,
                                      scfg=scfg)
        solver.sync()
        wall = time.perf_counter() - t0
        last["dev_" + couple] = {k: d[k].cpu().numpy() for k in keep}
        return wall

    def stack_host_steps():
        a = fresh()
        scfg = L.stack_config("achieved")
        t0 = time.perf_counter()
        for k in range(steps):
            solver.rmpc_stack_rollout(E, n, k, 1, 0, a["arm_prm"].shape[1], a, scfg=scfg)
        wall = time.perf_counter() - t0
        last["host"] = {k: a[k] for k in keep}
        return wall

    d_logs = {k: cu(v) for k, v in L.loop_logs(L.RMPC_LOOP_LOGS, steps, E).items()}
    d_T, d_P, d_mu = cu(tg), cu(rprm), cu(mu)

    def rmpc_dev():
        st = {k: cu(v) for k, v in solver.loop_state(x0).items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.rollout_dev(E, 0, steps, steps, d_T.data_ptr(), d_P.data_ptr(), d_mu.data_ptr(),
                           {k: v.data_ptr() for k, v in st.items()}, {k: v.data_ptr() for k, v in d_logs.items()})
        solver.sync()
        return time.perf_counter() - t0

    # the poses the ride-mode run commands (tray_pos | its log_quat): fed these, the arm loop does the arm half of the
    # ride-mode stack loop bit for bit
    stack_dev("ride", {k: v.data_ptr() for k, v in d_slogs.items()})
    d_tray = torch.cat([cu(np.broadcast_to(g["tray_pos"], (steps, E, 3))), d_slogs["quat_tray"]], dim=2).contiguous()
    d_grasp, d_models = cu(A.DACTL_GRASP), cu(rows)
    d_aprm = cu(np.tile(A.pack_params(prm), (B, 1)))
    dcfg, qcfg = A.arm_dyn_config(), A.arm_config()

    def arm_dev():
        q, qd, qp, met = cu(q0), cu(qd0), cu(np.zeros_like(q0)), cu(np.zeros((B, A.NMETRIC)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.dart_dual_arm_rollout_dev(ctypes.byref(dcfg), ctypes.byref(qcfg), E, n, steps, steps, vp(d_tray.data_ptr()),
                                           vp(d_grasp.data_ptr()), vp(d_models.data_ptr()), vp(d_models.data_ptr()),
                                           vp(d_aprm.data_ptr()), d_aprm.shape[1], vp(q.data_ptr()), vp(qd.data_ptr()),
                                           vp(qp.data_ptr()), vp(met.data_ptr()), vp(work.data_ptr()), *([None] * 6), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        last["arm"] = {"q": q.cpu().numpy().reshape(B, n), "arm_metrics": met.cpu().numpy()}
        return wall

    cases = {"stack_rollout_dev_achieved": lambda: stack_dev("achieved"), "stack_rollout_dev_ride": lambda: stack_dev("ride"),
             "stack_host_sequenced": stack_host_steps, "rmpc_rollout_dev": rmpc_dev, "dual_arm_rollout_dev": arm_dev}
    walls = {k: [] for k in cases}
    for fn in cases.values():
        fn()
    for _ in range(rounds):
        for k, fn in cases.items():
            walls[k].append(fn())
    res = {"tool": "tools/stack_rate.py", "controller": "rmpc", "experiments": E, "arms_per_step": B, "n": n, "N": N,
           "steps": steps, "rounds": rounds, "launches_per_step": 6}
    for k in cases:
        res[k] = summary(walls[k], steps)
        res[k]["unit"] = "us per step of 18 experiments"
    parts = res["rmpc_rollout_dev"]["us"] + res["dual_arm_rollout_dev"]["us"]
    res["sum_of_the_two_loops_us"] = parts
    res["ride_stack_minus_the_two_loops_us"] = res["stack_rollout_dev_ride"]["us"] - parts
    res["achieved_stack_minus_the_two_loops_us"] = res["stack_rollout_dev_achieved"]["us"] - parts
    res["arm_loop_bits_equal_ride_stack"] = bool(all(np.array_equal(last["arm"][k], last["dev_ride"][k])
                                                     for k in ("q", "arm_metrics")))
    res["speedup_over_host_sequenced"] = res["stack_host_sequenced"]["us"] / res["stack_rollout_dev_achieved"]["us"]
    res["resident_max_below_host_sequenced_min"] = bool(
        max(res["stack_rollout_dev_achieved"]["us_max"], res["stack_rollout_dev_ride"]["us_max"])
        < res["stack_host_sequenced"]["us_min"])
    res["host_sequenced_bits_agree"] = bool(all(np.array_equal(last["host"][k].reshape(-1), last["dev_achieved"][k].reshape(-1))
                                                for k in last["host"]))
    for c in ("achieved", "ride"):
        m = last["dev_" + c]
        res["run_" + c] = {"stack_metrics_max": dict(zip(L.STACK_METRIC_SLOTS, m["stack_metrics"].max(axis=0).tolist())),
                           "object_final_error_mean": float(m["metrics"][:, 0].mean()),
                           "rmpc_status_nonzero_steps": float(m["metrics"][:, 4].sum()),
                           "rmpc_iters_per_solve": float(m["metrics"][:, 5].sum() / (E * steps)),
                           "arm_qp_iters_per_solve": float(m["arm_metrics"][:, 4].sum() / (B * steps))}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)
    solver.close()


if __name__ == "__main__":
    main_rmpc() if controller == "rmpc" else main()
