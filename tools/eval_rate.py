"""Rate of the LMPC evaluation (dart_lmpc_eval_dev: P policies in one device-resident rollout, metrics made on the
device, no log written) against what it replaces.  Workload: the B = 18 object configurations of
tools/compare_controllers.py (its object_pvec as the plant, workload.lmpc_batch's states and targets, at rest in
rotation), N = 30, ``steps`` steps, P fresh policies (seeds 0 .. P-1), zero noise, restoration on.
  (a) evaluate_dev, metrics-only, scores on, for P in {1, 2, 4, 8}: one call, P B instances in every launch;
  (b) P dart_lmpc_rollout_dev calls with logs, B instances each, back to back on the same handle and stream (what
      comparing P members cost before, without the copies), one synchronisation at the end;
  (c) today's LMPC leg of harness.compare_controllers with the same policy: harness.rollout_lmpc (the host entry, every
      log row copied back) plus harness.rollout_metrics in Python; beside it harness.evaluate_lmpc for P = 1 (the host
      entry in metrics-only mode).  Both include the handle's creation, as a user's call does.
(a) and (b) go through the device entries with the arrays resident (fresh state uploaded before the clock starts); all
cases of a round alternate, ``rounds`` rounds after one untimed round; median and min - max of the wall times.
Usage: python tools/eval_rate.py [out.json] [steps] [rounds]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from compare_controllers import object_pvec  # noqa: E402
from dart_mpc import _lib, harness  # noqa: E402
from dart_mpc.lmpc import LmpcPolicy  # noqa: E402
from dart_mpc.workload import N_CONFIGS, lmpc_batch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lmpc_eval", "eval_rate.json")
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B, N, PS = N_CONFIGS, 30, (1, 2, 4, 8)


def summary(walls, solves):
    w = np.asarray(walls)
    return {"wall_s": float(np.median(w)), "wall_min_s": float(w.min()), "wall_max_s": float(w.max()),
            "solves_per_s": solves / float(np.median(w)), "rounds": len(walls)}


def main():
    import torch
    D = lmpc_batch(1, seed0=0)
    x0 = D["state"].copy()
    x0[:, 4:] = 0.0
    target = D["target"]
    pvec = np.stack([object_pvec(b) for b in range(B)])
    pols = [LmpcPolicy(B, seed=s) for s in range(max(PS))]
    dev = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    ptr = lambda d: None if d is None else {k: v.data_ptr() for k, v in d.items()}
    tile = lambda a, P: np.tile(a, (P, 1))
    s = _lib.LmpcSolver(N=N, B_max=max(PS) * B)
    const = {P: dev(dict(target=tile(target, P), prm=np.tile(_lib.LMPC_PRM_DEFAULT, (P * B, 1)), pvec=tile(pvec, P),
                         weights=np.stack([p.weights for p in pols[:P]]),
                         current_k=np.concatenate([p.current_k for p in pols[:P]]))) for P in PS}
    last = {}

    def fresh(P, metrics):
        parts = [s.loop_state(x0, policy=p) for p in pols[:P]]
        st = {n: np.concatenate([q[n] for q in parts]) for n in parts[0]}
        if metrics:
            st["metrics"] = _lib.loop_metrics(P * B)
        return st

    def evaluate(P):
        c = const[P]
        st, sc = dev(fresh(P, True)), torch.zeros((P, 8), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.evaluate_dev(P, B, 0, steps, steps, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(), ptr(st),
                       None, pcfg=pols[0].cfg, weights=c["weights"].data_ptr(), current_k=c["current_k"].data_ptr(),
                       scores=sc.data_ptr())
        s.sync()
        wall = time.perf_counter() - t0
        last["eval", P] = (st["metrics"].cpu().numpy(), sc.cpu().numpy())
        return wall

    def rollouts(P):
        c = const[1]
        runs = []
        for l in range(P):
            w = dev(dict(weights=pols[l].weights, current_k=pols[l].current_k))
            runs.append((dev(s.loop_state(x0, policy=pols[l])), dev(_lib.loop_logs(_lib.LMPC_LOOP_LOGS, steps, B)), w))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for st, lg, w in runs:
            s.rollout_dev(B, 0, steps, steps, c["target"].data_ptr(), c["prm"].data_ptr(), c["pvec"].data_ptr(), ptr(st),
                          ptr(lg), pcfg=pols[0].cfg, weights=w["weights"].data_ptr(), current_k=w["current_k"].data_ptr())
        s.sync()
        wall = time.perf_counter() - t0
        last["roll", P] = runs[-1][1]
        return wall

    def compare_leg():
        t0 = time.perf_counter()
        logs, st, X = harness.rollout_lmpc(x0, target, pvec, steps, N=N, policy_seed=0, return_logs=True)
        U = np.stack([lg["u_cmd"] for lg in logs], axis=1)
        M = harness.rollout_metrics(X["X"], target, U, st, X["iters"], X["X"][:, :, 4:], 0.002)
        wall = time.perf_counter() - t0
        last["leg"] = M
        return wall

    def evaluate_host():
        t0 = time.perf_counter()
        out = harness.evaluate_lmpc(x0, target, pvec, steps, LmpcPolicy(B, seed=0), N=N)
        wall = time.perf_counter() - t0
        last["host"] = out["metrics"][0]
        return wall

    cases = [("evaluate_dev", P) for P in PS] + [("rollout_dev_x_P", P) for P in PS] + [("compare_leg", 1), ("evaluate_lmpc", 1)]
    fn = {"evaluate_dev": evaluate, "rollout_dev_x_P": rollouts, "compare_leg": lambda P: compare_leg(),
          "evaluate_lmpc": lambda P: evaluate_host()}
    walls = {c: [] for c in cases}
    try:
        for c in cases:
            fn[c[0]](c[1])
        for _ in range(rounds):
            for c in cases:
                walls[c].append(fn[c[0]](c[1]))
    finally:
        s.close()
    result = {"tool": "tools/eval_rate.py", "B": B, "N": N, "steps": steps, "rounds": rounds, "evaluate_dev": {},
              "rollout_dev_x_P": {}}
    for name, P in cases[:2 * len(PS)]:
        result[name][str(P)] = summary(walls[name, P], P * B * steps)
    for P in PS:
        a, b = result["evaluate_dev"][str(P)], result["rollout_dev_x_P"][str(P)]
        a["speedup_over_P_rollouts"] = b["wall_s"] / a["wall_s"]
        M, sc = last["eval", P]
        a["mean_iters"] = float(M[:, 5].sum() / M[:, 7].sum())
        a["status_nonzero"] = int(M[:, 4].sum())
        a["log_bytes_not_written"] = int(P * B * steps * (8 * (8 + 2 + 1 + 34 + 1) + 4 + 4))
    result["compare_leg_host_logs_python_metrics"] = summary(walls["compare_leg", 1], B * steps)
    result["evaluate_lmpc_host_metrics_only"] = summary(walls["evaluate_lmpc", 1], B * steps)
    result["evaluate_lmpc_host_metrics_only"]["speedup_over_compare_leg"] = (
        result["compare_leg_host_logs_python_metrics"]["wall_s"] / result["evaluate_lmpc_host_metrics_only"]["wall_s"])
    # the three paths made the same table (same policy, zero noise)
    same = lambda a, b: bool(np.array_equal(a[:, [1, 4, 5, 6, 7]], b[:, [1, 4, 5, 6, 7]])
                             and np.allclose(a[:, [0, 2, 3]], b[:, [0, 2, 3]], rtol=1e-12, atol=0))
    result["metrics_agree"] = {"evaluate_dev_P1_vs_compare_leg": same(last["eval", 1][0], last["leg"]),
                               "evaluate_lmpc_vs_compare_leg": same(last["host"], last["leg"])}
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
