"""Closed-loop rate of the device-resident rollouts (harness.rollout_pmpc / rollout_rmpc) against the host loops
of the same build (harness.run_pmpc / run_rmpc): B = 18 and B = 18 x 64 experiments, N = 20.  Each loop is run
once untimed (library and code-object load), then timed as a whole call (handle creation included on both
sides); the episode tolerance is 0 so that both RMPC loops run every step.  Reports steps/s, solves/s, and from
the rollout's logs the mean iterations per solve and the share of solves with status != 0 over the chain (RMPC:
warm-started; PMPC: cold-started, as in the reference).
Usage: python tools/rollout_rate.py [out.json] [steps] [steps_large]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
from dart_mpc import harness  # noqa: E402
from dart_mpc.workload import pmpc_batch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rollout_rate.json")
steps_small = int(sys.argv[2]) if len(sys.argv) > 2 else 300
steps_large = int(sys.argv[3]) if len(sys.argv) > 3 else 100


def timed(fn, *a, **kw):
    t0 = time.perf_counter()
    r = fn(*a, **kw)
    return r, time.perf_counter() - t0


def rate(B, steps, wall):
    return {"wall_s": wall, "steps_per_s": steps / wall, "solves_per_s": B * steps / wall}


def rmpc_inputs(B):
    rng = np.random.default_rng(7)
    tg = np.zeros((B, 4)); tg[:, 0] = rng.uniform(-0.12, 0.12, B); tg[:, 2] = rng.uniform(-0.1, 0.1, B)
    return np.zeros((B, 4)), tg


results = []
for seeds, steps in ((1, steps_small), (64, steps_large)):
    B = 18 * seeds
    S, T, P = pmpc_batch(seeds, seed0=0)
    harness.run_pmpc(S, T, P, 3); harness.rollout_pmpc(S, T, P, 3)
    (_, st_h), t_host = timed(harness.run_pmpc, S, T, P, steps)
    (_, st_d, X), t_dev = timed(harness.rollout_pmpc, S, T, P, steps, return_logs=True)
    row = {"controller": "PMPC", "B": B, "N": 20, "steps": steps, "host_loop": rate(B, steps, t_host),
           "rollout": dict(rate(B, steps, t_dev), loop_only_s=X["solve_time"] * steps,
                           mean_iters=float(X["iters"].mean()), share_status_nonzero=float(np.mean(st_d != 0))),
           "host_share_status_nonzero": float(np.mean(st_h != 0)), "speedup": t_host / t_dev}
    results.append(row)
    print(json.dumps(row), flush=True)

    x0, tg = rmpc_inputs(B)
    harness.run_rmpc(x0, tg, 3, pos_tol=0.0); harness.rollout_rmpc(x0, tg, 3, pos_tol=0.0)
    (_, st_h, _), t_host = timed(harness.run_rmpc, x0, tg, steps, pos_tol=0.0)
    (_, st_d, _, X), t_dev = timed(harness.rollout_rmpc, x0, tg, steps, pos_tol=0.0, return_logs=True)
    row = {"controller": "RMPC", "B": B, "N": 20, "steps": steps, "host_loop": rate(B, steps, t_host),
           "rollout": dict(rate(B, steps, t_dev), loop_only_s=X["solve_time"] * steps,
                           mean_iters=float(X["iters"].mean()), share_status_nonzero=float(np.mean(st_d != 0))),
           "host_share_status_nonzero": float(np.mean(st_h != 0)), "speedup": t_host / t_dev}
    results.append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"tool": "tools/rollout_rate.py", "results": results}, f, indent=1)
print("wrote", out_path)
