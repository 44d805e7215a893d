"""What the arm layer does to the PMPC loop (harness.rollout_stack): the 18 object configurations of workload.pmpc_batch,
each on a tray held by two xArm7 (tests/golden/xarm7_arm_models.npz, started at the level grasp pose of
tests/golden/xarm7_grasp_q.npz and settled), in both couple modes, with the controller's own arm models as the plant and
with a payload (a point mass on each arm's last link) in ``plant_models`` that the controller does not know about.

Writes one JSON file: per run the loop metrics [18][8] (_lib.METRIC_SLOTS), the stack metrics [18][8]
(_lib.STACK_METRIC_SLOTS), the arm metrics [36][6] (arm.ARM_METRIC_SLOTS) and their summaries.
Usage: python tools/stack_metrics.py [--controller pmpc|rmpc] [out.json] [steps] [payload_kg] [settle_steps]

--controller rmpc runs the same study with the RMPC loop (harness.rollout_stack_rmpc) on the same 18 configurations (the
object's start state and target of workload.pmpc_batch, mu of the configuration as the plant's viscous friction, the
controller's parameters rob_ctrl.py's) and writes profiles/stack/rmpc_stack_metrics.json by default.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import arm_qp  # noqa: E402  (the reference's parameter set only)
from dart_mpc import harness  # noqa: E402
from dart_mpc._lib import METRIC_SLOTS, STACK_METRIC_SLOTS  # noqa: E402
from dart_mpc.arm import ARM_METRIC_SLOTS  # noqa: E402
from dart_mpc.arm_model import ArmModel  # noqa: E402
from dart_mpc.workload import N_CONFIGS, config_name, pmpc_batch  # noqa: E402


def main():
    argv = list(sys.argv)
    controller = "pmpc"
    if "--controller" in argv:
        i = argv.index("--controller")
        controller = argv[i + 1]
        del argv[i:i + 2]
    if controller not in ("pmpc", "rmpc"):
        sys.exit("--controller is pmpc or rmpc")
    rm = controller == "rmpc"
    default = "rmpc_stack_metrics.json" if rm else "stack_metrics.json"
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "stack", default)
    steps = int(argv[2]) if len(argv) > 2 else 500
    payload = float(argv[3]) if len(argv) > 3 else 1.0
    settle = int(argv[4]) if len(argv) > 4 else 100
    gold = os.path.join(ROOT, "tests", "golden")
    rows = np.load(os.path.join(gold, "xarm7_arm_models.npz"))["rows"]
    g = np.load(os.path.join(gold, "xarm7_grasp_q.npz"))
    S0, T, P = pmpc_batch(1)
    E = N_CONFIGS
    q0 = np.tile(g["q"], (E, 1, 1))
    heavy = [ArmModel.from_row(r, 7).with_payload(payload) for r in rows]
    prm = arm_qp.default_params()
    res = {"tool": "tools/stack_metrics.py", "steps": steps, "settle_steps": settle, "payload_kg": payload, "E": E,
           "configs": [config_name(b) for b in range(E)], "loop_slots": list(METRIC_SLOTS),
           "stack_slots": list(STACK_METRIC_SLOTS), "arm_slots": list(ARM_METRIC_SLOTS), "runs": {}}
    if rm:
        res["controller"] = "rmpc"
    for couple in ("ride", "achieved"):
        for name, plant in (("no_payload", None), ("payload", heavy)):
            if rm:
                r = harness.rollout_stack_rmpc(S0[:, :4], T[:, :4], q0, np.zeros_like(q0), rows, prm, steps, g["tray_pos"],
                                               couple=couple, mu=P[:, 0], plant_models=plant, metrics_only=True,
                                               settle_steps=settle)
            else:
                r = harness.rollout_stack(S0, T, P, q0, np.zeros_like(q0), rows, prm, steps, g["tray_pos"], couple=couple,
                                          plant_models=plant, metrics_only=True, settle_steps=settle)
            M, SM, AM = r["metrics"], r["stack_metrics"], r["arm"]["metrics"]
            res["runs"][f"{couple}_{name}"] = {
                "metrics": M.tolist(), "stack_metrics": SM.tolist(), "arm_metrics": AM.tolist(),
                "summary": {"mean_steady_state_error_m": float(M[:, 0].mean()), "converged": int((M[:, 1] >= 0).sum()),
                            "mean_convergence_step": float(M[M[:, 1] >= 0, 1].mean()) if (M[:, 1] >= 0).any() else None,
                            controller + "_status_nonzero_steps": float(M[:, 4].sum()),
                            "max_tilt_deviation_rad": float(SM[:, 1].max()), "max_yaw_rad": float(SM[:, 2].max()),
                            "max_grasp_gap_m": float(SM[:, 3].max()), "max_disagreement_angle_rad": float(SM[:, 4].max()),
                            "max_tray_pos_error_m": float(SM[:, 5].max()), "held_steps": float(SM[:, 6].sum()),
                            "max_arm_pos_error_m": float(AM[:, 1].max()), "arm_status_nonzero_steps": float(AM[:, 3].sum()),
                            "max_tau_ratio": float(AM[:, 5].max()), "wall_s": r["wall_s"]}}
            print(couple, name, res["runs"][f"{couple}_{name}"]["summary"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
