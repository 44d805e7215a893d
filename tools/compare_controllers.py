"""PMPC, RMPC and LMPC on the same objects (harness.compare_controllers): the 18 object configurations of the reference's
comparison (cube, cylinder, sphere x two masses x three frictions), ``seeds`` draws of start and target each, on
harness.LmpcPlant.  The plant's parameters are the point mass of each configuration (workload.point_mass_pvec: mass m,
viscous friction mu m) plus, per shape, what makes the simple models break: Coulomb / Stribeck friction for the cube,
a rolling radius for the cylinder and the sphere, and a centre-of-mass height (toppling) for the cylinder.  These shape
terms are this tool's own choice of illustrative values, not the reference's.

Writes one JSON file: per controller the metrics table [B][8] (_lib.METRIC_SLOTS) and its mean over the seeds per
configuration.
Usage: python tools/compare_controllers.py [out.json] [steps] [seeds]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dart-dual-arm-non-prehensile-manipulation_amd"))
from dart_mpc import harness  # noqa: E402
from dart_mpc._lib import METRIC_SLOTS  # noqa: E402
from dart_mpc.workload import FRICTIONS, MASSES, N_CONFIGS, SHAPE_WEIGHTS, config_name, lmpc_batch, point_mass_pvec  # noqa: E402


def object_pvec(b):
    """The plant's parameter row of object configuration ``b`` (index map of rlmpc2.py:301-334)."""
    shape_idx, rest = divmod(int(b), 6)
    mass_idx, fric_idx = divmod(rest, 3)
    m, mu = MASSES[mass_idx], FRICTIONS[fric_idx]
    p = point_mass_pvec(mu, m)[0]
    shape = SHAPE_WEIGHTS[shape_idx][0]
    g = 9.81
    if shape == "cube":             # slides: static and Coulomb friction [F_s, F_c, B, v_s, eps] on both axes
        p[6:11] = p[11:16] = [0.06 * m * g, 0.04 * m * g, 0.0, 0.01, 0.01]
    else:                           # rolls: radius, inertia of the shape, light rolling resistance
        r = 0.03
        p[18:20] = r
        p[16:18] = (0.5 if shape == "cylinder" else 0.4) * m * r * r
        p[6:11] = p[11:16] = [0.02 * m * g, 0.015 * m * g, 0.0, 0.01, 0.01]
        p[20:22] = 1e-4
        if shape == "cylinder":     # stands upright: a centre of mass above the tray
            p[32:34] = 0.04
    return p


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cross_plant", "compare_controllers.json")
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    seeds = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    D = lmpc_batch(seeds, seed0=0)
    B = N_CONFIGS * seeds
    x0 = D["state"].copy()
    x0[:, 4:] = 0.0                                             # at rest in rotation
    pvec = np.stack([object_pvec(i % N_CONFIGS) for i in range(B)])
    tables = harness.compare_controllers(x0, D["target"][:, [0, 2]], pvec, steps)
    result = {"tool": "tools/compare_controllers.py", "steps": steps, "seeds": seeds, "B": B, "slots": list(METRIC_SLOTS),
              "configs": [config_name(b) for b in range(N_CONFIGS)], "metrics": {}, "mean_per_config": {}}
    for name, M in tables.items():
        result["metrics"][name] = M.tolist()
        result["mean_per_config"][name] = M.reshape(seeds, N_CONFIGS, 8).mean(axis=0).tolist()
        conv = M[:, 1] >= 0
        print(f"{name}: converged {int(conv.sum())}/{B}, mean steady-state error {M[:, 0].mean():.4f} m, mean effort "
              f"{M[:, 2].mean():.4f}, solves with status != 0 {int(M[:, 4].sum())}, mean iterations "
              f"{M[:, 5].sum() / M[:, 7].sum():.1f}, max |rotation| {M[:, 6].max():.3f} rad")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
