"""Regenerates tests/golden/xarm7_arm_models.npz: the two xArm7 model rows (left, right) of the dual-arm scene.

    python tests/golden/make_xarm7_arm_models.py <reference checkout>

Reads the reference's scene files (data only) under PMPC/models/xarm7: ``chainL.xml`` / ``chainR.xml`` (the arms),
``xarm7.xml`` (the ``<default>`` tree) and ``world_cube_m=0.5_mu=0.05.xml`` (the poses of the two
``*_world_virtual_link`` bodies the chains are included in, and gravity).  ``body_name`` and ``offset`` are those of
PMPC/main.py:28-53.  The gripper below joint 7 (base, knuckles, fingers) is composed into link 7 with the finger joints at
0.  The fixture holds numbers only: ``rows`` [2, 172], ``joint_names`` [2, 7], ``limits`` [2, 7, 2].
"""
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dart-dual-arm-non-prehensile-manipulation_amd"))

from dart_mpc.arm_model import ArmModel  # noqa: E402


def main(ref):
    d = os.path.join(ref, "PMPC", "models", "xarm7")
    world = ET.parse(os.path.join(d, "world_cube_m=0.5_mu=0.05.xml")).getroot()
    gravity = [float(v) for v in world.find("option").get("gravity").split()]
    rows, names, limits = [], [], []
    for side in "LR":
        virt = world.find(f".//body[@name='{side}_world_virtual_link']")
        inc = virt.find("include").get("file")
        assert os.path.basename(inc) == f"chain{side}.xml", inc
        m = ArmModel.from_mjcf(os.path.join(d, f"chain{side}.xml"), os.path.join(d, "xarm7.xml"),
                               base_pos=[float(v) for v in virt.get("pos").split()],
                               base_quat=[float(v) for v in virt.get("quat").split()],      # (normalised by the loader)
                               joints=[f"{side}_joint{i}" for i in range(1, 8)],
                               body_name=f"xarm_{side}_gripper_base_link", offset=0.125, gravity=gravity)
        rows.append(m.row()); names.append(m.joint_names); limits.append(m.limits)
    out = os.path.join(HERE, "xarm7_arm_models.npz")
    np.savez(out, rows=np.array(rows), joint_names=np.array(names), limits=np.array(limits))
    print("wrote", out, np.array(rows).shape)


if __name__ == "__main__":
    main(sys.argv[1])
