"""Arm model table of the device dynamics (``dart_arm_dynamics_batch``): one fp64 row per serial hinge chain.

Row layout (``dart_arm_model_len(n) = 22 n + 18``, include/dart_mpc.h)::

    base_pos[3] base_quat[4]            world pose of the frame the first link hangs in
    per link i: pos[3] quat[4]          body frame in its parent's frame (MJCF body pos / quat, quat normalised)
                axis[3]                 joint axis in the body frame, through the body origin
                armature damping        added to M[i][i]; plant only
                mass com[3] inertia[6]  inertia about the com in the body frame: xx yy zz xy xz yz
    ee_pos[3] ee_quat[4]                frame of ``body_name`` in the last link's frame
    offset                              along that frame's z
    gravity[3]

``ArmModel.from_mjcf`` is a small ``xml.etree`` loader for exactly this case: nested ``<body pos quat>``,
``<inertial pos quat mass diaginertia>``, hinge joints through the body origin whose ``axis`` / ``armature`` / ``damping`` /
``range`` come through ``<default class>`` nesting and ``childclass``.  Bodies without one of the named joints are rigid
parts of the link above them (their own hinge joints, such as a gripper's fingers, are held at 0): everything rigidly
below a joint is composed into that link's mass, com and inertia.  ``<include>`` is not followed -- the caller names the
files.  Anything else in the subtree raises ``DartMPCError`` naming the element.
"""
from __future__ import annotations

import xml.etree.ElementTree as ET

import numpy as np

from ._lib import DartMPCError

LINK_LEN = 22
NMAX = 8


def model_len(n: int) -> int:
    return LINK_LEN * n + 18


def _unit(v, what):
    v = np.asarray(v, dtype=np.float64)
    nv = float(np.linalg.norm(v))
    if not np.isfinite(nv) or nv == 0.0:
        raise DartMPCError(f"{what} must be a non-zero finite vector")
    return v / nv


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) quaternions."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def quat_mat(q):
    """Rotation matrix of a unit (w, x, y, z) quaternion."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _sym6(I):
    return np.array([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])


def sym6_mat(v):
    return np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])


class ArmModel:
    """A serial chain of ``n`` hinge joints; ``row()`` is the model row of the device entries."""

    def __init__(self, base_pos, base_quat, pos, quat, axis, armature, damping, mass, com, inertia, ee_pos, ee_quat,
                 offset, gravity, joint_names=None, limits=None):
        self.n = n = int(np.shape(mass)[0])
        if not 1 <= n <= NMAX:
            raise DartMPCError(f"an arm model has 1..{NMAX} joints, not {n}")

        def arr(v, shape, what):
            v = np.array(v, dtype=np.float64)
            if v.shape != shape:
                raise DartMPCError(f"{what} must have shape {shape}, not {v.shape}")
            return v
        self.base_pos = arr(base_pos, (3,), "base_pos")
        self.base_quat = _unit(arr(base_quat, (4,), "base_quat"), "base_quat")
        self.pos = arr(pos, (n, 3), "pos")
        self.quat = np.array([_unit(v, "quat") for v in arr(quat, (n, 4), "quat")])
        self.axis = np.array([_unit(v, "axis") for v in arr(axis, (n, 3), "axis")])
        self.armature = arr(armature, (n,), "armature")
        self.damping = arr(damping, (n,), "damping")
        self.mass = arr(mass, (n,), "mass")
        self.com = arr(com, (n, 3), "com")
        self.inertia = arr(inertia, (n, 6), "inertia")
        self.ee_pos = arr(ee_pos, (3,), "ee_pos")
        self.ee_quat = _unit(arr(ee_quat, (4,), "ee_quat"), "ee_quat")
        self.offset = float(offset)
        self.gravity = arr(gravity, (3,), "gravity")
        self.joint_names = list(joint_names) if joint_names is not None else [f"joint{i + 1}" for i in range(n)]
        self.limits = None if limits is None else arr(limits, (n, 2), "limits")

    @classmethod
    def from_arrays(cls, **fields):
        """The constructor by keyword: base_pos, base_quat, pos [n, 3], quat [n, 4], axis [n, 3], armature [n], damping [n],
        mass [n], com [n, 3], inertia [n, 6], ee_pos, ee_quat, offset, gravity (joint_names, limits optional)."""
        return cls(**fields)

    @classmethod
    def from_row(cls, row, n, **extra):
        row = np.asarray(row, dtype=np.float64)
        if row.shape != (model_len(n),):
            raise DartMPCError(f"a model row of {n} joints has {model_len(n)} entries")
        L = row[7:7 + LINK_LEN * n].reshape(n, LINK_LEN)
        e = row[7 + LINK_LEN * n:]
        return cls(row[:3], row[3:7], L[:, 0:3], L[:, 3:7], L[:, 7:10], L[:, 10], L[:, 11], L[:, 12], L[:, 13:16],
                   L[:, 16:22], e[0:3], e[3:7], e[7], e[8:11], **extra)

    def row(self) -> np.ndarray:
        L = np.concatenate([self.pos, self.quat, self.axis, self.armature[:, None], self.damping[:, None],
                            self.mass[:, None], self.com, self.inertia], axis=1)
        return np.ascontiguousarray(np.concatenate([self.base_pos, self.base_quat, L.ravel(), self.ee_pos, self.ee_quat,
                                                    [self.offset], self.gravity]))

    def with_payload(self, mass, com=None):
        """A copy with a point mass added to the last link at ``com`` (last link's frame; default: the EE frame origin)."""
        c1 = self.ee_pos if com is None else np.asarray(com, dtype=np.float64)
        m0, c0, I0 = self.mass[-1], self.com[-1], sym6_mat(self.inertia[-1])
        m = m0 + mass
        c = (m0 * c0 + mass * c1) / m
        I = I0 + m0 * _shift(c0 - c) + mass * _shift(c1 - c)
        out = ArmModel.from_row(self.row(), self.n, joint_names=self.joint_names, limits=self.limits)
        out.mass[-1], out.com[-1], out.inertia[-1] = m, c, _sym6(I)
        return out

    # ---- MJCF --------------------------------------------------------------------------------------------------
    @classmethod
    def from_mjcf(cls, chain_xml, defaults_xml, base_pos, base_quat, joints, body_name, offset, gravity):
        """chain_xml: file (or XML text) whose first ``<body>`` is the chain's root; defaults_xml: file (or text) holding
        the ``<default>`` tree (None: no defaults).  base_pos / base_quat: world pose of the frame the root body hangs in.
        joints: the n joint names from the base outwards; body_name: the EE body, rigidly below the last joint."""
        root = _parse(chain_xml)
        top = root if root.tag == "body" else root.find(".//body")
        if top is None:
            raise DartMPCError("no <body> in the chain file")
        defaults = _Defaults(_parse(defaults_xml) if defaults_xml is not None else None)
        joints = list(joints)
        n = len(joints)
        if not 1 <= n <= NMAX:
            raise DartMPCError(f"an arm model has 1..{NMAX} joints, not {n}")
        links = []          # per link: dict(pos, quat, axis, armature, damping, limits, parts=[(m, com, I)])
        state = {"ee": None}

        def walk(body, childclass, link, p_rel, q_rel):
            """body's frame in the current link (or, before the first joint, in the world) is (p_rel, q_rel)."""
            for k in body.attrib:
                if k not in ("name", "pos", "quat", "childclass"):
                    raise DartMPCError(f"unsupported attribute {k!r} on <body name={body.get('name')!r}>")
            childclass = body.get("childclass", childclass)
            bp = _floats(body.get("pos", "0 0 0"), 3, body)
            bq = _unit(_floats(body.get("quat", "1 0 0 0"), 4, body), "body quat")
            p = p_rel + quat_mat(q_rel) @ bp
            q = quat_mul(q_rel, bq)
            named = None
            for j in body.findall("joint"):
                ja = defaults.resolve("joint", j, childclass)
                if ja.get("type", "hinge") != "hinge":
                    raise DartMPCError(f"unsupported joint type {ja['type']!r} on <joint name={j.get('name')!r}>")
                if "pos" in ja:
                    raise DartMPCError(f"unsupported attribute 'pos' on <joint name={j.get('name')!r}>")
                if j.get("name") in joints:
                    if named is not None:
                        raise DartMPCError(f"two chain joints on <body name={body.get('name')!r}>")
                    named = (j.get("name"), ja)
            for el in body:
                if el.tag not in ("body", "joint", "inertial", "geom", "site"):
                    raise DartMPCError(f"unsupported element <{el.tag}> in <body name={body.get('name')!r}>")
            if named is not None:
                name, ja = named
                if len(links) >= n or joints[len(links)] != name or link != len(links) - 1:
                    raise DartMPCError(f"joint {name!r} is not the next joint of a serial chain {joints}")
                links.append({"pos": p, "quat": q, "axis": _unit(_floats(ja.get("axis", "0 0 1"), 3, body), "axis"),
                              "armature": float(ja.get("armature", 0.0)), "damping": float(ja.get("damping", 0.0)),
                              "limits": _floats(ja.get("range", "-inf inf"), 2, body), "parts": []})
                link = len(links) - 1
                p, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
            inertial = body.find("inertial")
            if inertial is not None and link >= 0:
                for k in inertial.attrib:
                    if k not in ("pos", "quat", "mass", "diaginertia"):
                        raise DartMPCError(f"unsupported attribute {k!r} on <inertial> of <body name={body.get('name')!r}>")
                Rb = quat_mat(q)
                Ri = Rb @ quat_mat(_unit(_floats(inertial.get("quat", "1 0 0 0"), 4, body), "inertial quat"))
                d = _floats(inertial.get("diaginertia"), 3, body)
                links[link]["parts"].append((float(inertial.get("mass")), p + Rb @ _floats(inertial.get("pos"), 3, body),
                                             Ri @ np.diag(d) @ Ri.T))
            elif inertial is None and link >= 0 and body.find("geom") is not None:
                raise DartMPCError(f"<body name={body.get('name')!r}> has geoms but no <inertial>")
            if body.get("name") == body_name:
                if link != n - 1:
                    raise DartMPCError(f"body {body_name!r} is not rigidly below the last joint {joints[-1]!r}")
                state["ee"] = (p, q)
            for child in body.findall("body"):
                walk(child, childclass, link, p, q)

        # (bodies above the first joint are fixed to the world: their frames compose into the base pose)
        walk(top, None, -1, np.array(base_pos, dtype=np.float64), _unit(base_quat, "base_quat"))
        if len(links) != n:
            raise DartMPCError(f"joints {joints[len(links):]} not found in the chain")
        if state["ee"] is None:
            raise DartMPCError(f"body {body_name!r} not found in the chain")
        mass, com, inertia = [], [], []
        for i, lk in enumerate(links):
            if not lk["parts"]:
                raise DartMPCError(f"link of joint {joints[i]!r} has no <inertial>")
            m = sum(pt[0] for pt in lk["parts"])
            c = sum(pt[0] * pt[1] for pt in lk["parts"]) / m
            I = sum(pt[2] + pt[0] * _shift(pt[1] - c) for pt in lk["parts"])
            mass.append(m); com.append(c); inertia.append(_sym6(I))
        return cls(links[0]["pos"], links[0]["quat"], [np.zeros(3)] + [lk["pos"] for lk in links[1:]],
                   [[1.0, 0, 0, 0]] + [lk["quat"] for lk in links[1:]], [lk["axis"] for lk in links],
                   [lk["armature"] for lk in links], [lk["damping"] for lk in links], mass, com, inertia,
                   state["ee"][0], state["ee"][1], offset, gravity, joint_names=joints,
                   limits=[lk["limits"] for lk in links])


def _shift(d):
    """Parallel-axis term of a unit mass displaced by d: |d|^2 E - d d'."""
    return float(d @ d) * np.eye(3) - np.outer(d, d)


def _parse(src):
    try:
        if isinstance(src, str) and src.lstrip().startswith("<"):
            return ET.fromstring(src)
        return ET.parse(src).getroot()
    except ET.ParseError as e:
        raise DartMPCError(f"cannot parse {src!r}: {e}") from None


def _floats(text, count, el):
    try:
        v = np.array([float(t) for t in str(text).split()])
    except ValueError:
        v = np.zeros(0)
    if v.shape != (count,):
        raise DartMPCError(f"expected {count} numbers, got {text!r} in <{el.tag} name={el.get('name')!r}>")
    return v


class _Defaults:
    """``<default class>`` nesting: a class inherits its parent's attributes element by element."""

    def __init__(self, root):
        self.classes = {}
        if root is None:
            return
        top = root if root.tag == "default" else root.find("default")
        if top is not None:
            self._collect(top, {})

    def _collect(self, node, inherited):
        mine = {tag: dict(attrs) for tag, attrs in inherited.items()}
        for el in node:
            if el.tag != "default":
                mine.setdefault(el.tag, {}).update(el.attrib)
        self.classes[node.get("class", "main")] = mine
        for el in node.findall("default"):
            self._collect(el, mine)

    def resolve(self, tag, el, childclass):
        cname = el.get("class", childclass or "main")
        if cname not in self.classes and cname != "main":
            raise DartMPCError(f"unknown default class {cname!r} on <{tag} name={el.get('name')!r}>")
        out = dict(self.classes.get(cname, {}).get(tag, {}))
        out.update({k: v for k, v in el.attrib.items() if k not in ("class", "name")})
        return out
