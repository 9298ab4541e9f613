#!/usr/bin/env python3
"""URDF -> the rigid-body model of include/lmpc/lmpc_rbd.h (lmpc_rbd_model), as JSON.

    python tools/urdf_to_rbd.py URDF [--legs FL,FR,RL,RR] [--name NAME] [-o OUT.json]

Reads a quadruped's URDF with the standard library's XML parser and lumps every fixed-joint subtree into its moving
ancestor (mass, centre of mass and inertia by the parallel-axis theorem, with a general `rpy` on fixed joints and
on inertial origins), as Pinocchio does when it builds a model from a URDF.  The result has 13 bodies: the trunk
(the root link and everything fixed to it) and hip / thigh / calf of four legs.  `--legs` lists the name prefixes
of the legs' joints in the library's order FL, FR, RL, RR (e.g. `LF,RF,LH,RH` for a URDF that names them so).

The model class the library covers, and the only one this tool accepts: four chains of three revolute joints
hanging off the root body, every actuated joint with `rpy="0 0 0"` and the axes x, y, y, and one foot link fixed to
each calf (the link in the calf's fixed subtree whose name contains "foot").  Anything else is refused.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import xml.etree.ElementTree as ET


def _vec(s, n=3):
    v = [float(x) for x in (s or "0 0 0").split()]
    if len(v) != n:
        raise ValueError(f"expected {n} numbers, got {s!r}")
    return v


def _rpy(r, p, y):
    """URDF's fixed-axis roll-pitch-yaw: R = Rz(y) Ry(p) Rx(r)."""
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
            [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
            [-sp, cp * sr, cp * cr]]


def _mm(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _mv(a, v):
    return [sum(a[i][k] * v[k] for k in range(3)) for i in range(3)]


def _tr(a):
    return [[a[j][i] for j in range(3)] for i in range(3)]


_EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def _origin(el):
    o = el.find("origin") if el is not None else None
    if o is None:
        return _EYE, [0.0, 0.0, 0.0]
    return _rpy(*_vec(o.get("rpy"))), _vec(o.get("xyz"))


class ModelError(ValueError):
    pass


def lump(parts):
    """parts: (mass, com[3], inertia 3x3 about that com), all in one frame -> the same for their union."""
    m = sum(p[0] for p in parts)
    if m <= 0.0:
        raise ModelError("a body without mass")
    com = [sum(p[0] * p[1][i] for p in parts) / m for i in range(3)]
    inertia = [[0.0] * 3 for _ in range(3)]
    for pm, pc, pi in parts:
        d = [pc[i] - com[i] for i in range(3)]
        d2 = sum(x * x for x in d)
        for i in range(3):
            for j in range(3):
                inertia[i][j] += pi[i][j] + pm * ((d2 if i == j else 0.0) - d[i] * d[j])
    return m, com, inertia


def convert(urdf_text: str, legs=("FL", "FR", "RL", "RR"), name=None) -> dict:
    robot = ET.fromstring(urdf_text)
    links = {l.get("name"): l for l in robot.findall("link")}
    children = {n: [] for n in links}
    has_parent = set()
    for j in robot.findall("joint"):
        parent, child = j.find("parent").get("link"), j.find("child").get("link")
        if parent not in links or child not in links:
            raise ModelError(f"joint {j.get('name')}: unknown link")
        children[parent].append((j, child))
        has_parent.add(child)
    roots = [n for n in links if n not in has_parent]
    if len(roots) != 1:
        raise ModelError(f"expected one root link, found {roots}")

    def collect(link, R, p, parts, moving, feet):
        """Everything fixed to `link` (whose frame is (R, p) in the body frame) into `parts`; the moving joints that
        leave the body into `moving` with their origins in the body frame."""
        inert = links[link].find("inertial")
        if inert is not None:
            Ri, ci = _origin(inert)
            mass = float(inert.find("mass").get("value"))
            t = inert.find("inertia")
            g = lambda k: float(t.get(k, "0"))
            I = [[g("ixx"), g("ixy"), g("ixz")], [g("ixy"), g("iyy"), g("iyz")], [g("ixz"), g("iyz"), g("izz")]]
            Rb = _mm(R, Ri)
            com = [p[i] + _mv(R, ci)[i] for i in range(3)]
            if mass > 0.0:
                parts.append((mass, com, _mm(_mm(Rb, I), _tr(Rb))))
        if "foot" in link.lower():
            feet.append((link, p))
        for j, child in children[link]:
            Rj, pj = _origin(j)
            pc = [p[i] + _mv(R, pj)[i] for i in range(3)]
            if j.get("type") == "fixed":
                collect(child, _mm(R, Rj), pc, parts, moving, feet)
            else:
                moving.append((j, child, _mm(R, Rj), pc))

    def body(link):
        parts, moving, feet = [], [], []
        collect(link, _EYE, [0.0, 0.0, 0.0], parts, moving, feet)
        return lump(parts), moving, feet

    def check_joint(j, R, axis):
        if j.get("type") not in ("revolute", "continuous"):
            raise ModelError(f"joint {j.get('name')}: type {j.get('type')}, expected revolute")
        if any(abs(R[i][k] - _EYE[i][k]) > 0.0 for i in range(3) for k in range(3)):
            raise ModelError(f"joint {j.get('name')}: a rotated joint frame (rpy != 0) is outside the model class")
        a = _vec(j.find("axis").get("xyz")) if j.find("axis") is not None else [1.0, 0.0, 0.0]
        if a != axis:
            raise ModelError(f"joint {j.get('name')}: axis {a}, expected {axis}")

    trunk, hips, trunk_feet = body(roots[0])
    if len(hips) != 4 or trunk_feet:
        raise ModelError(f"expected four legs on the root body, found {len(hips)} moving joints")
    order = []
    for leg in legs:
        hit = [h for h in hips if h[0].get("name").startswith(leg + "_")]
        if len(hit) != 1:
            raise ModelError(f"leg prefix {leg!r} matches {len(hit)} hip joints")
        order.append(hit[0])
    if len({id(h[0]) for h in order}) != 4:
        raise ModelError("--legs must name four different legs")
    bodies, origins, feet, lower, upper = [trunk], [], [], [], []
    for hip in order:
        j, link, R, p = hip
        for k, axis in enumerate(([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])):
            check_joint(j, R, axis)
            lim = j.find("limit")
            lower.append(float(lim.get("lower")) if lim is not None and lim.get("lower") else -math.pi)
            upper.append(float(lim.get("upper")) if lim is not None and lim.get("upper") else math.pi)
            origins.append(p)
            b, moving, ft = body(link)
            bodies.append(b)
            if k < 2:
                if len(moving) != 1 or ft:
                    raise ModelError(f"link {link}: expected one moving child joint and no foot")
                j, link, R, p = moving[0]
            else:
                if moving or len(ft) != 1:
                    raise ModelError(f"link {link}: expected no moving child and one foot link, found {len(ft)}")
                feet.append(ft[0][1])
    sym = lambda I: [I[0][0], I[0][1], I[0][2], I[1][1], I[1][2], I[2][2]]
    return {
        "name": name or robot.get("name"),
        "legs": list(legs),
        "gravity": 9.81,
        "mass": [b[0] for b in bodies],
        "com": [b[1] for b in bodies],
        "inertia": [sym(b[2]) for b in bodies],
        "joint_origin": origins,
        "foot": feet,
        "joint_lower": lower,
        "joint_upper": upper,
    }


def dumps(model: dict) -> str:
    """One key per line, numbers with repr (round-trip exact)."""
    return "{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in model.items()) + "\n}\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("urdf")
    ap.add_argument("--legs", default="FL,FR,RL,RR", help="joint-name prefixes of the legs in the order FL,FR,RL,RR")
    ap.add_argument("--name", default=None)
    ap.add_argument("-o", "--output", default=None)
    a = ap.parse_args(argv)
    try:
        model = convert(open(a.urdf).read(), tuple(a.legs.split(",")), a.name)
    except ModelError as e:
        print(f"urdf_to_rbd: {a.urdf}: {e}", file=sys.stderr)
        return 2
    text = dumps(model)
    if a.output:
        open(a.output, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
