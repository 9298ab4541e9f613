"""Independent NumPy reference for the rigid-body dynamics of include/lmpc/lmpc_rbd.h (test helper, not a test).

It shares no algorithm with the product (composite rigid bodies + recursive Newton-Euler in world axes):

  * forward kinematics by explicit rotation matrices, complex-safe;
  * M = sum_b m_b Jv_b' Jv_b + Jw_b' (R_b I_b R_b') Jw_b from geometric body Jacobians;
  * h = Mdot v - 1/2 grad_q (v' M v) + grad_q V (Lagrange's equations in the holonomic coordinates q), with the
    derivatives of M(q) and of the potential V(q) by complex-step differentiation (step 1e-30: exact to rounding);
  * J = d p_foot / d q by complex step; dJv = d/dt (J(q + t v) v) by complex step of the geometric foot Jacobian;
  * Ab from the bodies' momenta; base_accel and swing_acc from the header's formulas with a general 6 x 6 solve.

Coordinates: q = [pos, yaw, pitch, roll, joints], v = [lin_vel_world, euler rates, joint_vel], R = Rz Ry Rx.
`model` is a dict as tools/urdf_to_rbd.py writes it (tests/golden/rbd_model_*.json).
"""
from __future__ import annotations

import numpy as np

EPS = 1e-30
AXES = (0, 1, 1)  # hip about x, thigh and calf about y


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    one, zero = c * 0 + 1, c * 0
    if axis == 0:
        return np.array([[one, zero, zero], [zero, c, -s], [zero, s, c]])
    if axis == 1:
        return np.array([[c, zero, s], [zero, one, zero], [-s, zero, c]])
    return np.array([[c, -s, zero], [s, c, zero], [zero, zero, one]])


def _inertia(six):
    ixx, ixy, ixz, iyy, iyz, izz = six
    return np.array([[ixx, ixy, ixz], [ixy, iyy, iyz], [ixz, iyz, izz]], dtype=np.float64)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _unit(k):
    e = np.zeros(3)
    e[k] = 1.0
    return e


def kinematics(model, q):
    """Per body: (R, origin, com); per foot: position; the joints' world axes and positions (Euler joints first)."""
    q = np.asarray(q)
    Rz, Ry, Rx = _rot(2, q[3]), _rot(1, q[4]), _rot(0, q[5])
    Rb = Rz @ Ry @ Rx
    pb = q[0:3] + 0 * q[3]
    euler_axes = [_unit(2) + 0 * q[3], Rz @ _unit(1), Rz @ Ry @ _unit(0)]
    bodies = [(Rb, pb, pb + Rb @ np.asarray(model["com"][0]))]
    feet, joints = [], []
    for leg in range(4):
        R, p = Rb, pb
        for k in range(3):
            j = 3 * leg + k
            p = p + R @ np.asarray(model["joint_origin"][j])
            joints.append((R @ _unit(AXES[k]), p))
            R = R @ _rot(AXES[k], q[6 + j])
            bodies.append((R, p, p + R @ np.asarray(model["com"][1 + j])))
        feet.append(p + R @ np.asarray(model["foot"][leg]))
    return bodies, feet, euler_axes, joints, pb


def _point_jacobian(point, leg, euler_axes, joints, pb, upto=3):
    """3 x 18 Jacobians (linear, angular) of a point fixed to link `upto - 1` of `leg` (leg < 0: the trunk)."""
    dtype = np.result_type(point.dtype, pb.dtype, joints[0][0].dtype)
    Jv, Jw = np.zeros((3, 18), dtype=dtype), np.zeros((3, 18), dtype=dtype)
    Jv[:, 0:3] = np.eye(3)
    for k in range(3):
        Jw[:, 3 + k] = euler_axes[k]
        Jv[:, 3 + k] = _cross(euler_axes[k], point - pb)
    if leg >= 0:
        for k in range(upto):
            a, p = joints[3 * leg + k]
            Jw[:, 6 + 3 * leg + k] = a
            Jv[:, 6 + 3 * leg + k] = _cross(a, point - p)
    return Jv, Jw


def body_jacobians(model, q):
    bodies, feet, ea, joints, pb = kinematics(model, q)
    out = [_point_jacobian(bodies[0][2], -1, ea, joints, pb)]
    for leg in range(4):
        for k in range(3):
            out.append(_point_jacobian(bodies[1 + 3 * leg + k][2], leg, ea, joints, pb, upto=k + 1))
    return bodies, out


def mass_matrix(model, q):
    bodies, jac = body_jacobians(model, q)
    M = 0
    for b, ((R, _, _), (Jv, Jw)) in enumerate(zip(bodies, jac)):
        M = M + model["mass"][b] * (Jv.T @ Jv) + Jw.T @ (R @ _inertia(model["inertia"][b]) @ R.T) @ Jw
    return M


def potential(model, q):
    bodies = kinematics(model, q)[0]
    return sum(model["mass"][b] * model["gravity"] * bodies[b][2][2] for b in range(13))


def foot_positions(model, q):
    return np.concatenate(kinematics(model, q)[1])


def foot_jacobian_geometric(model, q):
    bodies, feet, ea, joints, pb = kinematics(model, q)
    return np.vstack([_point_jacobian(feet[leg], leg, ea, joints, pb)[0] for leg in range(4)])


def euler_map(euler):
    """E: omega_world = E (yaw, pitch, roll) rates."""
    Rz, Ry = _rot(2, euler[0]), _rot(1, euler[1])
    return np.column_stack([_unit(2), Rz @ _unit(1), Rz @ Ry @ _unit(0)])


def q_v_from_state(state):
    """wbc.cpp:49-57 on measured_rbd_state (36)."""
    s = np.asarray(state, dtype=np.float64)
    q = np.concatenate([s[3:6], s[0:3], s[6:18]])
    rates = np.linalg.solve(euler_map(s[0:3]), s[18:21])
    v = np.concatenate([s[21:24], rates, s[24:36]])
    return q, v


def _cstep(f, q, d):
    return np.imag(f(np.asarray(q, dtype=np.complex128) + 1j * EPS * d)) / EPS


def terms(model, state):
    """M, nle, J, dJv, foot_pos, foot_vel, com, Ab, mass for one measured_rbd_state."""
    q, v = q_v_from_state(state)
    I18 = np.eye(18)
    M = np.real(mass_matrix(model, q.astype(np.complex128)))
    Mdot_v = _cstep(lambda x: mass_matrix(model, x), q, v) @ v
    grad_T = np.array([_cstep(lambda x: v @ mass_matrix(model, x) @ v, q, I18[k]) for k in range(18)])
    grad_V = np.array([_cstep(lambda x: potential(model, x), q, I18[k]) for k in range(18)])
    nle = Mdot_v - 0.5 * grad_T + grad_V
    J = np.column_stack([_cstep(lambda x: foot_positions(model, x), q, I18[k]) for k in range(18)])
    dJv = _cstep(lambda x: foot_jacobian_geometric(model, x) @ v, q, v)
    foot_pos = np.real(foot_positions(model, q.astype(np.complex128)))
    # centroidal block from the bodies' momenta under unit base velocities
    bodies, jac = body_jacobians(model, q)
    mass = float(sum(model["mass"]))
    com = sum(model["mass"][b] * bodies[b][2] for b in range(13)) / mass
    Ab = np.zeros((6, 6))
    for b, ((R, _, c), (Jv, Jw)) in enumerate(zip(bodies, jac)):
        lin = model["mass"][b] * Jv[:, :6]
        Ab[0:3] += lin
        Ab[3:6] += np.cross(np.tile((c - com)[:, None], (1, 6)), lin, axis=0) + \
            (R @ _inertia(model["inertia"][b]) @ R.T) @ Jw[:, :6]
    return dict(M=M, nle=nle, J=J, dJv=dJv, foot_pos=foot_pos, foot_vel=J @ v, com=com, Ab=Ab, mass=mass, q=q, v=v,
                grad_V=grad_V)


def wbc_terms(model, state, forces_des, foot_pos_des, foot_vel_des, kp=350.0, kd=37.0):
    """terms() plus base_accel and swing_acc (include/lmpc/lmpc_rbd.h; wbc.cpp:195-203, :239)."""
    t = terms(model, state)
    f = np.asarray(forces_des, dtype=np.float64).reshape(4, 3)
    feet = t["foot_pos"].reshape(4, 3)
    hdot = np.concatenate([f.sum(axis=0) + t["mass"] * np.array([0.0, 0.0, -model["gravity"]]),
                           sum(np.cross(feet[i] - t["com"], f[i]) for i in range(4))])
    Ainv = np.linalg.inv(t["Ab"])
    b = Ainv @ hdot
    w = euler_map(np.asarray(state)[0:3]) @ t["v"][3:6]
    Aww = t["Ab"][3:6, 3:6]
    b[3:6] -= Ainv[3:6, 3:6] @ np.cross(w, Aww @ w)
    t["base_accel"] = b
    t["swing_acc"] = kp * (np.asarray(foot_pos_des, dtype=np.float64).reshape(12) - t["foot_pos"]) + \
        kd * (np.asarray(foot_vel_des, dtype=np.float64).reshape(12) - t["foot_vel"])
    return t
