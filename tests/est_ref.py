"""Independent NumPy restatement of the reference's BasicKF (src/estimation/BasicKF.cpp) and of the sensor model of
include/lmpc/lmpc_est.h (test helper, not a test).

It shares no algorithm with the product: dense A, B, C, Q, R matrices, S = C Pbar C' + R formed in full and the two
solves by np.linalg.solve (LU with partial pivoting), where the product applies 28 scalar updates.  Leg kinematics come
from rbd_ref (explicit rotation matrices, geometric Jacobians), with the base at the origin.

Sensors are dicts of NumPy arrays: imu_acc, imu_ang_vel, euler (yaw, pitch, roll), joint_pos, joint_vel, contact.
"""
from __future__ import annotations

import numpy as np

import rbd_ref as R

NX, NY = 18, 28
DEFAULTS = dict(noise_pimu=0.01, noise_vimu=0.01, noise_pfoot=0.01, noise_pimu_rel_foot=0.001, noise_vimu_rel_foot=0.1,
                noise_zfoot=0.001, gravity=9.81, drift_threshold=1e-6, drift_divisor=10.0, init_P=3.0,
                assume_flat_ground=True)


def rot(euler):
    return R._rot(2, euler[0]) @ R._rot(1, euler[1]) @ R._rot(0, euler[2])


def leg_kinematics(model, joint_pos, joint_vel):
    """fk [4, 3] and J_leg qd [4, 3] in the body frame."""
    q = np.concatenate([np.zeros(6), joint_pos])
    fk = R.foot_positions(model, q).reshape(4, 3)
    J = R.foot_jacobian_geometric(model, q)
    fv = np.stack([J[3 * l:3 * l + 3, 6 + 3 * l:9 + 3 * l] @ joint_vel[3 * l:3 * l + 3] for l in range(4)])
    return fk, fv


def c_matrix():
    C = np.zeros((NY, NX))
    for i in range(4):
        C[3 * i:3 * i + 3, 0:3] = -np.eye(3)
        C[3 * i:3 * i + 3, 6 + 3 * i:9 + 3 * i] = np.eye(3)
        C[12 + 3 * i:15 + 3 * i, 3:6] = np.eye(3)
        C[24 + i, 6 + 3 * i + 2] = 1.0
    return C


def init(model, sensors, pos0=None, cfg=DEFAULTS):
    fk, _ = leg_kinematics(model, sensors["joint_pos"], sensors["joint_vel"])
    Rm = rot(sensors["euler"])
    x = np.zeros(NX)
    x[0:3] = (0.0, 0.0, 0.09) if pos0 is None else pos0
    for l in range(4):
        x[6 + 3 * l:9 + 3 * l] = Rm @ fk[l] + x[0:3]
    return x, cfg["init_P"] * np.eye(NX)


def update(model, sensors, x, P, dt, cfg=DEFAULTS):
    """One BasicKF::update_estimation -> (x, P, det of P[0:2, 0:2] before the drift rule, cond(S))."""
    fk, fv = leg_kinematics(model, sensors["joint_pos"], sensors["joint_vel"])
    Rm = rot(sensors["euler"])
    c = np.asarray(sensors["contact"], dtype=np.float64)
    A, B = np.eye(NX), np.zeros((NX, 3))
    A[0:3, 3:6] = dt * np.eye(3)
    B[3:6, 0:3] = dt * np.eye(3)
    u = Rm @ sensors["imu_acc"] + np.array([0.0, 0.0, -cfg["gravity"]])
    k = 1 + (1 - c) * 1e3
    Q = np.zeros((NX, NX))
    Q[0:3, 0:3] = cfg["noise_pimu"] * dt / 20.0 * np.eye(3)
    Q[3:6, 3:6] = cfg["noise_vimu"] * dt * 9.8 / 20.0 * np.eye(3)
    Rd = np.zeros(NY)
    y = np.zeros(NY)
    for l in range(4):
        Q[6 + 3 * l:9 + 3 * l, 6 + 3 * l:9 + 3 * l] = k[l] * dt * cfg["noise_pfoot"] * np.eye(3)
        Rd[3 * l:3 * l + 3] = k[l] * cfg["noise_pimu_rel_foot"]
        Rd[12 + 3 * l:15 + 3 * l] = k[l] * cfg["noise_vimu_rel_foot"]
        Rd[24 + l] = k[l] * cfg["noise_zfoot"] if cfg["assume_flat_ground"] else 1e5
        y[3 * l:3 * l + 3] = Rm @ fk[l]
        leg_v = -fv[l] - np.cross(sensors["imu_ang_vel"], fk[l])
        y[12 + 3 * l:15 + 3 * l] = (1.0 - c[l]) * x[3:6] + c[l] * (Rm @ leg_v)
        y[24 + l] = (1.0 - c[l]) * (x[2] + fk[l][2])
    C = c_matrix()
    xbar = A @ x + B @ u
    Pbar = A @ P @ A.T + Q
    S = C @ Pbar @ C.T + np.diag(Rd)
    S = 0.5 * (S + S.T)
    err = y - C @ xbar
    xn = xbar + Pbar @ C.T @ np.linalg.solve(S, err)
    Pn = Pbar - Pbar @ C.T @ np.linalg.solve(S, C) @ Pbar
    Pn = 0.5 * (Pn + Pn.T)
    det = Pn[0, 0] * Pn[1, 1] - Pn[0, 1] * Pn[1, 0]
    if det > cfg["drift_threshold"]:
        Pn[0:2, 2:] = 0.0
        Pn[2:, 0:2] = 0.0
        Pn[0:2, 0:2] /= cfg["drift_divisor"]
    return xn, Pn, det, np.linalg.cond(S)


def report(model, sensors, x):
    """state_est (36) and the fields of lmpc_est_out."""
    fk, fv = leg_kinematics(model, sensors["joint_pos"], sensors["joint_vel"])
    Rm = rot(sensors["euler"])
    w = sensors["imu_ang_vel"]
    state = np.concatenate([sensors["euler"], x[0:3], sensors["joint_pos"], Rm @ w, x[3:6], sensors["joint_vel"]])
    world = np.stack([Rm @ fk[l] + x[0:3] for l in range(4)])
    vel = np.stack([Rm @ fv[l] + x[3:6] + Rm @ np.cross(w, fk[l]) for l in range(4)])
    return state, dict(foot_pos_rel=fk.reshape(12), foot_pos_world=world.reshape(12), foot_vel_world=vel.reshape(12),
                       estimated_contacts=(np.asarray(sensors["contact"]) >= 0.5).astype(np.int32))


def sensors_from_plant(model, state, qdd, touch, stand=False):
    """Exact sensors of a plant state (36) with base acceleration qdd[0:3]."""
    s = np.asarray(state, dtype=np.float64)
    Rm = rot(s[0:3])
    return dict(imu_acc=Rm.T @ (np.asarray(qdd[0:3]) + np.array([0.0, 0.0, model["gravity"]])), imu_ang_vel=Rm.T @ s[18:21],
                euler=s[0:3].copy(), joint_pos=s[6:18].copy(), joint_vel=s[24:36].copy(),
                contact=np.ones(4) if stand else (np.asarray(touch) != 0).astype(np.float64))
