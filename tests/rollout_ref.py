"""NumPy restatement of one closed-loop MPC tick (TEST INFRASTRUCTURE ONLY): the independent checker of
include/lmpc/lmpc_rollout.h.  Written from the reference's lines (relative to src/legged_ctrl), on oracle/fsm.py's
LegFSM and the oracle's own A / B matrices and exact QP solve -- not from csrc/lmpc_common.h:

    ConvexMpc::update / foot_update        src/mpc_ctrl/convex_mpc/ConvexMpc.cpp:24-108
    LeggedContactFSM foot bookkeeping      src/utils/LeggedContactFSM.cpp:38-84,231-254
    BezierUtils                            src/utils/Utils.cpp:136-192
    Raibert foothold                       src/interfaces/BaseInterface.cpp:358-399
    the plant = the QP's stage-0 row       src/mpc_ctrl/convex_mpc/ConvexQPSolver.cpp:198-228,294-297
    calc_mpc_reference                     src/mpc_ctrl/convex_mpc/ConvexQPSolver.cpp:254-313
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from oracle import fsm as F
from oracle import oracle as O

GO1_FEET = np.array([[0.17, 0.12, -0.3], [0.17, -0.17, -0.3], [-0.17, 0.17, -0.3], [-0.17, -0.12, -0.3]])
CLEARANCE1, CLEARANCE2 = 0.0, float(np.float32(0.23))  # LeggedParams.h:26-27 (floats)
DELTA_LIMIT = (0.8, 0.8)                               # LeggedParams.h:29-30


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def rot_zyx(e):
    cr, sr, cp, sp, cy, sy = math.cos(e[0]), math.sin(e[0]), math.cos(e[1]), math.sin(e[1]), math.cos(e[2]), math.sin(e[2])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def bezier(t, P):  # Utils.cpp:179-192
    y = 0.0
    for i, c in enumerate((1, 4, 6, 4, 1)):
        y += c * t ** i * (1 - t) ** (4 - i) * P[i]
    return y


def foot_curve(t, start, final):  # Utils.cpp:136-176; t arrives as a float
    t = float(np.float32(t))
    out = np.zeros(3)
    for a in range(3):
        P = [start[a], start[a], final[a], final[a], final[a]]
        if a == 2:
            P[1] += CLEARANCE1
            P[2] += CLEARANCE2 + 0.5 * math.sin(0.0)
        out[a] = bezier(t, P)
    return out


class RefRobot:
    """One robot of the restated loop.  x = [euler, pos, omega, v]."""

    def __init__(self, x0, vel_d, yaw_rate, height, gait, speed, feet=GO1_FEET, ground_z=0.0):
        self.x = np.array(x0, dtype=np.float64)
        self.vel_d = np.array([vel_d[0], vel_d[1], 0.0])
        self.yaw_rate, self.height, self.gait, self.speed = float(yaw_rate), float(height), int(gait), float(speed)
        self.feet_rel, self.ground_z = np.array(feet, dtype=np.float64), float(ground_z)
        self.euler_d = np.array([0.0, 0.0, self.x[2]])
        self.fsm = [F.LegFSM(gait, j, speed) for j in range(4)]
        c, s = math.cos(self.x[2]), math.sin(self.x[2])
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        self.foot_world = (Rz @ self.feet_rel.T).T + self.x[3:6]
        self.foot_world[:, 2] = self.ground_z
        self.swing_start = self.foot_world.copy()
        self.contacts = [f.s for f in self.fsm]
        self.target = np.zeros((4, 3))
        self.R = rot_zyx(self.x[0:3])

    def raibert(self):  # BaseInterface.cpp:358-399
        c, s = math.cos(self.x[2]), math.sin(self.x[2])
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        v = self.x[9:12].copy()
        v[2] = 0
        vd = Rz @ self.vel_d
        tgt = (Rz @ self.feet_rel.T).T
        k = math.sqrt(abs(self.x[5]) / 9.8)
        for a in range(2):
            d = k * (v[a] - vd[a]) + (1.0 / self.speed / 2.0) / 2.0 * vd[a]
            d = min(max(d, -DELTA_LIMIT[a]), DELTA_LIMIT[a])
            tgt[:, a] += d
        return tgt + self.x[3:6]

    def bookkeep(self, dt):
        self.target = self.raibert()
        self.euler_d[2] += self.yaw_rate * dt  # ConvexMpc.cpp:38
        if self.gait == F.STAND:  # movement mode 0, ConvexMpc.cpp:86-92
            for f in self.fsm:
                f.reset()
            self.contacts = [1, 1, 1, 1]
        else:
            for j, f in enumerate(self.fsm):
                was = f.s
                f.update(dt, False)
                if was == F.STANCE and f.s == F.SWING:  # swing_enter, :231-235
                    self.swing_start[j] = self.foot_world[j]
                if was == F.SWING and f.s == F.STANCE:  # stance_enter: the plant lands the foot on the target
                    self.foot_world[j] = [self.target[j, 0], self.target[j, 1], self.ground_z]
                if f.s == F.SWING:  # swing_update, :242-254
                    self.foot_world[j] = foot_curve(f.percent_in_state(), self.swing_start[j], self.target[j])
            self.contacts = [f.s for f in self.fsm]
        self.R = rot_zyx(self.x[0:3])

    def record(self, H, dt):  # calc_mpc_reference, ConvexQPSolver.cpp:254-313 and :329-346
        rec = np.zeros(33 + 12 * H)
        rec[0:12] = self.x
        rec[12:21] = self.R.reshape(9)
        rec[21:33] = (self.foot_world - self.x[3:6]).reshape(12)
        vdw = self.R @ self.vel_d
        for i in range(H):
            rec[33 + 12 * i:45 + 12 * i] = [self.euler_d[0], self.euler_d[1], self.x[2] + self.yaw_rate * dt * i,
                                            self.x[3] + vdw[0] * dt * i, self.x[4] + vdw[1] * dt * i, self.height,
                                            0.0, 0.0, self.yaw_rate, vdw[0], vdw[1], 0.0]
        con = np.zeros((H, 4), dtype=np.uint8)
        con[0] = self.contacts
        for i in range(1, H):
            con[i] = [f.predict_contact_state(i * dt) for f in self.fsm]
        return rec, con

    def plant(self, op, u0):
        self.x = plant_step(op, self.x, self.R, self.foot_world - self.x[3:6], u0)


def plant_step(op, x, R, feet_abs, u0):
    """x+ = A(yaw) x + B u0 - g dt e11 with the oracle's matrices (ConvexQPSolver.cpp:198-228,294-297)."""
    A, B = np.zeros(144), np.zeros(144)
    O.lib().oracle_update_A(op.dt, float(x[2]), _dp(A))
    Rc = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    fc = np.ascontiguousarray(feet_abs, dtype=np.float64).reshape(12)
    O.lib().oracle_update_B(ctypes.byref(op), _dp(Rc), _dp(fc), _dp(B))
    xn = A.reshape(12, 12) @ np.asarray(x, dtype=np.float64) + B.reshape(12, 12) @ np.asarray(u0, dtype=np.float64)
    xn[11] -= op.gravity * op.dt
    return xn


def run(op, H, robots, ticks, rng=None, eps=0.0):
    """The restated loop with the oracle's exact solve -> x [ticks, B, 12] after each plant step, u0 [ticks, B, 12].
    eps > 0: every u_0 perturbed by a relative eps, uniform in +-eps per component (rng)."""
    xs = np.zeros((ticks, len(robots), 12))
    us = np.zeros((ticks, len(robots), 12))
    for t in range(ticks):
        for b, r in enumerate(robots):
            r.bookkeep(op.dt)
            rec, con = r.record(H, op.dt)
            grf, _, _ = O.solve(op, H, rec, con)
            u0 = grf[0].copy()
            if eps:
                u0 *= 1.0 + rng.uniform(-eps, eps, 12)
            r.plant(op, u0)
            xs[t, b], us[t, b] = r.x, u0
    return xs, us


# The robots of the end-to-end fixture (tests/golden/make_rollout_golden.py, tests/test_gpu_rollout.py test 6):
# x0 = standing at 0.30; (vx, vy, yaw rate); Go1, trot, gait speed 4.0
GOLDEN_ROBOTS = [((0.5, 0.1), 0.3), ((0.3, 0.0), 0.0), ((-0.2, 0.15), -0.2), ((0.0, 0.0), 0.4)]
GOLDEN_TICKS, GOLDEN_H = 60, 10


def golden_robots():
    x0 = np.zeros(12)
    x0[5] = 0.30
    return [RefRobot(x0, vd, yr, 0.30, F.TROT, 4.0) for vd, yr in GOLDEN_ROBOTS]
