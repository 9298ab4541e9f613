"""NumPy restatement of the full loop's MPC tick (TEST INFRASTRUCTURE ONLY): the independent checker of
include/lmpc/lmpc_stack.h.  Written from the reference's lines (relative to src/legged_ctrl), on oracle/fsm.py's LegFSM
(which has the early-touchdown branch) and rollout_ref's foot_curve / rot_zyx / Raibert target -- not from
csrc/lmpc_stack_common.h:

    ConvexMpc::update / foot_update        src/mpc_ctrl/convex_mpc/ConvexMpc.cpp:24-108
    LeggedContactFSM::update, in full      src/utils/LeggedContactFSM.cpp:16-84,214-254
    BezierUtils                            src/utils/Utils.cpp:136-192
    Raibert foothold                       src/interfaces/BaseInterface.cpp:358-399
    measured_rbd_state                     src/interfaces/BaseInterface.cpp:511-518 (read backwards)
"""
from __future__ import annotations

import numpy as np

from oracle import fsm as F
from rollout_ref import GO1_FEET, RefRobot, foot_curve, rot_zyx


class FootFSM(F.LegFSM):
    """LegFSM plus the foot bookkeeping of LeggedContactFSM (LeggedContactFSM.cpp:16-84,231-254)."""

    def __init__(self, gait, leg, speed):
        super().__init__(gait, leg, speed)
        self.swing_start = np.zeros(3)
        self.swing_end = np.zeros(3)
        self.pos_target = np.zeros(3)
        self.vel_target = np.zeros(3)
        self.not_first_call = False
        self.early = 0      # swings ended by the contact flag
        self.timed_out = 0  # swings ended at percent_in_state() >= 1

    def reset(self):  # :16-36
        if getattr(self, "s", F.STANCE) == F.SWING and hasattr(self, "swing_end"):
            self.pos_target = self.swing_end.copy()
            self.vel_target = np.zeros(3)
        super().reset()
        self.not_first_call = False

    def update_feet(self, dt, foot_cur, foot_target, flag):  # :38-84
        foot_cur, foot_target = np.array(foot_cur, dtype=np.float64), np.array(foot_target, dtype=np.float64)
        if not self.not_first_call:
            self.swing_start = foot_cur.copy()
            self.swing_end = foot_target.copy()
            self.pos_target = foot_target.copy()
            self.vel_target = np.zeros(3)
            self.not_first_call = True
        was = self.s
        before = None
        if was == F.SWING:  # which branch will end the swing, if any (evaluated at the advanced phase, as :56-67)
            ph = self.phase + self.speed * dt
            pc = min(max((ph - self.start) / (self.end - self.start), 0.0), 1.0)
            before = "early" if (pc > 0.9 and flag) else ("timeout" if pc >= 1.0 else None)
        self.update(dt, bool(flag))
        if was == F.STANCE and self.s == F.SWING:  # swing_enter, :231-235
            self.swing_start = foot_cur.copy()
        if was == F.SWING and self.s == F.STANCE:  # stance_enter, :236-240
            self.pos_target = foot_cur.copy()
            self.vel_target = np.zeros(3)
            if before == "early":
                self.early += 1
            else:
                self.timed_out += 1
        if self.s == F.SWING:  # swing_update, :242-254
            new = foot_curve(self.percent_in_state(), self.swing_start, foot_target)
            self.swing_end = foot_target.copy()
            prev = self.pos_target
            self.pos_target = new
            self.vel_target = (new - prev) / dt


class StackRef(RefRobot):
    """One robot's MPC side of the full loop.  `state`: the 36 doubles of lmpc_rbd_state."""

    def __init__(self, state, vel_d, yaw_rate, height, gait, speed, feet=GO1_FEET):
        state = np.asarray(state, dtype=np.float64)
        super().__init__(self.x_of(state), vel_d, yaw_rate, height, gait, speed, feet=feet)
        self.fsm = [FootFSM(gait, j, speed) for j in range(4)]
        self.contacts = [f.s for f in self.fsm]
        self.tick = 0

    @staticmethod
    def x_of(state):
        """[roll, pitch, yaw, pos, omega_world, v_world] from [yaw, pitch, roll, pos, joints, omega, v, joint rates]."""
        return np.concatenate([state[0:3][::-1], state[3:6], state[18:21], state[21:24]])

    def advance(self, state, foot_pos, touch, dt):
        state = np.asarray(state, dtype=np.float64)
        self.x = self.x_of(state)
        self.foot_world = np.array(foot_pos, dtype=np.float64).reshape(4, 3)
        self.target = self.raibert()
        self.euler_d[2] += self.yaw_rate * dt  # ConvexMpc.cpp:38
        if self.gait == F.STAND:  # movement mode 0, ConvexMpc.cpp:86-92
            for j, f in enumerate(self.fsm):
                f.reset()
                # the library's choice (lmpc_stack.h): the targets follow the measured feet
                f.pos_target = self.foot_world[j].copy()
                f.vel_target = np.zeros(3)
            self.contacts = [1, 1, 1, 1]
        else:
            for j, f in enumerate(self.fsm):
                f.update_feet(dt, self.foot_world[j], self.target[j], bool(touch[j]))
            self.contacts = [f.s for f in self.fsm]
        self.R = rot_zyx(self.x[0:3])
        self.foot_abs = self.foot_world - self.x[3:6]
        self.tick += 1

    def wbc_targets(self, u0):
        """(forces_des, foot_pos_des, foot_vel_des, contact) -- ConvexMpc.cpp:54-56."""
        return (np.asarray(u0, dtype=np.float64).copy(), np.concatenate([f.pos_target for f in self.fsm]),
                np.concatenate([f.vel_target for f in self.fsm]), list(self.contacts))


def synthetic_feedback(rng, ticks, base_state, p_touch=0.5):
    """A smooth random trajectory of lmpc_rbd_state (36 doubles) and of the four measured feet around `base_state`, and
    touch flags drawn with probability p_touch per tick and leg (as oracle.fsm.random_walk draws its contacts), so that
    early touchdowns occur -> states [ticks, 36], feet [ticks, 12], touch [ticks, 4]."""
    t = np.arange(ticks)[:, None] * 0.01
    amp = np.concatenate([[0.3, 0.15, 0.15], [0.2, 0.2, 0.03], np.full(12, 0.2), [0.5, 0.5, 0.5], [0.4, 0.4, 0.2],
                          np.full(12, 1.0)])
    w = rng.uniform(2.0, 9.0, 36)
    ph = rng.uniform(0.0, 2 * np.pi, 36)
    states = np.asarray(base_state, dtype=np.float64)[None, :] + amp[None, :] * np.sin(w[None, :] * t + ph[None, :])
    fw, fph = rng.uniform(2.0, 9.0, 12), rng.uniform(0.0, 2 * np.pi, 12)
    base_feet = (GO1_FEET + np.asarray(base_state[3:6])).reshape(12)
    feet = base_feet[None, :] + 0.05 * np.sin(fw[None, :] * t + fph[None, :])
    touch = (rng.random((ticks, 4)) < p_touch).astype(np.int32)
    return states, feet, touch
