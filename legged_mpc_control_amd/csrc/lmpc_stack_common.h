// lmpc_stack_common.h -- the MPC tick of the full loop (include/lmpc/lmpc_stack.h), written once and compiled for the
// host (lmpc_stack_advance, lmpc_stack_targets) and for gfx950 (lmpc_stack.hip's kernels):
//
//   feedback from the measured state      BaseInterface.cpp:511-518 read backwards
//   Raibert foothold                      BaseInterface.cpp:358-399 (lmpc_common.h robot_bookkeep's formulas)
//   LeggedContactFSM::update, in full     LeggedContactFSM.cpp:16-84,214-278 (early touchdown, FSM foot targets)
//   swing Bezier                          Utils.cpp:136-192 (lmpc_common.h swing_bezier)
//   optimized_state / optimized_input     ConvexMpc.cpp:54-56
//
// No FMA contraction (LMPC_NO_FMA) and no HIP runtime call: the host and the device differ only through sin, cos and
// sqrt.  Every loop is unrolled to constant indices, each leg's FSM lives in locals that are stored back once, and the
// gait table is read by selects (leg_tab / tab_end): nothing here needs a private (scratch) array on the device.
#pragma once
#include <cstddef>

#include "lmpc/lmpc_stack.h"
#include "lmpc_common.h"

static_assert(sizeof(lmpc_stack_robot) == 960, "lmpc_stack_robot layout (mirrored by _native.LmpcStackRobot)");
static_assert(sizeof(lmpc_wbc_target) == 352, "lmpc_wbc_target layout");

namespace lmpc_stack {

using lmpc_common::GaitTab;

// One leg's gait table as scalars (size <= 3): a switch time is picked by two two-way selects on values.  On the
// device the first select's result is made opaque: otherwise the compiler merges the two into one pick by a run-time
// index, which it then serves from a table in scratch.
struct LegTab {
    int size;
    double e0, e1, e2;
};
LMPC_HD inline LegTab leg_tab(int gait, int leg) {
    const GaitTab t = lmpc_common::gait_table(gait, leg);
    return LegTab{t.size, t.sw[0], t.sw[1], t.sw[2]};
}
LMPC_HD inline double tab_end(const LegTab& t, int idx) {
    double hi = idx == 1 ? t.e1 : t.e2;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(hi));
#endif
    return idx == 0 ? t.e0 : hi;
}

// common_enter (LeggedContactFSM.cpp:214-229)
LMPC_HD inline void common_enter(const LegTab& t, int& idx, double& phase, double& start) {
    LMPC_NO_FMA
    const int prev = idx;
    idx = idx + 1 < t.size ? idx + 1 : 0;  // (idx + 1) % size for idx < size
    if (idx < prev) phase -= 1.0;
    start = phase;
}

// Steps 1-4 of lmpc_stack.h's advance.  foot_pos[12] / touch[4]: the plant's latest lmpc_sim_out.  target (may be
// null): the Raibert foot_pos_target_world [12].
LMPC_HD inline void advance(const lmpc_rollout_cfg& cfg, double dt, lmpc_stack_robot& sr, const lmpc_rbd_state& rs,
                            const double* foot_pos, const int32_t* touch, double* target) {
    LMPC_NO_FMA
    lmpc_robot& rb = sr.rb;
    lmpc_command& c = rb.cmd;
    lmpc_state_in& st = c.state;
    // 1. feedback: lmpc_rbd_state.euler is yaw, pitch, roll; root_euler is roll, pitch, yaw
    st.root_euler[0] = rs.euler[2];
    st.root_euler[1] = rs.euler[1];
    st.root_euler[2] = rs.euler[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        st.root_pos[a] = rs.pos[a];
        st.root_ang_vel[a] = rs.omega[a];
        st.root_lin_vel[a] = rs.lin_vel[a];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) rb.foot_pos_world[e] = foot_pos[e];
    // 2. Raibert heuristic from the current state
    const double px = st.root_pos[0], py = st.root_pos[1], pz = st.root_pos[2];
    const double cy = cos(st.root_euler[2]), sy = sin(st.root_euler[2]);
    const double vd[2] = {cy * st.root_lin_vel_d_rel[0] - sy * st.root_lin_vel_d_rel[1],
                          sy * st.root_lin_vel_d_rel[0] + cy * st.root_lin_vel_d_rel[1]};
    const double v[2] = {st.root_lin_vel[0], st.root_lin_vel[1]};
    const double lim[2] = {cfg.foot_delta_limit[0], cfg.foot_delta_limit[1]};
    const double k = sqrt(fabs(pz) / 9.8);
    const double speed = c.gait_speed;
    double delta[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double d = k * (v[a] - vd[a]) + (1.0 / speed / 2.0) / 2.0 * vd[a];
        if (d < -lim[a]) d = -lim[a];
        if (d > lim[a]) d = lim[a];
        delta[a] = d;
    }
    // ConvexMpc.cpp:38
    st.root_euler_d[2] = st.root_euler_d[2] + st.root_ang_vel_d_rel[2] * dt;
    // 3. foot_update (ConvexMpc.cpp:80-108) with LeggedContactFSM::update (LeggedContactFSM.cpp:38-84)
    const int gait = c.gait;
    const double clearance = cfg.swing_clearance;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double* df = cfg.default_feet + 3 * j;
        const double tg[3] = {(cy * df[0] - sy * df[1]) + delta[0] + px, (sy * df[0] + cy * df[1]) + delta[1] + py,
                              df[2] + pz};
        if (target) {
            target[3 * j + 0] = tg[0];
            target[3 * j + 1] = tg[1];
            target[3 * j + 2] = tg[2];
        }
        const double meas[3] = {foot_pos[3 * j + 0], foot_pos[3 * j + 1], foot_pos[3 * j + 2]};
        // the leg's FSM in locals, stored back once at the end of the body
        double P[3], V[3], S[3], E[3];  // FSM position / velocity target, swing start, swing end
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            P[a] = sr.fsm_pos_target[3 * j + a];
            V[a] = sr.fsm_vel_target[3 * j + a];
            S[a] = rb.swing_start_world[3 * j + a];
            E[a] = sr.swing_end_world[3 * j + a];
        }
        double phase = c.gait_phase[j], start = rb.fsm_start[j];
        int idx = rb.fsm_index[j], s = c.plan_contacts[j] ? 1 : 0, nfc = sr.not_first_call[j];
        if (gait == LMPC_GAIT_STAND) {
            // movement mode 0 (ConvexMpc.cpp:86-92): reset, plan_contacts true.  The FSM targets follow the measured
            // feet: this library's choice (lmpc_stack.h), the reference leaves them stale
            phase = 0.0, start = 0.0, idx = 0, nfc = 0, s = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) P[a] = meas[a], V[a] = 0.0;
        } else {
            if (!nfc) {
#pragma unroll
                for (int a = 0; a < 3; ++a) S[a] = meas[a], E[a] = tg[a], P[a] = tg[a], V[a] = 0.0;
                nfc = 1;
            }
            const LegTab t = leg_tab(gait, j);
            phase = phase + speed * dt;
            if (s == 1) {
                if (phase >= tab_end(t, idx)) {  // stance_exit, swing_enter
                    common_enter(t, idx, phase, start);
#pragma unroll
                    for (int a = 0; a < 3; ++a) S[a] = meas[a];
                    s = 0;
                }
            } else {
                const double pc = lmpc_common::fsm_percent(phase, start, tab_end(t, idx));
                if ((pc > 0.9 && touch[j] != 0) || pc >= 1.0) {  // swing_exit, stance_enter (early touchdown first)
                    s = 1;
                    common_enter(t, idx, phase, start);
#pragma unroll
                    for (int a = 0; a < 3; ++a) P[a] = meas[a], V[a] = 0.0;
                }
            }
            if (s == 0) {  // swing_update: get_foot_pos_curve takes its t as a float (Utils.cpp:136)
                const double tt = (double)(float)lmpc_common::fsm_percent(phase, start, tab_end(t, idx));
                const double np[3] = {lmpc_common::swing_bezier(tt, S[0], tg[0], 0.0),
                                      lmpc_common::swing_bezier(tt, S[1], tg[1], 0.0),
                                      lmpc_common::swing_bezier(tt, S[2], tg[2], clearance)};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    E[a] = tg[a];
                    V[a] = (np[a] - P[a]) / dt;
                    P[a] = np[a];
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            sr.fsm_pos_target[3 * j + a] = P[a];
            sr.fsm_vel_target[3 * j + a] = V[a];
            rb.swing_start_world[3 * j + a] = S[a];
            sr.swing_end_world[3 * j + a] = E[a];
        }
        c.gait_phase[j] = phase;
        rb.fsm_start[j] = start;
        rb.fsm_index[j] = idx;
        sr.not_first_call[j] = nfc;
        c.plan_contacts[j] = (uint8_t)s;
    }
    // 4. derived fields
    lmpc_common::euler_zyx_to_rot(st.root_euler[0], st.root_euler[1], st.root_euler[2], st.root_rot_mat);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        st.foot_pos_abs[3 * j + 0] = foot_pos[3 * j + 0] - px;
        st.foot_pos_abs[3 * j + 1] = foot_pos[3 * j + 1] - py;
        st.foot_pos_abs[3 * j + 2] = foot_pos[3 * j + 2] - pz;
    }
    rb.tick += 1;
}

// The 8-byte word w (0..43) of a robot's lmpc_wbc_target: [forces_des 12 | foot_pos_des 12 | foot_vel_des 12 |
// torque_limits 3, mu, swing_kp, swing_kd | contact 4 x int32].  Words 42, 43 are handled by targets_contact.
LMPC_HD inline double targets_word(const lmpc_stack_robot& sr, const double* u0, const lmpc_wbc_target& tmpl, int w) {
    if (w < 12) return u0[w];
    if (w < 24) return sr.fsm_pos_target[w - 12];
    if (w < 36) return sr.fsm_vel_target[w - 24];
    if (w < 39) return tmpl.torque_limits[w - 36];
    return w == 39 ? tmpl.mu : w == 40 ? tmpl.swing_kp : tmpl.swing_kd;
}
LMPC_HD inline int32_t targets_contact(const lmpc_stack_robot& sr, int leg) { return sr.rb.cmd.plan_contacts[leg] ? 1 : 0; }

static_assert(offsetof(lmpc_wbc_target, torque_limits) == 36 * 8 && offsetof(lmpc_wbc_target, swing_kd) == 41 * 8 &&
                  offsetof(lmpc_wbc_target, contact) == 42 * 8,
              "lmpc_wbc_target word layout");

}  // namespace lmpc_stack
