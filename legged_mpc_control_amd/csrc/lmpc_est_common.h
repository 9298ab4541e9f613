// lmpc_est_common.h -- the state estimator of include/lmpc/lmpc_est.h, written once and compiled for the host (one
// robot, the columns of P in a loop) and for gfx950 (lmpc_est.hip: one lane per column of P).
//
// P is symmetric to the bit throughout, so "column j" below is row j of the stored matrix: Pc[j][r] = P[r][j].
//
//   sensors_from_plant()  the ideal IMU / encoder readings of a plant state, plus Philox noise
//   leg_kin()             fk and J_leg qd of one leg by leg_pass on a base at the origin and at rest
//   q_diag(), xbar_elem(), pbar_col()   the predict step, one column at a time
//   meas_row(), meas_value()          row i of C (at most two entries, -1 at p and +1 at q) and y_i, R_ii
//   row_v(), step_gain(), step_x(), step_col()   one scalar measurement update: v = c P, s = v c' + r, then x and a
//                                     column of P
//   drift_det(), drift_col()          BasicKF.cpp:146-150
//   report_*()                        state_est and lmpc_est_out of a filter
//
// No function here contracts a * b + c (LMPC_NO_FMA): host and device differ only through sin / cos / log / sqrt.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "lmpc/lmpc_est.h"
#include "lmpc_common.h"
#include "lmpc_rbd_common.h"

namespace lmpc_est {
using namespace lmpc_rbd;

constexpr int NX = LMPC_EST_NX, NY = LMPC_EST_NY;
constexpr uint32_t NOISE_STREAM = 0x45535453u;  // "ESTS": the sensor noise's own Philox stream

LMPC_HD inline bool finite(double x) {
    LMPC_NO_FMA
    return x - x == 0.0;
}
LMPC_HD inline double comp(const V3& a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }
LMPC_HD inline V3 mul_t(const M3& m, const V3& a) { return V3{dot(m.cx, a), dot(m.cy, a), dot(m.cz, a)}; }  // m' a
LMPC_HD inline V3 neg(const V3& a) { return V3{-a.x, -a.y, -a.z}; }

// R = Rz(yaw) Ry(pitch) Rx(roll) of euler = (yaw, pitch, roll): base_kin()'s
LMPC_HD inline M3 rot_of(const double* euler) {
    lmpc_rbd_state s{};
    s.euler[0] = euler[0], s.euler[1] = euler[1], s.euler[2] = euler[2];
    return base_kin(s).R;
}

LMPC_HD inline bool good_cfg(const lmpc_est_cfg& c) { return c.dt > 0.0 && finite(c.dt); }
LMPC_HD inline bool good_sigmas(const lmpc_est_cfg& c) {
    return c.sigma_acc >= 0.0 && c.sigma_gyro >= 0.0 && c.sigma_euler >= 0.0 && c.sigma_joint_pos >= 0.0 &&
           c.sigma_joint_vel >= 0.0;
}

// ---- sensor model ---------------------------------------------------------------------------------------------------
LMPC_HD inline void sensors_from_plant(const lmpc_rbd_model& md, const lmpc_est_cfg& cfg, const lmpc_rbd_state& st,
                                       const lmpc_sim_out& so, int32_t robot_index, uint32_t tick, bool stand,
                                       lmpc_est_sensors& sn) {
    LMPC_NO_FMA
    const M3 R = rot_of(st.euler);
    const V3 acc = mul_t(R, v3(so.qdd[0], so.qdd[1], so.qdd[2] + md.gravity));
    const V3 gyro = mul_t(R, v3(st.omega[0], st.omega[1], st.omega[2]));
    sn.imu_acc[0] = acc.x, sn.imu_acc[1] = acc.y, sn.imu_acc[2] = acc.z;
    sn.imu_ang_vel[0] = gyro.x, sn.imu_ang_vel[1] = gyro.y, sn.imu_ang_vel[2] = gyro.z;
    for (int i = 0; i < 3; ++i) sn.euler[i] = st.euler[i];
    for (int i = 0; i < 12; ++i) sn.joint_pos[i] = st.joint_pos[i], sn.joint_vel[i] = st.joint_vel[i];
    for (int l = 0; l < 4; ++l) sn.contact[l] = stand || so.touch[l] != 0 ? 1.0 : 0.0;
    // a channel with sigma 0 draws nothing: exact sensors do not depend on the seed
    lmpc_common::Philox rng(cfg.seed, (uint64_t)(uint32_t)robot_index | ((uint64_t)tick << 32), NOISE_STREAM);
    if (cfg.sigma_acc > 0.0)
        for (int i = 0; i < 3; ++i) sn.imu_acc[i] = sn.imu_acc[i] + rng.normal(cfg.sigma_acc);
    if (cfg.sigma_gyro > 0.0)
        for (int i = 0; i < 3; ++i) sn.imu_ang_vel[i] = sn.imu_ang_vel[i] + rng.normal(cfg.sigma_gyro);
    if (cfg.sigma_euler > 0.0)
        for (int i = 0; i < 3; ++i) sn.euler[i] = sn.euler[i] + rng.normal(cfg.sigma_euler);
    if (cfg.sigma_joint_pos > 0.0)
        for (int i = 0; i < 12; ++i) sn.joint_pos[i] = sn.joint_pos[i] + rng.normal(cfg.sigma_joint_pos);
    if (cfg.sigma_joint_vel > 0.0)
        for (int i = 0; i < 12; ++i) sn.joint_vel[i] = sn.joint_vel[i] + rng.normal(cfg.sigma_joint_vel);
}

// ---- leg kinematics -------------------------------------------------------------------------------------------------
struct LegKin {
    V3 fk;  // foot in the body frame (foot_pos_rel)
    V3 fv;  // J_leg qd (foot_vel_rel)
};

// `st` carries the joints only: its base is at the origin, unrotated and at rest.
LMPC_HD inline LegKin leg_kin(const lmpc_rbd_model& md, const lmpc_rbd_state& st, int leg) {
    const BaseKin bk = base_kin(st);
    LegOut g;
    leg_pass(md, st, bk, leg, g);
    return LegKin{g.foot, g.foot_vel};
}

// ---- predict --------------------------------------------------------------------------------------------------------
LMPC_HD inline double contact_scale(double c) {
    LMPC_NO_FMA
    return 1 + (1 - c) * 1e3;
}
// Q[j][j] (BasicKF.cpp:91-97)
LMPC_HD inline double q_diag(const lmpc_est_cfg& cfg, int j, const double* contact) {
    LMPC_NO_FMA
    if (j < 3) return cfg.noise_pimu * cfg.dt / 20.0;
    if (j < 6) return cfg.noise_vimu * cfg.dt * 9.8 / 20.0;
    return contact_scale(contact[(j - 6) / 3]) * cfg.dt * cfg.noise_pfoot;
}
// u = R imu_acc + (0, 0, -gravity)
LMPC_HD inline V3 input_u(const lmpc_est_cfg& cfg, const M3& R, const double* imu_acc) {
    LMPC_NO_FMA
    V3 u = mul(R, v3(imu_acc[0], imu_acc[1], imu_acc[2]));
    u.z = u.z + -cfg.gravity;
    return u;
}
// element j of A x + B u from x[j] and x[j + 3] (read only when j < 3)
LMPC_HD inline double xbar_elem(int j, double xj, double xj3, double dt, double ux, double uy, double uz) {
    LMPC_NO_FMA
    const double pos = xj + dt * xj3;
    const double vx = xj + dt * ux, vy = xj + dt * uy, vz = xj + dt * uz;
    return j < 3 ? pos : j == 3 ? vx : j == 4 ? vy : j == 5 ? vz : xj;
}
// Column j of A P A' + Q from column j of P and column j + 3 (read only when j < 3).  The top-left block is summed as
// (a + dt (b + c)) + dt^2 d, which is the same number for [r][j] and [j][r].
LMPC_HD inline void pbar_col(int j, const double* Pj, const double* Pj3, double dt, double qj, double* out) {
    LMPC_NO_FMA
    const bool left = j < 3;
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        double a = Pj[r];
        if (r < 3) {
            const double both = (a + dt * (Pj[r + 3] + Pj3[r])) + (dt * dt) * Pj3[r + 3];
            const double rows = a + dt * Pj[r + 3];
            a = left ? both : rows;
        } else {
            const double cols = a + dt * Pj3[r];
            a = left ? cols : a;
        }
        out[r] = r == j ? a + qj : a;
    }
}

// ---- measurements ---------------------------------------------------------------------------------------------------
// Row i of C: -1 at p (p < 0: no such entry) and +1 at q.
LMPC_HD constexpr int meas_p(int i) { return i < 12 ? i % 3 : -1; }
LMPC_HD constexpr int meas_q(int i) { return i < 12 ? 6 + i : i < 24 ? 3 + (i - 12) % 3 : 6 + 3 * (i - 24) + 2; }
LMPC_HD constexpr int meas_leg(int i) { return i < 12 ? i / 3 : i < 24 ? (i - 12) / 3 : i - 24; }

// y_i and R_ii (BasicKF.cpp:101-109, 122-131) from the leg's kinematics and contact flag c; x_z = x[2] and x_vel =
// x[3:6] of the estimate BEFORE the predict step (by value: a ?: over elements of an array in memory becomes an
// indexed load on the device, which puts the array into scratch).
LMPC_HD inline void meas_value(const lmpc_est_cfg& cfg, int i, const M3& R, const V3& w_body, const LegKin& k, double c,
                               double x_z, const V3& x_vel, double& y, double& r) {
    LMPC_NO_FMA
    const double scale_c = contact_scale(c);
    const int kk = i < 12 ? i % 3 : (i - 12) % 3;
    const double y_fk = comp(mul(R, k.fk), kk);
    const V3 leg_v = sub(neg(k.fv), cross(w_body, k.fk));
    const double y_v = (1.0 - c) * comp(x_vel, kk) + c * comp(mul(R, leg_v), kk);
    const double y_z = (1.0 - c) * (x_z + k.fk.z);
    y = i < 12 ? y_fk : i < 24 ? y_v : y_z;
    const double r_z = cfg.assume_flat_ground ? scale_c * cfg.noise_zfoot : 1e5;
    r = i < 12 ? scale_c * cfg.noise_pimu_rel_foot : i < 24 ? scale_c * cfg.noise_vimu_rel_foot : r_z;
}

// ---- one scalar update ----------------------------------------------------------------------------------------------
// (c P)[j] from column j
LMPC_HD inline double row_v(const double* Pj, int p, int q) {
    LMPC_NO_FMA
    return p < 0 ? Pj[q] : Pj[q] - Pj[p];
}
// s = c P c' + r and the innovation from v and x at the row's entries p and q (single: the row has no p); false for
// a non-positive (or NaN) s
LMPC_HD inline bool step_gain(double vp, double vq, bool single, double r, double y, double xp, double xq, double& inv_s,
                              double& gain_e) {
    LMPC_NO_FMA
    const double s = single ? vq + r : (vq - vp) + r;
    const double e = single ? y - xq : y - (xq - xp);
    inv_s = 1.0 / s;
    gain_e = e * inv_s;
    return s > 0.0;
}
LMPC_HD inline double step_x(double xj, double vj, double gain_e) {
    LMPC_NO_FMA
    return xj + vj * gain_e;
}
// (v_r v_j) / s is the same number for [r][j] and [j][r]: P stays symmetric to the bit
LMPC_HD inline void step_col(double* Pj, const double* v, double vj, double inv_s) {
    LMPC_NO_FMA
#pragma unroll
    for (int r = 0; r < NX; ++r) Pj[r] = Pj[r] - (v[r] * vj) * inv_s;
}

// ---- the drift rule (BasicKF.cpp:146-150) -----------------------------------------------------------------------------
LMPC_HD inline double drift_det(double p00, double p11, double p01, double p10) {
    LMPC_NO_FMA
    return p00 * p11 - p01 * p10;
}
LMPC_HD inline void drift_col(int j, double* Pj, double divisor) {
    LMPC_NO_FMA
    const bool block = j < 2;
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        const double kept = r < 2 ? Pj[r] / divisor : 0.0;
        const double other = r < 2 ? 0.0 : Pj[r];
        Pj[r] = block ? kept : other;
    }
}

// ---- report ---------------------------------------------------------------------------------------------------------
struct LegReport {
    V3 rel, world, vel;
};
// BaseInterface.cpp:296-301 on the estimate pos = x[0:3], vel = x[3:6]
LMPC_HD inline LegReport report_leg(const M3& R, const V3& w_body, const LegKin& k, const double* x) {
    LMPC_NO_FMA
    LegReport o;
    o.rel = k.fk;
    o.world = add(mul(R, k.fk), v3(x[0], x[1], x[2]));
    o.vel = add(add(mul(R, k.fv), v3(x[3], x[4], x[5])), mul(R, cross(w_body, k.fk)));
    return o;
}
LMPC_HD inline V3 world_omega(const M3& R, const double* imu_ang_vel) {
    return mul(R, v3(imu_ang_vel[0], imu_ang_vel[1], imu_ang_vel[2]));
}

// ---- one robot by one thread: the host functions, and the device's init kernel ----------------------------------------
LMPC_HD inline void host_kin(const lmpc_rbd_model& md, const lmpc_est_sensors& sn, LegKin* k) {
    lmpc_rbd_state js{};
    for (int i = 0; i < 12; ++i) js.joint_pos[i] = sn.joint_pos[i], js.joint_vel[i] = sn.joint_vel[i];
    for (int l = 0; l < 4; ++l) k[l] = leg_kin(md, js, l);
}

LMPC_HD inline void init_robot(const lmpc_rbd_model& md, const lmpc_est_cfg& cfg, const lmpc_est_sensors& sn, const double* pos0,
                       lmpc_est_filter& f) {
    LegKin k[4];
    host_kin(md, sn, k);
    const M3 R = rot_of(sn.euler);
    for (int j = 0; j < NX; ++j) f.x[j] = 0.0;
    for (int j = 0; j < NX * NX; ++j) f.P[j] = 0.0;
    f.ticks = 0;
    for (int j = 0; j < NX; ++j) f.P[j * NX + j] = cfg.init_P;
    f.x[0] = pos0 ? pos0[0] : 0.0, f.x[1] = pos0 ? pos0[1] : 0.0, f.x[2] = pos0 ? pos0[2] : 0.09;
    for (int l = 0; l < 4; ++l) {
        const V3 w = add(mul(R, k[l].fk), v3(f.x[0], f.x[1], f.x[2]));
        f.x[6 + 3 * l] = w.x, f.x[7 + 3 * l] = w.y, f.x[8 + 3 * l] = w.z;
    }
    f.inited = 1;
}

LMPC_HD inline void report_robot(const lmpc_rbd_model& md, const lmpc_est_sensors& sn, const lmpc_est_filter& f,
                         lmpc_rbd_state* se, lmpc_est_out* out) {
    LegKin k[4];
    host_kin(md, sn, k);
    const M3 R = rot_of(sn.euler);
    const V3 wb = v3(sn.imu_ang_vel[0], sn.imu_ang_vel[1], sn.imu_ang_vel[2]);
    if (se) {
        const V3 w = world_omega(R, sn.imu_ang_vel);
        for (int i = 0; i < 3; ++i) se->euler[i] = sn.euler[i], se->pos[i] = f.x[i], se->lin_vel[i] = f.x[3 + i];
        se->omega[0] = w.x, se->omega[1] = w.y, se->omega[2] = w.z;
        for (int i = 0; i < 12; ++i) se->joint_pos[i] = sn.joint_pos[i], se->joint_vel[i] = sn.joint_vel[i];
    }
    if (out) {
        *out = lmpc_est_out{};
        for (int l = 0; l < 4; ++l) {
            const LegReport g = report_leg(R, wb, k[l], f.x);
            for (int i = 0; i < 3; ++i) {
                out->foot_pos_rel[3 * l + i] = comp(g.rel, i), out->foot_pos_world[3 * l + i] = comp(g.world, i);
                out->foot_vel_world[3 * l + i] = comp(g.vel, i);
            }
            out->estimated_contacts[l] = sn.contact[l] < 0.5 ? 0 : 1;
        }
    }
}

// One update in place.  Returns the status; on 1 the filter is as it was and state_est / out are zero but for the
// status.
inline int update_robot(const lmpc_rbd_model& md, const lmpc_est_cfg& cfg, const lmpc_est_sensors& sn, lmpc_est_filter& f,
                        lmpc_rbd_state* se, lmpc_est_out* out) {
    LegKin k[4];
    host_kin(md, sn, k);
    const M3 R = rot_of(sn.euler);
    const V3 wb = v3(sn.imu_ang_vel[0], sn.imu_ang_vel[1], sn.imu_ang_vel[2]);
    bool bad = f.inited == 0;
    double x[NX], Pc[NX][NX], y[NY], rd[NY];
    const V3 u = input_u(cfg, R, sn.imu_acc);
    for (int j = 0; j < NX; ++j) x[j] = xbar_elem(j, f.x[j], f.x[j < 3 ? j + 3 : j], cfg.dt, u.x, u.y, u.z);
    for (int j = 0; j < NX; ++j)
        pbar_col(j, f.P + j * NX, f.P + (j < 3 ? j + 3 : j) * NX, cfg.dt, q_diag(cfg, j, sn.contact), Pc[j]);
    for (int i = 0; i < NY; ++i) meas_value(cfg, i, R, wb, k[meas_leg(i)], sn.contact[meas_leg(i)], f.x[2], v3(f.x[3], f.x[4], f.x[5]),
                   y[i], rd[i]);
    for (int i = 0; i < NY; ++i) {
        const int p = meas_p(i), q = meas_q(i);
        double v[NX], inv_s, gain_e;
        for (int j = 0; j < NX; ++j) v[j] = row_v(Pc[j], p, q);
        const int pp = p < 0 ? 0 : p;
        bad = !step_gain(v[pp], v[q], p < 0, rd[i], y[i], x[pp], x[q], inv_s, gain_e) || bad;
        for (int j = 0; j < NX; ++j) x[j] = step_x(x[j], v[j], gain_e);
        for (int j = 0; j < NX; ++j) step_col(Pc[j], v, v[j], inv_s);
    }
    if (drift_det(Pc[0][0], Pc[1][1], Pc[1][0], Pc[0][1]) > cfg.drift_threshold)
        for (int j = 0; j < NX; ++j) drift_col(j, Pc[j], cfg.drift_divisor);
    for (int j = 0; j < NX; ++j) {
        bad = bad || !finite(x[j]);
        for (int r = 0; r < NX; ++r) bad = bad || !finite(Pc[j][r]);
    }
    if (bad) {
        if (se) std::memset(se, 0, sizeof *se);
        if (out) std::memset(out, 0, sizeof *out), out->status = 1;
        return 1;
    }
    for (int j = 0; j < NX; ++j) {
        f.x[j] = x[j];
        for (int r = 0; r < NX; ++r) f.P[j * NX + r] = Pc[j][r];
    }
    f.ticks += 1;
    report_robot(md, sn, f, se, out);
    return 0;
}

LMPC_HD inline void feedback_robot(const lmpc_sim_out& so, const lmpc_est_out& eo, lmpc_sim_out& sh) {
    if (&sh != &so) sh = so;
    for (int i = 0; i < 12; ++i) sh.foot_pos[i] = eo.foot_pos_world[i], sh.foot_vel[i] = eo.foot_vel_world[i];
    for (int l = 0; l < 4; ++l) sh.touch[l] = eo.estimated_contacts[l];
}

}  // namespace lmpc_est
