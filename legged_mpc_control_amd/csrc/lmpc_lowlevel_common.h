// lmpc_lowlevel_common.h -- the joint-PD low-level controller (include/lmpc/lmpc_lowlevel.h), written once and
// compiled for the host (lmpc_lowlevel, lmpc_leg_fk, lmpc_leg_inv_kin) and for gfx950 (lmpc_lowlevel.hip's kernel):
//
//   BaseInterface::tau_ctrl_update      BaseInterface.cpp:451-489
//   A1Kinematics::inv_kin               A1Kinematics.cpp:321-446
//   the torque sent                     GazeboInterface.cpp:106-110
//
// One leg at a time, restated and not improved.  No FMA contraction (LMPC_NO_FMA) and no HIP runtime call: the host
// and the device differ only through sin, cos, sqrt, atan2 and acos.  Everything lives in scalars and arrays indexed by
// constants (the LU's row exchange is a select on values): nothing here needs a private (scratch) array on the device.
#pragma once
#include <cstddef>

#include "lmpc/lmpc_lowlevel.h"
#include "lmpc_common.h"

static_assert(sizeof(lmpc_lowlevel_cfg) == 472, "lmpc_lowlevel_cfg layout (mirrored by _native.LmpcLowlevelCfg)");
static_assert(sizeof(lmpc_lowlevel_out) == 400 && offsetof(lmpc_lowlevel_out, flags) == 384,
              "lmpc_lowlevel_out layout (mirrored by _native.LmpcLowlevelOut)");

namespace lmpc_ll {

constexpr double PI = 3.14159265358979323846;  // M_PI

LMPC_HD inline bool is_nan(double x) { return x != x; }
LMPC_HD inline bool is_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// What one leg reads of lmpc_lowlevel_cfg.
struct LegCfg {
    double rf[5], ro[3];  // rho_fix, rho_opt
    double kp[3], kd[3], lim[3];
};
// What one leg reads of the robot: the base, its own joints, its own targets.
struct LegIn {
    double euler[3], pos[3], lin_vel[3];  // lmpc_rbd_state's: yaw, pitch, roll
    double q[3], qd[3];
    double f[3], p_des[3], v_des[3];  // forces_des, foot_pos_des, foot_vel_des of the leg (world)
};
struct LegOut {
    double tau[3], tau_ff[3], ang[3], vel[3];
    int32_t flags;
};

// A1Kinematics::fk (A1Kinematics.cpp:8-12,38-75) in the closed form lmpc_common::foot_jacobian differentiates.
LMPC_HD inline void fk(const double rf[5], const double ro[3], const double q[3], double p[3]) {
    LMPC_NO_FMA
    const double L1 = rf[3], a = ro[0], b = rf[4] - ro[2], d = rf[2] + ro[1];
    const double s0 = sin(q[0]), c0 = cos(q[0]);
    const double s1 = sin(q[1]), c1 = cos(q[1]);
    const double s12 = sin(q[1] + q[2]), c12 = cos(q[1] + q[2]);
    const double h = L1 * c1 + (b * c12 + a * s12);
    p[0] = rf[0] - L1 * s1 - b * s12 + a * c12;
    p[1] = rf[1] + d * c0 + h * s0;
    p[2] = d * s0 - h * c0;
}

// A1Kinematics::inv_kin (A1Kinematics.cpp:321-446), branch for branch.  rho_opt is not read, as there.  atan2(L, +-d)
// is taken once per side; every use of it in the reference has these arguments.
LMPC_HD inline void inv_kin(const double rf[5], const double p[3], const double cur[3], double out[3]) {
    LMPC_NO_FMA
    const double ox = rf[0], oy = rf[1], d = rf[2], lt = rf[3], lc = rf[4];
    const double Xf = p[0], Yf = p[1], Zf = p[2];
    const double Yf_ = Yf - oy, Xf_ = Xf - ox;
    const double L_square = Zf * Zf + Yf_ * Yf_ - d * d;
    double L = sqrt(L_square);
    double t1 = 0.0, t1_candidate = 0.0, t2 = 0.0, t3 = 0.0;
    const double cur_t1 = cur[0];
    if (oy > 0) {  // FL or RL
        const double aL = atan2(L, d);
        if (Zf > 0) {  // the foot above the hip
            if (Yf_ > 0) t1 = atan2(Zf, Yf_) - aL;
            else if (Yf_ == 0) t1 = PI / 2 - aL;
            else if (Yf_ < 0) t1 = PI - atan2(Zf, -Yf_) - aL;
            t1_candidate = atan2(Zf, Yf_) + aL;
        } else if (Zf < 0) {  // below it
            if (Yf_ > 0) t1 = atan2(Zf, Yf_) + aL;
            else if (Yf_ == 0) t1 = -PI / 2 + aL;
            else if (Yf_ < 0) t1 = -PI - atan2(Zf, -Yf_) + aL;
            t1_candidate = atan2(Zf, Yf_) - aL;
        } else {
            t1 = aL;
            t1_candidate = -aL;
        }
    } else {  // FR or RR: no Zf == 0 case, both stay 0
        const double aR = atan2(L, -d);
        if (Zf > 0) {
            if (Yf_ < 0) t1 = -atan2(Zf, -Yf_) + aR;
            else if (Yf_ == 0) t1 = -PI / 2 + aR;
            else if (Yf_ > 0) t1 = -PI + atan2(Zf, Yf_) + aR;
            t1_candidate = -aR - atan2(Zf, -Yf_);
        } else if (Zf < 0) {
            if (Yf_ < 0) t1 = atan2(-Zf, -Yf_) - aR;
            else if (Yf_ == 0) t1 = -PI / 2 - aR;
            else if (Yf_ > 0) t1 = PI - atan2(-Zf, Yf_) - aR;
            t1_candidate = atan2(-Zf, -Yf_) + aR;
        }
    }
    if (!(fabs(t1 - cur_t1) < fabs(t1_candidate - cur_t1))) t1 = t1_candidate;

    const double cos_beta = (lt * lt + lc * lc - Xf_ * Xf_ - L * L) / (2 * lt * lc);
    double beta = 0;
    if (fabs(cos_beta + 1) < 0.001) beta = PI;
    else if (fabs(cos_beta - 1) < 0.001) beta = 0;
    else beta = acos(cos_beta);
    t3 = beta - PI;

    const double joint_2_z = d * sin(t1);
    if (Zf > joint_2_z) L = -L;
    const double gamma = atan2(-Xf_, L);
    const double alpha = atan2(lc * sin(-t3), lt + lc * cos(-t3));
    t2 = gamma + alpha;
    if (t2 < -60 * PI / 180) t2 = t2 + 2 * PI;
    else if (t2 > 240 * PI / 180) t2 = t2 - 2 * PI;
    out[0] = t1, out[1] = t2, out[2] = t3;
}

// x = J^-1 b as Eigen::PartialPivLU solves it (J row-major, J[3 r + c]): per column the pivot of largest magnitude,
// the first one on ties; the column below a zero pivot is left undivided; x = U^-1 L^-1 P b.  The rows are three
// scalars-of-four that are exchanged by value.
LMPC_HD inline void swap_if(bool take, double (&a)[4], double (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x = a[i], y = b[i];
        a[i] = take ? y : x;
        b[i] = take ? x : y;
    }
}
LMPC_HD inline void lu_solve3(const double J[9], const double b[3], double x[3]) {
    LMPC_NO_FMA
    double r0[4] = {J[0], J[1], J[2], b[0]}, r1[4] = {J[3], J[4], J[5], b[1]}, r2[4] = {J[6], J[7], J[8], b[2]};
    // column 0
    int piv = 0;
    double big = fabs(r0[0]);
    if (fabs(r1[0]) > big) piv = 1, big = fabs(r1[0]);
    if (fabs(r2[0]) > big) piv = 2, big = fabs(r2[0]);
    swap_if(piv == 1, r0, r1);
    swap_if(piv == 2, r0, r2);
    if (big != 0.0) {
        r1[0] = r1[0] / r0[0];
        r2[0] = r2[0] / r0[0];
    }
    r1[1] = r1[1] - r1[0] * r0[1], r1[2] = r1[2] - r1[0] * r0[2];
    r2[1] = r2[1] - r2[0] * r0[1], r2[2] = r2[2] - r2[0] * r0[2];
    // column 1
    const bool second = fabs(r2[1]) > fabs(r1[1]);
    swap_if(second, r1, r2);
    if (fabs(r1[1]) != 0.0) r2[1] = r2[1] / r1[1];
    r2[2] = r2[2] - r2[1] * r1[2];
    // L y = P b (unit lower), then U x = y
    const double y0 = r0[3];
    const double y1 = r1[3] - r1[0] * y0;
    const double y2 = r2[3] - (r2[0] * y0 + r2[1] * y1);
    x[2] = y2 / r2[2];
    x[1] = (y1 - r1[2] * x[2]) / r1[1];
    x[0] = (y0 - (r0[1] * x[1] + r0[2] * x[2])) / r0[0];
}

// One leg of tau_ctrl_update and send_cmd.  mode: the reference's movement_mode (0 standing, 1 moving).
LMPC_HD inline void leg(const LegCfg& c, const LegIn& in, int mode, LegOut& o) {
    LMPC_NO_FMA
    double R[9], J[9], fr[3];
    lmpc_common::euler_zyx_to_rot(in.euler[2], in.euler[1], in.euler[0], R);
    lmpc_common::foot_jacobian(c.rf, c.ro, in.q, J);
    // BaseInterface.cpp:455-459, in lmpc_common::leg_torque's order
#pragma unroll
    for (int r = 0; r < 3; ++r) fr[r] = R[r] * in.f[0] + R[3 + r] * in.f[1] + R[6 + r] * in.f[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.tau_ff[k] = -(J[k] * fr[0] + J[3 + k] * fr[1] + J[6 + k] * fr[2]);
    int32_t flags = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.ang[k] = in.q[k], o.vel[k] = in.qd[k];
    if (mode > 0) {
        double dp[3], dv[3], p_rel[3], v_rel[3], a[3], w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) dp[k] = in.p_des[k] - in.pos[k], dv[k] = in.v_des[k] - in.lin_vel[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            p_rel[r] = R[r] * dp[0] + R[3 + r] * dp[1] + R[6 + r] * dp[2];
            v_rel[r] = R[r] * dv[0] + R[3 + r] * dv[1] + R[6 + r] * dv[2];
        }
        inv_kin(c.rf, p_rel, in.q, a);
        if (is_nan(a[0]) || is_nan(a[1]) || is_nan(a[2])) flags |= LMPC_LL_IK_NAN;
        lu_solve3(J, v_rel, w);
        if (is_nan(w[0]) || is_nan(w[1]) || is_nan(w[2])) flags |= LMPC_LL_VEL_NAN;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o.ang[k] = (flags & LMPC_LL_IK_NAN) ? in.q[k] : a[k];
            o.vel[k] = (flags & LMPC_LL_VEL_NAN) ? in.qd[k] : w[k];
        }
    }
    // GazeboInterface.cpp:108-110, then the clamp
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double t = c.kp[k] * (o.ang[k] - in.q[k]) + c.kd[k] * (o.vel[k] - in.qd[k]) + o.tau_ff[k];
        if (!is_finite(t)) flags |= LMPC_LL_TAU_NONFINITE;
        if (c.lim[k] > 0.0) {
            if (t > c.lim[k]) t = c.lim[k], flags |= LMPC_LL_CLAMPED;
            else if (t < -c.lim[k]) t = -c.lim[k], flags |= LMPC_LL_CLAMPED;
        }
        o.tau[k] = t;
    }
    o.flags = flags;
}

// What leg `l` reads of the configuration; l is a compile-time constant on the host and the opaque
// lane index on the device.
LMPC_HD inline void leg_cfg(const lmpc_lowlevel_cfg& cfg, int l, LegCfg& c) {
#pragma unroll
    for (int i = 0; i < 5; ++i) c.rf[i] = cfg.kin.rho_fix[l][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c.ro[i] = cfg.kin.rho_opt[l][i];
        c.kp[i] = cfg.kp[l][i], c.kd[i] = cfg.kd[l][i], c.lim[i] = cfg.tau_limit[i];
    }
}

LMPC_HD inline void leg_in(const lmpc_rbd_state& st, const lmpc_wbc_target& tg, int l, LegIn& in) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        in.euler[i] = st.euler[i], in.pos[i] = st.pos[i], in.lin_vel[i] = st.lin_vel[i];
        in.q[i] = st.joint_pos[3 * l + i], in.qd[i] = st.joint_vel[3 * l + i];
        in.f[i] = tg.forces_des[3 * l + i], in.p_des[i] = tg.foot_pos_des[3 * l + i];
        in.v_des[i] = tg.foot_vel_des[3 * l + i];
    }
}

LMPC_HD inline void leg_store(const LegOut& o, int l, lmpc_lowlevel_out& out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out.tau[3 * l + i] = o.tau[i], out.joint_tau_tgt[3 * l + i] = o.tau_ff[i];
        out.joint_ang_tgt[3 * l + i] = o.ang[i], out.joint_vel_tgt[3 * l + i] = o.vel[i];
    }
    out.flags[l] = o.flags;
}

// One robot, host: the four legs in turn.
inline void robot(const lmpc_lowlevel_cfg& cfg, const lmpc_rbd_state& st, const lmpc_wbc_target& tg, int mode,
                  lmpc_lowlevel_out& out) {
    for (int l = 0; l < 4; ++l) {
        LegCfg c;
        LegIn in;
        LegOut o;
        leg_cfg(cfg, l, c);
        leg_in(st, tg, l, in);
        leg(c, in, mode, o);
        leg_store(o, l, out);
    }
}

// held | touch of the plant's last step: lmpc_stack_candidates_device's rule
LMPC_HD inline int32_t candidate(int32_t held, int32_t touch) { return (held | touch) != 0 ? 1 : 0; }

}  // namespace lmpc_ll
