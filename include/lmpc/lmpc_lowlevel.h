/*
 * lmpc_lowlevel.h -- the reference's joint-PD low-level controller, for one robot on the host or a batch resident in
 * HBM (library liblmpc.so).
 *
 * In simulation the reference does not fly its whole-body controller: GazeboInterface::ctrl_update calls
 * tau_ctrl_update and leaves wbc_update commented out (src/interfaces/GazeboInterface.cpp:75-77).  This header is
 * that path (file:line relative to the reference's src/legged_ctrl/src):
 *
 *   BaseInterface::tau_ctrl_update        interfaces/BaseInterface.cpp:451-489
 *   A1Kinematics::inv_kin, closed form    utils/A1Kinematics.cpp:321-446
 *   the torque sent to the joints         interfaces/GazeboInterface.cpp:106-110
 *
 * Per robot, from an lmpc_rbd_state, an lmpc_wbc_target (only forces_des, foot_pos_des and foot_vel_des are read:
 * optimized_input.head(12), optimized_state.segment(6 + 3 i) and optimized_input.segment(12 + 3 i),
 * ConvexMpc.cpp:54-56) and a gait word; per leg i with joints q_i, rates qd_i:
 *
 *   R = Rz(yaw) Ry(pitch) Rx(roll) from state.euler
 *   joint_tau_tgt_i = -J_i' R' f_i                                  J_i = lmpc_foot_jacobian's (lmpc.h)
 *   movement mode = 0 when the gait word is LMPC_GAIT_STAND, else 1 (ConvexMpc.cpp:86-92)
 *   mode 0: joint_ang_tgt_i = q_i, joint_vel_tgt_i = qd_i           the PD terms vanish
 *   mode 1: joint_ang_tgt_i = inv_kin(R' (foot_pos_des_i - pos), q_i, rho_opt_i, rho_fix_i); any NaN component:
 *             q_i instead (flag 1)
 *           joint_vel_tgt_i = J_i^-1 R' (foot_vel_des_i - lin_vel), by a 3 x 3 LU with partial pivoting
 *             (Eigen::PartialPivLU: the largest magnitude of the column, the first one on ties; a zero pivot column is
 *             left undivided); any NaN component: qd_i instead (flag 2).  An infinity passes through.
 *   tau_i = kp_i (joint_ang_tgt_i - q_i) + kd_i (joint_vel_tgt_i - qd_i) + joint_tau_tgt_i
 *   flag 4 when a component of that tau_i is not finite; then, THIS LIBRARY'S ADDITION, each component is clamped to
 *   +-tau_limit[k] where tau_limit[k] > 0 (flag 8 when one was changed; a NaN stays a NaN).  The reference has no
 *   clamp: tau_limit <= 0.
 *
 * inv_kin is restated branch for branch, not improved: the left / right split on rho_fix's oy > 0, the Zf and Yf_ sign
 * cases (the right legs have no Zf == 0 case: both candidates stay 0 there), the choice between t1 and t1_candidate by
 * their distance to the current angle, the 0.001 windows on cos_beta, the sign flip of L, the wrap of t2 at -60 / 240
 * degrees.  rho_opt is not read by it, as in the reference.  Nothing is carried between ticks: the reference's
 * prev_joint_ang_tgt is written and never read on this path.
 *
 * Kinematics.  The reference gives both of its robots A1's link lengths (BaseInterface.cpp:76-89): that is
 * lmpc_leg_kin_default, and what lmpc_lowlevel_cfg_go1 / _a1 carry.  lmpc_leg_kin_from_model reads the lengths off an
 * lmpc_rbd_model instead, so that the controller's kinematics are the plant's; the device loop (stack.StackLoop) uses
 * that one.
 *
 * The arithmetic is written once (csrc/lmpc_lowlevel_common.h, no FMA contraction) and compiled for the host and for
 * gfx950: the two differ only through sin, cos, sqrt, atan2 and acos.
 *
 * Not here: the tauEst foot-force estimate (BaseInterface.cpp:331-350), motor delay, HardwareInterface's on-motor PD.
 *
 * Return codes, stream and ordering conventions are lmpc.h's / lmpc_stack.h's.
 */
#ifndef LMPC_LMPC_LOWLEVEL_H
#define LMPC_LMPC_LOWLEVEL_H

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rbd.h"
#include "lmpc/lmpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_LOWLEVEL_ABI_VERSION 1

#define LMPC_LL_IK_NAN 1        /* inv_kin gave a NaN: the angle target is the measured angle */
#define LMPC_LL_VEL_NAN 2       /* the velocity solve gave a NaN: the rate target is the measured rate */
#define LMPC_LL_TAU_NONFINITE 4 /* a component of tau (before the clamp) is not finite */
#define LMPC_LL_CLAMPED 8       /* a component of tau was clamped */

typedef struct lmpc_lowlevel_cfg {
    lmpc_leg_kin kin;    /* rho_fix / rho_opt per leg, FL FR RL RR (lmpc.h) */
    double kp[4][3];     /* param.kp_foot(k, leg): leg-major here, joint k = hip, thigh, calf */
    double kd[4][3];
    double tau_limit[3]; /* per joint k; <= 0: no clamp, which is the reference.  This library's addition. */
} lmpc_lowlevel_cfg;

typedef struct lmpc_lowlevel_out {
    double tau[12];           /* the torque sent: GazeboInterface.cpp:108-110.  First, so the plant reads it by stride */
    double joint_tau_tgt[12]; /* -J' R' f   (BaseInterface.cpp:455-459) */
    double joint_ang_tgt[12];
    double joint_vel_tgt[12];
    int32_t flags[4];         /* per leg: LMPC_LL_* */
} lmpc_lowlevel_out;

int lmpc_lowlevel_abi_version(void);
int lmpc_lowlevel_cfg_size(void);
int lmpc_lowlevel_out_size(void);
/* robots per block of the device kernel (for tests that straddle a block's edge) */
int lmpc_lowlevel_block_robots(void);

/* The gains of the reference's two Gazebo configurations, every leg and joint alike: kp 0.5 / kd 0.3
 * (config/gazebo_go1_convex.yaml:74-80) and kp 15 / kd 0.4 (config/gazebo_a1_convex.yaml:75-81); kin =
 * lmpc_leg_kin_default, tau_limit = 0. */
void lmpc_lowlevel_cfg_go1(lmpc_lowlevel_cfg* cfg);
void lmpc_lowlevel_cfg_a1(lmpc_lowlevel_cfg* cfg);

/* kin from the rigid-body model: per leg l
 *   rho_fix = (joint_origin[3l].x, joint_origin[3l].y, joint_origin[3l+1].y, -joint_origin[3l+2].z, -foot[l].z),
 *   rho_opt = 0.
 * LMPC_ERR_ARG (kin untouched) when any other component of those four vectors exceeds 1e-12 in magnitude: such a model
 * is outside the class A1Kinematics describes. */
int lmpc_leg_kin_from_model(const lmpc_rbd_model* model, lmpc_leg_kin* kin);

/* One leg's kinematics, host: the body-frame foot position lmpc_foot_jacobian differentiates, and the closed-form
 * inverse above (q may hold NaNs: the fallback is the controller's, not inv_kin's). */
int lmpc_leg_fk(const lmpc_leg_kin* kin, int leg, const double q[3], double p[3]);
int lmpc_leg_inv_kin(const lmpc_leg_kin* kin, int leg, const double p[3], const double cur_q[3], double q[3]);

/* One robot, host.  gait (may be NULL: mode 1): the robot's gait word. */
int lmpc_lowlevel(const lmpc_lowlevel_cfg* cfg, const lmpc_rbd_state* state, const lmpc_wbc_target* target,
                  const int32_t* gait, lmpc_lowlevel_out* out);

/* A batch on the device, one launch, asynchronous on `stream`.  d_gait (may be NULL: mode 1): robot b's gait word at
 * d_gait + b * gait_stride (int32s, >= 1; lmpc_est.h's convention: lmpc_stack_robot's rb.cmd.gait with stride
 * sizeof(lmpc_stack_robot) / 4).  d_sim_out and d_candidates, both or neither: the same launch also writes
 * d_candidates[b][l] = held[l] | touch[l] of d_sim_out[b] (0 / 1), bit for bit lmpc_stack_candidates_device's, so that a
 * low-level tick is two launches: this one and the plant's, which reads tau at d_out with stride
 * sizeof(lmpc_lowlevel_out) / 8.
 * batch == 0: LMPC_OK, nothing done.  LMPC_ERR_ARG: a NULL required pointer, a negative batch, a gait_stride below 1
 * with d_gait given, only one of d_sim_out / d_candidates, a stream on another device than d_state's. */
int lmpc_lowlevel_device(const lmpc_lowlevel_cfg* cfg, const lmpc_rbd_state* d_state, const lmpc_wbc_target* d_target,
                         const int32_t* d_gait, int64_t gait_stride, const lmpc_sim_out* d_sim_out,
                         int32_t* d_candidates, int batch, lmpc_lowlevel_out* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_LMPC_LOWLEVEL_H */
