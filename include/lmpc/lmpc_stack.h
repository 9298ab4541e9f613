/*
 * lmpc_stack.h -- the full control loop on the device: MPC -> whole-body controller -> rigid-body plant, for batches
 * of robots on one stream (library liblmpc.so).
 *
 * lmpc_rollout.h closes the MPC around its own linearised stage-0 model: its FSM never sees a contact flag and its
 * feet are the FSM's own bookkeeping.  This header joins the three stages that exist in HBM into the reference's one
 * path (file:line relative to the reference's src/legged_ctrl):
 *
 *   ConvexMpc::update around the QP, on MEASURED feet and the contact flag   src/mpc_ctrl/convex_mpc/ConvexMpc.cpp:24-108
 *   LeggedContactFSM::update in full, early touchdown included               src/utils/LeggedContactFSM.cpp:16-84,214-278
 *   the swing Bezier                                                         src/utils/Utils.cpp:136-192
 *   the Raibert foothold                                                     src/interfaces/BaseInterface.cpp:358-399
 *   optimized_state / optimized_input -> the WBC's targets                   ConvexMpc.cpp:54-56, BaseInterface.cpp:502-530
 *   the whole-body controller                                                lmpc_rbd.h, lmpc_hoqp.h (rbd.WbcPipeline)
 *   the robot                                                                lmpc_sim.h's plant, used exactly as it is
 *                                                                            (stands in for Gazebo)
 *
 * One MPC tick of a robot (`lmpc_stack_robot`), period params.dt:
 *
 *   advance (before the solve), from the robot's lmpc_rbd_state and the plant's latest lmpc_sim_out:
 *     1. feedback (BaseInterface.cpp:511-518 read backwards) -- from the plant's own state and block, or, when the
 *        caller runs the estimator of lmpc_est.h between the plant and this call, from its state_est and its shadow
 *        lmpc_sim_out (stack.StackLoop's `estimator` option does):
 *          cmd.state.root_euler = (roll, pitch, yaw) = (state.euler[2], state.euler[1], state.euler[0])
 *          root_pos, root_ang_vel (world), root_lin_vel (world) copied
 *          foot_pos_world[l] = sim_out.foot_pos[l]            the measured feet (state.fbk.foot_pos_world), all four
 *          foot_contact_flag[l] = sim_out.touch[l] != 0       the plant's stand-in for the foot force sensor
 *     2. the Raibert target from that state, then root_euler_d[2] += yaw_rate dt (ConvexMpc.cpp:38): lmpc_rollout.h's
 *        formulas.
 *     3. LeggedContactFSM::update per leg with foot_pos_cur_world the MEASURED foot:
 *          first call (not_first_call == 0): swing start = measured foot, swing end = target, FSM position target =
 *            target, FSM velocity target = 0
 *          gait_phase += gait_speed dt
 *          STANCE -> SWING when phase >= the state's end: common_enter, swing start = measured foot
 *          SWING -> STANCE when percent_in_state() > 0.9 and the flag is set (early touchdown), else when
 *            percent_in_state() >= 1: common_enter, FSM position target = measured foot, velocity target = 0
 *          common_enter: next pattern entry; a wrap of the pattern index wraps the phase by -1; start time = phase
 *          in SWING (swing_update): position target = the Bezier at (float)percent_in_state() from the swing start to
 *            the Raibert target (clearance cfg.swing_clearance); swing end = target; velocity target = (new position
 *            target - previous position target) / dt -- the reference's finite difference, restated, not improved
 *        The legs' phases differ after an early touchdown and may be negative (lmpc_command.gait_phase[4]).
 *        LMPC_GAIT_STAND is the reference's movement mode 0 (ConvexMpc.cpp:86-92): every FSM reset every tick
 *        (phase 0, first pattern entry, not_first_call = 0), plan_contacts all true.  The FSM position targets are
 *        then set to the measured feet and the velocity targets to 0: THIS LIBRARY'S CHOICE -- the reference leaves
 *        them stale in mode 0 (its WBC ignores them there; this one's swing task reads them for every foot).
 *     4. derived fields: root_rot_mat = euler_zyx_to_rot(root_euler), foot_pos_abs = measured foot - root_pos,
 *        plan_contacts = the FSM states, tick += 1.
 *   the QP (lmpc.h) on that command; u_0 = its first 12 forces.
 *   targets (after the solve), from a template lmpc_wbc_target (torque limits, mu, swing gains):
 *     forces_des = u_0 (ConvexMpc.cpp:54), foot_pos_des / foot_vel_des = the FSM targets (:55-56),
 *     contact = plan_contacts.
 *
 * Then `wbc_per_mpc` low-level ticks, the targets held between MPC ticks as in the reference: the WBC on the current
 * state and those targets, then one plant step (`substeps` substeps of sim_cfg.dt) on its torques.  The plant's
 * candidate contacts are physical, not planned:
 *     candidate[l] = held[l] | touch[l]   of the previous plant step (lmpc_stack_candidates_device)
 * A foot stays a candidate while it carries load, even after its O(dt^2) drift has lifted it a hair off ground_z; a
 * lifted swing foot is a candidate once more and the unilateral rule (sim_cfg.unilateral = 1) releases it; a swing
 * foot that reaches the ground becomes a candidate on the next step.
 * wbc_per_mpc * substeps * sim_cfg.dt must equal params.dt (to 1e-12; lmpc_stack_check_rates).  The reference's
 * rates are 10 ms / 1.25 ms = 8.
 *
 * Chosen here, not restated:
 *   - Zero latency: an MPC tick's result is applied to the low-level ticks that follow it at once.  The reference's
 *     MPC and low-level loops are asynchronous threads; the delay between them is not modelled.
 *   - The feedback is whatever lmpc_rbd_state / lmpc_sim_out the caller passes: the plant's own (perfect state
 *     knowledge), or the estimate of lmpc_est.h (the reference's BasicKF on a sensor model of the plant, with noise).
 *   - touch as the contact flag, the candidate rule above, and mode 0's FSM targets (see 3.).
 *   - Nothing special is done for a robot whose QP, WBC chain or plant step reports a non-zero status: it continues
 *     on what those stages return -- the QP's forces as they are (zeros for LMPC_QP_NAN), the hierarchical solver's
 *     x as it is, and, on the plant's status 1, the state passed through unchanged with a zeroed lmpc_sim_out (so no
 *     held and no touch: the next step has no candidates and the FSM sees no contact, and foot_pos = 0).  Every
 *     stage is per robot: one robot's failure never changes another's bits.
 *
 * The arithmetic of advance and targets is written once (csrc/lmpc_stack_common.h, no FMA contraction) and compiled
 * for the host (lmpc_stack_advance, lmpc_stack_targets) and for gfx950: the two differ only through sin, cos and
 * sqrt.  Flat ground only.  Warm-started ticks are not offered: an early touchdown breaks the one-step shift of the
 * active set.
 *
 * Return codes, stream and ordering conventions are lmpc.h's / lmpc_rollout.h's.
 */
#ifndef LMPC_LMPC_STACK_H
#define LMPC_LMPC_STACK_H

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rbd.h"
#include "lmpc/lmpc_rollout.h"
#include "lmpc/lmpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_STACK_ABI_VERSION 1

/* everything one robot's MPC carries between ticks */
typedef struct lmpc_stack_robot {
    lmpc_robot rb;                /* cmd: the command of the last advance; foot_pos_world: the measured feet it saw;
                                     swing_start_world, fsm_start, fsm_index: the FSMs; tick: MPC ticks taken */
    double fsm_pos_target[12];    /* FSM_foot_pos_target_world, leg-major xyz */
    double fsm_vel_target[12];    /* FSM_foot_vel_target_world */
    double swing_end_world[12];   /* swing_end_foot_pos_world */
    int32_t not_first_call[4];    /* per leg */
} lmpc_stack_robot;

int lmpc_stack_abi_version(void);
int lmpc_stack_robot_size(void); /* sizeof(lmpc_stack_robot): bindings check their mirror against it */

/* LMPC_OK when wbc_per_mpc * substeps * sim_cfg->dt equals params->dt to 1e-12 (both counts >= 1), else
 * LMPC_ERR_ARG. */
int lmpc_stack_check_rates(const lmpc_params* params, const lmpc_sim_cfg* sim_cfg, int wbc_per_mpc, int substeps);

/* A robot in `state` commanded the body velocity vel_d (x, y; body frame), yaw_rate and height: FSMs at reset
 * (LeggedContactFSM.cpp:16-36, not_first_call = 0), root_euler_d = (0, 0, yaw), tick 0.  first_out: zero but for
 * foot_pos from the model's kinematics of `state` (lmpc_rbd_compute) and touch = held = foot_pos_z <= cfg->ground_z +
 * 1e-9, so that tick 0 has feedback and the first plant step has candidates. */
int lmpc_stack_robot_init(const lmpc_rollout_cfg* cfg, const lmpc_rbd_model* model, const lmpc_rbd_state* state,
                          const double vel_d[2], double yaw_rate, double height, int gait, double gait_speed,
                          lmpc_stack_robot* robot, lmpc_sim_out* first_out);

/* One robot's advance, host (steps 1-4 above).  foot_target (may be NULL) receives the Raibert
 * foot_pos_target_world [12]. */
int lmpc_stack_advance(const lmpc_params* p, const lmpc_rollout_cfg* cfg, lmpc_stack_robot* robot,
                       const lmpc_rbd_state* state, const lmpc_sim_out* sim_out, double* foot_target);
/* One robot's targets, host: a pure copy -- the template's torque_limits, mu, swing_kp, swing_kd; forces_des = u0;
 * foot_pos_des / foot_vel_des = the FSM targets; contact = plan_contacts. */
int lmpc_stack_targets(const lmpc_stack_robot* robot, const double u0[12], const lmpc_wbc_target* tmpl,
                       lmpc_wbc_target* target);

/* ---- device: every buffer resident in HBM, asynchronous on `stream` ------
 * batch == 0: LMPC_OK, nothing done.  LMPC_ERR_ARG: a NULL required pointer, a negative batch, a stride below its
 * minimum, a stream on another device than the context's (the functions without a context: than d_robots' /
 * d_sim_out's). */

/* The context's record buffers and solver workspace for `batch` robots, so that no later call of this header
 * allocates (growing a buffer synchronises the device). */
int lmpc_stack_reserve(lmpc_ctx* ctx, int batch);
/* Advance d_robots[batch] from d_state[batch] and d_sim_out[batch] and, in the same launch, expand the new commands
 * into the context's record and contact buffers by the functions lmpc_build_records_device uses (bit-identical to it).
 * lmpc_stack_solve_device then solves them.  Joins the context's launch ordering like every entry point that uses
 * the context's buffers. */
int lmpc_stack_advance_device(lmpc_ctx* ctx, const lmpc_rollout_cfg* cfg, lmpc_stack_robot* d_robots,
                              const lmpc_rbd_state* d_state, const lmpc_sim_out* d_sim_out, int batch, void* stream);
/* Cold solves, on the context's normal routing, of the `batch` QPs the last lmpc_stack_advance_device left in the
 * context: what lmpc_solve_commands_device does after its own expansion.  d_grf [batch][H][12]; d_status / d_iters
 * [batch], may be NULL.  batch above the record buffers' size (no advance of that many robots yet): LMPC_ERR_ARG. */
int lmpc_stack_solve_device(lmpc_ctx* ctx, int batch, double* d_grf, int32_t* d_status, int32_t* d_iters, void* stream);
/* Copies of the first `batch` records [batch][33 + 12 H] and contact schedules [batch][H][4] of the context's own
 * buffers, as the last expansion left them, for inspection.  batch above the buffers' size: LMPC_ERR_ARG. */
int lmpc_stack_copy_records_device(lmpc_ctx* ctx, int batch, double* d_rec, uint8_t* d_contact, void* stream);

/* d_target[b] = lmpc_stack_targets(d_robots[b], u_0 = d_grf + b * grf_stride (doubles, >= 12: the solver's
 * [B][H][12] output has stride 12 H), *tmpl). */
int lmpc_stack_targets_device(const lmpc_stack_robot* d_robots, const double* d_grf, int64_t grf_stride,
                              const lmpc_wbc_target* tmpl, int batch, lmpc_wbc_target* d_target, void* stream);
/* d_candidates[b][l] = d_sim_out[b].held[l] | d_sim_out[b].touch[l] (0 / 1), int32 [batch][4]: the plant's candidate
 * contacts of the next step. */
int lmpc_stack_candidates_device(const lmpc_sim_out* d_sim_out, int batch, int32_t* d_candidates, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_LMPC_STACK_H */
