/*
 * lmpc_rollout.h -- a device-resident closed-loop MPC rollout for batches of robots (library liblmpc.so).
 *
 * lmpc.h is one MPC tick: commands in, GRFs out, the robot's next state from somewhere outside the library.  This
 * header closes the loop in HBM: `ticks` MPC ticks for `batch` robots on one stream with no host synchronisation
 * between ticks.  Each tick restates, per robot (file:line relative to the reference's src/legged_ctrl):
 *
 *   what ConvexMpc::update does around the QP             src/mpc_ctrl/convex_mpc/ConvexMpc.cpp:24-108
 *   the per-leg contact FSM with its foot bookkeeping     src/utils/LeggedContactFSM.cpp:16-84,214-278
 *   the swing Bezier                                      src/utils/Utils.cpp:136-192
 *   the Raibert foothold                                  src/interfaces/BaseInterface.cpp:358-399
 *   the QP's own stage-0 transition as the plant          src/mpc_ctrl/convex_mpc/ConvexQPSolver.cpp:198-228,294-297
 *       x+ = A(yaw) x + B u_0 - g dt e11   (stands in for Gazebo: the MPC's prediction of x_1 and the plant agree)
 *
 * Flat ground only: the plant lands every foot at cfg.ground_z and the QPs are the reference's (no terrain normals).
 * No force sensor: a swing ends when percent_in_state() >= 1, never by an early touchdown.
 *
 * Two properties of the reference are restated, not repaired:
 *   - the FSM alternates STANCE / SWING blindly on every state exit (LeggedContactFSM.cpp:54-72), so the three-entry
 *     patterns (crawl FR / RL, trot-with-stand FR / RL) run inverted on every other cycle; the reference only ever
 *     enables trot.  Every gait gets the same per-tick arithmetic; only trot tracks its command.
 *   - the one-entry stand pattern would leave STANCE at phase 1.0; LMPC_GAIT_STAND here is the reference's movement
 *     mode 0 (ConvexMpc.cpp:86-92): the FSMs are reset every tick and all plan_contacts are true.
 *
 * The arithmetic of a tick is written once (csrc/lmpc_common.h, no FMA contraction) and compiled for the host
 * (lmpc_robot_advance) and for gfx950 (the rollout's advance kernel): the two differ only through sin, cos and sqrt.
 *
 * Return codes, stream and ordering conventions are lmpc.h's.
 */
#ifndef LMPC_LMPC_ROLLOUT_H
#define LMPC_LMPC_ROLLOUT_H

#include "lmpc/lmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_ROLLOUT_ABI_VERSION 1

typedef struct lmpc_rollout_cfg {
    double default_feet[12];    /* default_foot_pos_rel, leg-major (as lmpc_synth_cfg) */
    double swing_clearance;     /* FOOT_SWING_CLEARANCE2 (LeggedParams.h:27, the float 0.23f); CLEARANCE1 is 0 */
    double foot_delta_limit[2]; /* FOOT_DELTA_X/Y_LIMIT, 0.8 (LeggedParams.h:29-30) */
    double ground_z;            /* flat ground the plant lands feet on, 0 */
} lmpc_rollout_cfg;

/* everything one robot carries between ticks */
typedef struct lmpc_robot {
    lmpc_command cmd;             /* state, desired values, gait, per-leg phase, plan_contacts (= the FSM states s);
                                     the derived fields (root_rot_mat, foot_pos_abs) are rewritten every tick */
    double foot_pos_world[12];    /* stance anchors / current swing positions, leg-major xyz */
    double swing_start_world[12]; /* swing_start_foot_pos_world */
    double fsm_start[4];          /* cur_state_start_time; the end time comes from the gait table */
    int32_t fsm_index[4];         /* gait_pattern_index */
    int32_t tick;                 /* plant steps taken */
} lmpc_robot;

/* device pointers, each [ticks][batch]..., each may be NULL */
typedef struct lmpc_rollout_log {
    lmpc_command* cmd; /* [ticks][batch]      the command each tick's QP was built from */
    double* u0;        /* [ticks][batch][12]  the forces applied */
    double* x;         /* [ticks][batch][12]  [euler, pos, omega, v] after the plant step */
    int32_t* status;   /* [ticks][batch] */
    int32_t* iters;    /* [ticks][batch] */
} lmpc_rollout_log;

int lmpc_rollout_abi_version(void);
int lmpc_robot_size(void); /* sizeof(lmpc_robot): bindings check their mirror against it */
/* Go1: gazebo_go1_convex.yaml:18-35 feet, the reference's clearance and foothold limits, ground at 0 */
void lmpc_rollout_cfg_go1(lmpc_rollout_cfg* cfg);

/* A robot at x0 = [euler(3), pos(3), omega_world(3), v_world(3)] commanded the body velocity vel_d (x, y; body frame),
 * yaw_rate and height: FSMs at reset (LeggedContactFSM.cpp:16-36), feet at Rz(yaw) default_feet + pos with
 * z = ground_z, root_euler_d = (0, 0, yaw), tick 0. */
int lmpc_robot_init(const lmpc_rollout_cfg* cfg, const double x0[12], const double vel_d[2], double yaw_rate,
                    double height, int gait, double gait_speed, lmpc_robot* robot);

/* One robot's plant step, host: x+ = A(yaw) x + B u_0 - g dt e11 with A, B of the robot's current command (its
 * root_rot_mat and foot_pos_abs, as the QP that produced u0 saw them); tick += 1. */
int lmpc_robot_plant_step(const lmpc_params* p, lmpc_robot* robot, const double u0[12]);
/* One robot's tick bookkeeping, host: lmpc_robot_plant_step on u0 (skipped when u0 is NULL: the first tick), then
 * the work before the next QP in the reference's order -- the Raibert target from the current state;
 * root_euler_d[2] += yaw_rate dt (ConvexMpc.cpp:38); the FSM update per leg; swing_enter records the start position;
 * stance_enter puts the foot on the target's x, y at ground_z; a swing foot sits on the Bezier at
 * percent_in_state(); R = euler_zyx_to_rot(euler), foot_pos_abs = foot_pos_world - pos, plan_contacts = s, gait_phase
 * from the FSMs.  foot_target (may be NULL) receives the Raibert foot_pos_target_world [12]. */
int lmpc_robot_advance(const lmpc_params* p, const lmpc_rollout_cfg* cfg, lmpc_robot* robot, const double* u0,
                       double* foot_target);

/* ---- device ------------------------------------------------------------- */

/* lmpc_shift_active_set on device buffers [batch][H][4] (H the context's), asynchronous.  d_shifted must not alias
 * d_act (one thread per byte; LMPC_ERR_ARG). */
int lmpc_shift_active_set_device(lmpc_ctx* ctx, const uint8_t* d_act, int batch, uint8_t* d_shifted, void* stream);

/* lmpc_solve_batch_warm on device buffers, asynchronous: d_cmd[batch] is expanded into the context's record buffers
 * (as lmpc_solve_commands_device) and every QP goes to the scratch Riccati kernel, which starts from d_act_in
 * ([batch][H][4], NULL: cold) and writes the verified set to d_act_out (may be NULL; must not alias d_act_in).  The
 * factor workspace comes from lmpc_reserve_warm, or grows on demand.  d_normals as lmpc_solve_commands_device. */
int lmpc_solve_commands_warm_device(lmpc_ctx* ctx, const lmpc_command* d_cmd, const double* d_normals, int batch,
                                    const uint8_t* d_act_in, uint8_t* d_act_out, double* d_grf, int32_t* d_status,
                                    int32_t* d_iters, void* stream);

/* `ticks` MPC ticks for d_robots[batch], asynchronous on `stream`.  Per tick: advance (the plant step on the previous
 * tick's u_0, then the bookkeeping above), record expansion, solve; u_0 stays in a context-owned buffer.  A last
 * launch applies the final plant step, so d_robots holds the state after `ticks` ticks and calls chain: one call of
 * n + m ticks and a call of n followed by one of m leave the same bits.
 * d_act [batch][H][4] u8, read and written: the verified active set carried between ticks and between calls, shifted
 * one step before each solve; every QP then runs warm on the scratch Riccati kernel.  A zero-filled buffer is a valid
 * "nothing known" start (the kernel's own fallback makes that tick cold).  NULL: every tick is a cold solve on the
 * context's normal routing (dense, fused, LDS).
 * A robot whose QP returns status != 0 advances on the forces returned (zeros for LMPC_QP_NAN, as the reference).
 * log may be NULL; each non-NULL array of it receives [ticks][batch] entries.
 * ticks == 0 or batch == 0: LMPC_OK, nothing done.  LMPC_ERR_ARG: NULL ctx / cfg / d_robots, negative counts, a
 * stream on another device. */
int lmpc_rollout_device(lmpc_ctx* ctx, const lmpc_rollout_cfg* cfg, lmpc_robot* d_robots, uint8_t* d_act, int batch,
                        int ticks, const lmpc_rollout_log* log, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_LMPC_ROLLOUT_H */
