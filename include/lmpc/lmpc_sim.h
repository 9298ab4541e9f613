/* lmpc_sim.h -- C-ABI of the batched rigid-body plant: contact-constrained forward dynamics and a time-stepping
 * integrator over the dynamics terms of lmpc_rbd.h.  Torques and a candidate contact set in; accelerations, contact
 * forces and the next state out: one robot on the host, or a batch resident in HBM.
 *
 * Coordinates, leg order and the lmpc_rbd_state <-> (q, v) conversion are lmpc_rbd.h's: q = [pos, yaw, pitch, roll,
 * joints], v = [world linear velocity, Euler rates, joint rates], |pitch| < pi/2.  S' tau = [0 (6); tau (12)].  For a
 * held set C of feet, J_C holds the three rows of J of each held foot.
 *
 * Forward dynamics (acceleration level).  Given state, tau and a candidate contact set,
 *     M qdd - J_C' F_C = S' tau - h,        J_C qdd = -(dJ v)_C;
 * F of every foot outside C is exactly 0.0.
 *
 * One plant step of length dt (velocity level).  One linear solve covers sustained contact and inelastic touchdown,
 * and leaves no velocity drift on held feet:
 *     M v+ - J_C' P_C = M v + dt (S' tau - h(q, v)),     J_C v+ = 0,     q+ = q + dt v+,
 * solved for the increment v+ - v (J_C (v+ - v) = -J_C v).  Reported: qdd = (v+ - v) / dt, force = P / dt; the next
 * lmpc_rbd_state from (q+, v+) with omega = E(euler+) rates+; foot_vel = J(q) v+, foot_pos = foot_pos(q) + dt foot_vel
 * (from the J already at hand: no second kinematics pass), touch[l] = foot_pos_z[l] <= cfg.ground_z -- the plant's
 * stand-in for a foot force sensor.  substeps > 1 repeats the step with tau and the candidates held.
 *
 * Unilateral rule (cfg.unilateral, default on; flat ground, normal = z).  Start with C = the candidates; solve;
 * release every foot of C whose normal component of F (or P) is < 0; repeat until none is released.  The set only
 * shrinks: at most four solves.  A fourth solve that still releases a foot has emptied the set (every pass released at
 * least one of at most four candidates): every F (or P) is then 0.0 and the result is the free body's, with no further
 * solve.  The final set is reported as held[4].  With unilateral = 0 the candidates are held
 * bilaterally.  This is a fixed, deterministic rule, NOT the solution of a complementarity problem: a released foot
 * is not re-added within a step, the friction cone is not enforced (no sliding contact), and held feet drift in
 * position by O(dt^2) per step.
 *
 * Elimination.  M is block-arrowhead (a 6 x 6 base block, four 3 x 3 leg blocks, 6 x 3 couplings, no leg-leg
 * coupling) and a foot's J touches the base columns and its own leg's three.  So every leg's joints are eliminated on
 * their own (a 3 x 3 Cholesky), which leaves M's Schur complement on the base (one 6 x 6 Cholesky) and then the dense
 * J_C M^-1 J_C' (at most 12 x 12, a block Cholesky over the legs); back-substitution for the base, then per leg.  No
 * pivoting: every factor is symmetric positive definite.  Every sum over legs runs in the order FL, FR, RL, RR on the
 * host and on the device: a robot's result does not depend on its place in the batch, and the two sides differ only
 * through sin / cos.
 *
 * Status per robot.  0 = solved.  1 = a non-positive pivot (for J_C M^-1 J_C': one not above 1e-10 of its diagonal
 * entry, i.e. singular to rounding) or a non-finite result: the state is passed through
 * unchanged (of a step with substeps > 1: the state that entered the failing substep) and every other field of
 * lmpc_sim_out is zero.
 *
 * Return codes and the stream convention are lmpc.h's.  The device functions take no context and allocate nothing.
 */
#ifndef LMPC_SIM_H
#define LMPC_SIM_H

#include <stddef.h>
#include <stdint.h>

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rbd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_SIM_ABI_VERSION 1

typedef struct {
    double dt;          /* length of one (sub)step, > 0 */
    double ground_z;    /* height of the flat ground, for touch[] */
    int32_t unilateral; /* 1: release feet that pull (the rule above); 0: hold the candidates bilaterally */
    int32_t reserved;   /* 0 */
} lmpc_sim_cfg;

typedef struct {
    double qdd[18];      /* forward dynamics: qdd; step: (v+ - v) / dt of the last substep */
    double force[12];    /* F, or P / dt of the last substep; exactly 0.0 on feet that are not held */
    double foot_pos[12]; /* forward dynamics: foot_pos(q); step: foot_pos(q) + dt foot_vel */
    double foot_vel[12]; /* forward dynamics: J v; step: J(q) v+ */
    int32_t held[4];     /* the final contact set */
    int32_t touch[4];    /* step: foot_pos_z <= ground_z; forward dynamics: 0 */
    int32_t status;      /* 0 solved, 1 failed */
    int32_t reserved;    /* 0 */
} lmpc_sim_out;

int lmpc_sim_abi_version(void);
int lmpc_sim_cfg_size(void);
int lmpc_sim_out_size(void);
/* dt = 0.002, ground_z = 0, unilateral = 1 */
void lmpc_sim_cfg_default(lmpc_sim_cfg* cfg);
/* Bytes of caller-provided workspace the device functions need for `batch` robots: 0, the plant is one kernel that
 * keeps everything in registers.  Negative batch: 0. */
size_t lmpc_sim_work_bytes(int batch);

/* One robot, host.  tau: 12 doubles; contact: 4 candidate flags (non-zero = candidate).  `next` may alias `state`.
 * NULL pointers, or cfg->dt that is not a positive finite number: LMPC_ERR_ARG. */
int lmpc_rbd_forward_dynamics(const lmpc_rbd_model* model, const lmpc_rbd_state* state, const double* tau,
                              const int32_t* contact, int unilateral, lmpc_sim_out* out);
int lmpc_sim_step(const lmpc_rbd_model* model, const lmpc_sim_cfg* cfg, const lmpc_rbd_state* state, const double* tau,
                  const int32_t* contact, lmpc_rbd_state* next_state, lmpc_sim_out* out);

/* A batch on the device (every buffer resident in HBM), asynchronous on `stream`.  Robot b reads tau at
 * d_tau + b * tau_stride (in doubles, >= 12) and its candidates at d_contact + b * contact_stride (in int32s, >= 4):
 * tau straight from the WBC's x[B][3][42] (offset 30 of the last level, stride 126), the candidates from
 * lmpc_wbc_target.contact (stride 88).  d_next may alias d_state; d_out may be NULL.  d_work / work_bytes:
 * lmpc_sim_work_bytes(batch) bytes, may be NULL / 0.  batch == 0: LMPC_OK, nothing done.  NULL required pointers with
 * a positive batch, a negative batch, strides below 12 / 4, substeps < 1 or a dt that is not positive and finite:
 * LMPC_ERR_ARG. */
int lmpc_rbd_forward_dynamics_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state, const double* d_tau,
                                     int64_t tau_stride, const int32_t* d_contact, int64_t contact_stride, int batch,
                                     int unilateral, lmpc_sim_out* d_out, void* stream);
int lmpc_sim_step_device(const lmpc_rbd_model* model, const lmpc_sim_cfg* cfg, const lmpc_rbd_state* d_state,
                         const double* d_tau, int64_t tau_stride, const int32_t* d_contact, int64_t contact_stride,
                         int batch, int substeps, lmpc_rbd_state* d_next, lmpc_sim_out* d_out, void* d_work,
                         size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_SIM_H */
