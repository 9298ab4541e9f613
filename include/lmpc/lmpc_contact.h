/* lmpc_contact.h -- C-ABI of the frictional contact model of the batched rigid-body plant: a second plant step, next
 * to lmpc_sim_step (lmpc_sim.h, which stays as it is), that solves a friction-pyramid complementarity problem per
 * robot per step.  Torques and a mask of feet in; accelerations, contact forces, contact modes, slip velocities and the
 * next state out: one robot on the host, or a batch resident in HBM.
 *
 * Coordinates, the velocity-level discretisation and the elimination are lmpc_sim.h's.  With
 *     v_free   M v_free = M v + dt (S' tau - h(q, v))                    the unconstrained step's velocity
 *     K        J M^-1 J'  (12 x 12, symmetric positive definite)         lmpc_sim_common.h's K, whatever the contact set
 *     u_free   J v_free                                                  the feet's velocities after that step
 *     g_l      foot_pos_z(q) - cfg.ground_z                              foot l's gap (flat ground, normal = z)
 *     b_l      (0, 0, max(g_l, -cfg.recover_speed dt) / dt)              the bias; (0, 0, 0) with cfg.use_gap = 0
 * one step solves, over the impulses P in R^12 of the feet inside the caller's mask (P_l = 0 outside it),
 *     min 1/2 P' K P + P' (u_free + b)     s.t. per foot   |P_x| <= mu P_z,   |P_y| <= mu P_z,
 * then v+ = v_free + M^-1 J' P and q+ = q + dt v+.  K is positive definite, so the optimum is unique.  This is the
 * convex (Anitescu) relaxation of Coulomb friction on the friction pyramid that the MPC and the WBC use.  With
 * w = K P + u_free + b (the foot's velocity after the step, plus the bias) the optimality conditions per foot are:
 * P in the pyramid; w in its dual cone, w_z >= mu (|w_x| + |w_y|); P' w = 0.
 *
 * Modes.  Each foot of the mask ends in one of ten modes (lmpc_contact_out.mode):
 *     0        free   P in the pyramid's interior, hence w = 0: the foot sticks
 *     1 .. 4   face   P_x = +mu P_z, P_x = -mu P_z, P_y = +mu P_z, P_y = -mu P_z: sliding against one side
 *     5 .. 8   edge   (P_x, P_y) = mu P_z (+1, +1), (+1, -1), (-1, +1), (-1, -1)
 *     9        apex   P = 0, no contact force
 * and a foot outside the mask reports 10 (not in the problem).
 *
 * What the model is and is not.
 *   - A sticking foot with zero gap gets exactly lmpc_sim_step's held-foot result (w = 0).
 *   - A foot in the air with g / dt above its approach speed gets P = 0: no candidate rule is needed, every foot can
 *     be in the mask on every step.
 *   - A landing foot is decelerated so that it arrives at gap 0 and does not penetrate (w_z = 0 means
 *     foot_vel_z+ = -g / dt).  A foot below the ground is pushed out at no more than cfg.recover_speed (default 0: it is
 *     held where it is).
 *   - A sliding foot separates at mu (|w_x| + |w_y|): the relaxation's known artefact.  For the same reason a fast
 *     tangential swing foot within about mu |u_t| dt of the ground feels the ground early.
 *   - The cone is the pyramid, not the second-order cone; the ground is flat; friction does not enter the
 *     acceleration-level forward dynamics (lmpc_rbd_forward_dynamics is unchanged).
 * cfg.use_gap = 0 switches the bias off and treats the mask as lmpc_sim_step treats its candidates (all at gap 0):
 * with a large mu the step then agrees with lmpc_sim_step wherever that one's rule ends on a complementary set.
 *
 * Solver.  (1) All feet of the mask are first tried as sticking (the linear solve of lmpc_sim_step's first pass).
 * (2) Otherwise block Gauss-Seidel sweeps over the four feet, each foot's 3-variable pyramid problem solved exactly by
 * evaluating its ten modes in closed form and taking the feasible minimiser; (3) after every sweep the modes are
 * fixed, every P_l restricted to its mode's basis (3 x {3, 2, 1, 0}, padded with the identity) and the reduced system
 * solved by the 4 x 4 block Cholesky over the legs (the polish); (4) the certificate below decides; a polished point
 * that is feasible becomes the next sweep's start.  cfg.max_sweeps and cfg.max_polish cap (2) and (1) + (3); once the
 * polish rounds are used up the sweeps continue and are certified as they are.
 *
 * Certificate (independent of the algebra that produced P), all relative to s = max(1, |P|inf, |u_free + b|inf) over
 * the feet of the mask:  primal: every pyramid slack >= -tol_p s.  dual, per foot by mode: free |w|inf <= tol_d s;
 * face / edge: the least-squares multipliers of the active faces' normals are >= -tol_d s and their fit residual is
 * <= tol_d s; apex: w_z - mu (|w_x| + |w_y|) >= -tol_d s.  lmpc_contact_out.res_primal / res_dual are the largest
 * violations divided by s.
 *
 * Status per robot.  0 = the returned P passed the certificate.  1 = a non-positive pivot (lmpc_sim.h's rule) or a
 * non-finite result: the state is passed through unchanged and every other field is zero (lmpc_sim.h).  2 = no
 * active set verified within the caps: the last feasible iterate is used and flagged.  With substeps > 1 the status
 * covers the whole step: 0 means every substep was certified, 2 that some substep was not (and none failed); the
 * other fields report the last substep.
 *
 * Outputs.  The step writes lmpc_sim.h's lmpc_sim_out with force = P / dt, held[l] = P_z[l] > 0 and touch by
 * cfg.touch_rule: 0 = geometric, foot_pos_z <= ground_z (lmpc_sim.h); 1 = |force_l| > cfg.force_threshold, the
 * reference's force-sensor threshold (BaseInterface.cpp:319-328) with the plant's exact force as the sensor.  With
 * use_gap = 1 a foot that carries a force ends at gap 0 by construction (w_z = 0), so its geometric flag is decided
 * by rounding: rule 0 tells a foot in the air from one below the ground, not a loaded foot from an unloaded one.
 * Use rule 1 (or held) for that.
 *
 * Device forms.  lmpc_contact_step_device runs one fused kernel (substeps with the state in registers) when d_work
 * is NULL, and with a workspace of lmpc_contact_work_bytes(batch) bytes three launches per substep -- K and c into
 * the workspace, the bare solve, the back-substitution -- which leave the same bits.  The fused kernel is the faster
 * one as measured and what the library's loops use.
 *
 * Every sum over feet runs in the order FL, FR, RL, RR on the host and on the device: a robot's result does not depend
 * on its place in the batch, and the two sides differ only through sin / cos.
 *
 * Return codes and the stream convention are lmpc.h's.  The device functions take no context and allocate nothing.
 */
#ifndef LMPC_CONTACT_H
#define LMPC_CONTACT_H

#include <stddef.h>
#include <stdint.h>

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rbd.h"
#include "lmpc/lmpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_CONTACT_ABI_VERSION 1

#define LMPC_CONTACT_MODE_FREE 0
#define LMPC_CONTACT_MODE_APEX 9
#define LMPC_CONTACT_MODE_NONE 10
#define LMPC_CONTACT_MAX_CAP 1024 /* the largest max_sweeps / max_polish accepted */

typedef struct {
    double dt;              /* length of one (sub)step, > 0 */
    double ground_z;        /* height of the flat ground */
    double mu;              /* friction coefficient of the pyramid, > 0 */
    double recover_speed;   /* >= 0: the largest speed at which a foot below the ground is pushed out */
    double force_threshold; /* touch_rule 1: touch[l] = |force_l| > force_threshold (newtons) */
    double tol_p;           /* certificate, primal */
    double tol_d;           /* certificate, dual */
    int32_t use_gap;        /* 1: the bias b from the gaps; 0: every foot of the mask at gap 0 */
    int32_t touch_rule;     /* 0: geometric; 1: force threshold */
    int32_t max_sweeps;     /* cap on the Gauss-Seidel sweeps of one step, 0 .. LMPC_CONTACT_MAX_CAP */
    int32_t max_polish;     /* cap on the polish rounds of one step, 0 .. LMPC_CONTACT_MAX_CAP */
} lmpc_contact_cfg;

typedef struct {
    double w[12];       /* K P + u_free + b per foot: the slip velocity (plus the bias); 0 outside the mask */
    double gap[4];      /* foot_pos_z(q) - ground_z before the (last sub)step; the bare solve: 0 */
    double res_primal;  /* the certificate's largest primal violation / s */
    double res_dual;    /* the certificate's largest dual violation / s */
    int32_t mode[4];    /* 0 .. 9, or 10 outside the mask */
    int32_t sweeps;     /* Gauss-Seidel sweeps used */
    int32_t polish;     /* polish rounds used */
    int32_t status;     /* 0 certified, 1 failed, 2 not certified within the caps */
    int32_t reserved;   /* 0 */
} lmpc_contact_out;

int lmpc_contact_abi_version(void);
int lmpc_contact_cfg_size(void);
int lmpc_contact_out_size(void);
/* dt = 0.002, ground_z = 0, mu = 0.6 (the feet's mu1 / mu2 in the reference's go1_description/xacro/gazebo.xacro:
 * 293-294), recover_speed = 0, force_threshold = 50 N (foot_sensor_min_value + foot_sensor_ratio * (max - min) of the
 * reference's gazebo_go1_lci.yaml:51-53, the rule of BaseInterface.cpp:324-325; a standing Go1 carries about 30 N per
 * foot, so set it lower for a robot at rest), tol_p = tol_d = 1e-9, use_gap = 1, touch_rule = 0, max_sweeps = 16,
 * max_polish = 8. */
void lmpc_contact_cfg_default(lmpc_contact_cfg* cfg);
/* Bytes of caller-provided workspace the three-launch form of lmpc_contact_step_device needs for `batch` robots
 * (1544 per robot); the fused form needs none.  batch <= 0: 0. */
size_t lmpc_contact_work_bytes(int batch);

/* The bare problem, one on the host: K 12 x 12 row-major (symmetric positive definite), c = u_free + b (12), mask (4,
 * non-zero = in the problem) -> P (12) and *out (w, mode, sweeps, polish, residuals, status; gap = 0).  Of cfg only mu,
 * tol_p, tol_d, max_sweeps and max_polish are read.  Status 1: P = 0.  NULL pointers, mu or a tolerance that is not
 * positive and finite, or a cap outside 0 .. LMPC_CONTACT_MAX_CAP: LMPC_ERR_ARG. */
int lmpc_contact_solve(const lmpc_contact_cfg* cfg, const double* K, const double* c, const int32_t* mask, double* P,
                       lmpc_contact_out* out);
/* One robot's step on the host.  tau: 12 doubles; mask: 4 flags.  `next_state` may alias `state`; `cout` may be NULL.
 * NULL pointers otherwise, a dt, mu or tolerance that is not positive and finite, a recover_speed or force_threshold
 * that is negative or not finite, a cap outside 0 .. LMPC_CONTACT_MAX_CAP or a touch_rule other than 0 / 1:
 * LMPC_ERR_ARG. */
int lmpc_contact_step(const lmpc_rbd_model* model, const lmpc_contact_cfg* cfg, const lmpc_rbd_state* state,
                      const double* tau, const int32_t* mask, lmpc_rbd_state* next_state, lmpc_sim_out* out,
                      lmpc_contact_out* cout);

/* Batches on the device (every buffer resident in HBM), asynchronous on `stream`.  The bare solve: d_K [batch][144],
 * d_c [batch][12], d_mask [batch][4], d_P [batch][12], d_out [batch] (may be NULL). */
int lmpc_contact_solve_device(const lmpc_contact_cfg* cfg, const double* d_K, const double* d_c, const int32_t* d_mask,
                              int batch, double* d_P, lmpc_contact_out* d_out, void* stream);
/* lmpc_sim_step_device's argument list (strided tau, strided mask, substeps with tau and the mask held, d_next may
 * alias d_state, d_out may be NULL) plus d_cout [batch] (may be NULL), which reports the last substep.  d_work /
 * work_bytes: NULL / 0 (the fused kernel), or at least lmpc_contact_work_bytes(batch) bytes (the three-launch form;
 * a non-NULL d_work with fewer bytes: LMPC_ERR_ARG).  batch == 0: LMPC_OK, nothing done.  Argument errors as
 * lmpc_sim_step_device's and lmpc_contact_step's: LMPC_ERR_ARG. */
int lmpc_contact_step_device(const lmpc_rbd_model* model, const lmpc_contact_cfg* cfg, const lmpc_rbd_state* d_state,
                             const double* d_tau, int64_t tau_stride, const int32_t* d_mask, int64_t mask_stride,
                             int batch, int substeps, lmpc_rbd_state* d_next, lmpc_sim_out* d_out,
                             lmpc_contact_out* d_cout, void* d_work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_CONTACT_H */
