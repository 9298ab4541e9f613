/* lmpc_rbd.h -- C-ABI of the batched floating-base rigid-body dynamics that feed the whole-body controller.
 *
 * The reference takes the WBC's dynamics terms from Pinocchio (src/legged_ctrl/src/wbc_ctrl/wbc.cpp:59-91) and
 * derives the base-acceleration and swing-leg targets from them (wbc.cpp:177-246).  This header produces the same
 * quantities from the robot's measured state: one robot on the host, or a batch resident in HBM, as the
 * lmpc_wbc_input blocks of lmpc_hoqp.h that lmpc_wbc_tasks_device turns into hierarchical-QP records.
 *
 * Model class.  A trunk and four legs of three revolute joints each (hip, thigh, calf), every actuated joint frame
 * unrotated against its parent link (`rpy="0 0 0"` in the URDF) with the axes x, y, y, and one foot point per calf.
 * Links on fixed joints are lumped into their moving ancestor, as Pinocchio does when it reads a URDF
 * (tools/urdf_to_rbd.py).  Both of the reference's robots (Go1, A1) are of this class.
 *
 * Coordinates.  The base is OCS2's composite of a translation and a ZYX spherical joint:
 *     q = [pos (3), yaw, pitch, roll, joints (12)],   v = [lin_vel_world (3), euler-angle rates (3), joint_vel (12)],
 *     R = Rz(yaw) Ry(pitch) Rx(roll),                 omega_world = E(euler) rates.
 * q and v are formed from lmpc_rbd_state exactly as wbc.cpp:49-57 forms them.  The Euler parametrisation is singular
 * at |pitch| = pi/2: |pitch| < pi/2 is required; beyond it the outputs are non-finite, and no error is returned.
 * Leg order FL, FR, RL, RR; joint 3 * leg + k (k = 0 hip, 1 thigh, 2 calf) is q index 6 + 3 * leg + k.
 *
 * Definitions (the specification; parity with Pinocchio / OCS2 themselves is not pinned):
 *     M         joint-space inertia in the coordinates above, sum_b m_b Jv_b' Jv_b + Jw_b' (R_b I_b R_b') Jw_b,
 *               symmetric with both triangles written (wbc.cpp:67); by the composite-rigid-body algorithm
 *     nle       h(q, v) of M qdd + h = tau_gen, gravity included; by recursive Newton-Euler at qdd = 0
 *     J         d p_foot / d q per foot (3 x 18): the LOCAL_WORLD_ALIGNED translation rows in these coordinates
 *     dJv       the foot's acceleration at qdd = 0, d/dt (J(q(t)) v) along qdot = v
 *     foot_pos, foot_vel   p_foot and J v
 *     swing_acc kp (foot_pos_des - foot_pos) + kd (foot_vel_des - foot_vel), every foot (wbc.cpp:239)
 *     Ab        left 6 x 6 block of the centroidal momentum matrix: v[0:6] -> [linear momentum; angular momentum
 *               about the CoM], world-aligned axes.  Block upper triangular: the lower-left block is exactly zero.
 *     base_accel (wbc.cpp:195-203, restated, not repaired)  b = Ab^-1 hdot with
 *               hdot = [sum_i f_i + m g_vec; sum_i (foot_pos_i - com) x f_i] over all four feet of forces_des,
 *               m the model's total mass, g_vec = (0, 0, -gravity); then b[3:6] -= Aww^-1 (w x (Aww w)) with
 *               Aww = Ab[3:6, 3:6] and w the world angular velocity E rates.
 * Every sum over bodies runs in the fixed order trunk, FL, FR, RL, RR (within a leg: calf, thigh, hip), on the host
 * and on the device: a robot's result does not depend on its position in the batch, and the two sides differ only
 * through sin / cos of the Euler and joint angles (a few ulp).
 *
 * Return codes and the stream convention are lmpc.h's (LMPC_OK / LMPC_ERR_*; `stream` is a hipStream_t, NULL = the
 * null stream).  The device functions take no context and allocate nothing.
 */
#ifndef LMPC_RBD_H
#define LMPC_RBD_H

#include <stddef.h>
#include <stdint.h>

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_hoqp.h" /* lmpc_wbc_input */

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_RBD_ABI_VERSION 1
#define LMPC_RBD_BODIES 13

/* Body 0 = trunk, body 1 + 3 * leg + k = hip / thigh / calf of leg `leg` (fixed-joint children lumped in). */
typedef struct {
    double mass[LMPC_RBD_BODIES];
    double com[LMPC_RBD_BODIES][3];     /* centre of mass in the link frame */
    double inertia[LMPC_RBD_BODIES][6]; /* ixx ixy ixz iyy iyz izz about the CoM, link axes */
    double joint_origin[12][3];         /* joint 3 * leg + k in its parent link's frame */
    double foot[4][3];                  /* foot point in the calf frame */
    double gravity;                     /* 9.81: Pinocchio's, which the WBC's terms use -- not the MPC's 9.8 (lmpc_params) */
} lmpc_rbd_model;

/* The reference's measured_rbd_state (BaseInterface.cpp:511-518), 36 doubles. */
typedef struct {
    double euler[3];      /* ZYX: yaw, pitch, roll */
    double pos[3];
    double joint_pos[12];
    double omega[3];      /* world angular velocity */
    double lin_vel[3];    /* world linear velocity of the base origin */
    double joint_vel[12];
} lmpc_rbd_state;

/* Targets of the work-space WBC tasks (swing_task_type != 0, wbc.cpp:224-229) and its constants. */
typedef struct {
    double forces_des[12];   /* input_desired.head(12) */
    double foot_pos_des[12]; /* state_desired.segment(6 + 3 i, 3) */
    double foot_vel_des[12]; /* input_desired.segment(12 + 3 i, 3) */
    double torque_limits[3]; /* HAA HFE KFE (config/task.info: 33.5 each) */
    double mu;               /* 0.3 */
    double swing_kp;         /* 350 */
    double swing_kd;         /* 37 */
    int32_t contact[4];      /* stance flags, FL FR RL RR */
} lmpc_wbc_target;

/* The dynamics alone. */
typedef struct {
    double M[18 * 18];
    double nle[18];
    double J[12 * 18];
    double dJv[12];
    double foot_pos[12];
    double foot_vel[12];
    double com[3];       /* world */
    double Ab[36];       /* row-major */
    double mass;         /* total */
} lmpc_rbd_terms;

int lmpc_rbd_abi_version(void);
int lmpc_rbd_model_size(void);
int lmpc_rbd_state_size(void);
int lmpc_wbc_target_size(void);
int lmpc_rbd_terms_size(void);

/* Values of the reference's urdf/go1_description/urdf/go1.urdf and urdf/a1_description/urdf/a1.urdf (tests/golden/
 * rbd_model_*.json, written by tools/urdf_to_rbd.py), legs in the library's order. */
void lmpc_rbd_model_go1(lmpc_rbd_model* m);
void lmpc_rbd_model_a1(lmpc_rbd_model* m);
/* config/task.info's torque limits 33.5, friction 0.3, swing gains 350 / 37; zero targets, all feet in stance */
void lmpc_wbc_target_default(lmpc_wbc_target* t);

/* one robot, host */
int lmpc_rbd_compute(const lmpc_rbd_model* model, const lmpc_rbd_state* state, lmpc_rbd_terms* terms);
int lmpc_wbc_input_from_state(const lmpc_rbd_model* model, const lmpc_rbd_state* state, const lmpc_wbc_target* target,
                              lmpc_wbc_input* in);

/* A batch on the device (every buffer resident in HBM), asynchronous on `stream`.  batch == 0: LMPC_OK, nothing
 * done; NULL pointers with a positive batch, or a negative batch: LMPC_ERR_ARG. */
int lmpc_wbc_inputs_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state, const lmpc_wbc_target* d_target,
                           int batch, lmpc_wbc_input* d_in, void* stream);
int lmpc_rbd_compute_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state, int batch,
                            lmpc_rbd_terms* d_terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_RBD_H */
