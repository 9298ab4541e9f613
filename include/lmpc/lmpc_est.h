/* lmpc_est.h -- C-ABI of the batched state estimator: a sensor model over the plant of lmpc_sim.h and the reference's
 * linear Kalman filter for the base position and velocity, one robot on the host or a batch resident in HBM.
 *
 * In the reference the MPC and the WBC never see the true base position and velocity: they see BasicKF's estimate
 * (file:line relative to the reference's src/legged_ctrl):
 *
 *   BasicKF, 18 states and 28 measurements            src/estimation/BasicKF.cpp, include/estimation/BasicKF.h
 *   what feeds it and what is derived from it         src/interfaces/BaseInterface.cpp:212-301, 404-449 (kf_type == 1)
 *
 * State x = [pos (3), vel (3), foot FL (3), FR, RL, RR], world frame.  Measurements y = [R fk_l - that is foot_l - pos
 * (4 x 3), the base velocity seen through every leg (4 x 3), the four foot heights].  The orientation is taken as
 * known from the IMU (sensors.euler), exactly as BasicKF does.
 *
 * One update (BasicKF::update_estimation, restated line by line; c_l = sensors.contact[l], k_l = 1 + (1 - c_l) 1e3):
 *   A = 1 + dt [pos <- vel], B = dt [vel <- u], u = R imu_acc + (0, 0, -gravity)                       (:74-78)
 *   Q = diag(noise_pimu dt / 20 (3), noise_vimu dt 9.8 / 20 (3), k_l dt noise_pfoot (3 per leg))        (:91-97)
 *   R = diag(k_l noise_pimu_rel_foot (3 per leg), k_l noise_vimu_rel_foot (3 per leg), k_l noise_zfoot (1 per leg));
 *       with assume_flat_ground = 0 the four height entries are 1e5 whatever the contact                (:101-109, :53)
 *   xbar = A x + B u, Pbar = A P A' + Q                                                                 (:114-115)
 *   y[3 l + i]      = (R fk_l)[i]
 *   y[12 + 3 l + i] = (1 - c_l) x[3 + i] + c_l (R leg_v_l)[i],  leg_v = -J_leg qd - imu_ang_vel x fk    (:125-127)
 *                     -- x is the PREVIOUS estimate, not xbar: the reference's quirk, restated
 *   y[24 + l]       = (1 - c_l) (x[2] + fk_l.z)                 -- the body-frame fk_z, and again x      (:129-130)
 *   x+ = xbar + Pbar C' S^-1 (y - C xbar), P+ = Pbar - Pbar C' S^-1 C Pbar, S = C Pbar C' + R           (:133-142)
 *   P+ = (P+ + P+') / 2                                                                                 (:143)
 *   if P+[0][0] P+[1][1] - P+[0][1] P+[1][0] > drift_threshold: rows and columns 0, 1 of P+ are cleared outside their
 *     2 x 2 block, and the block is divided by drift_divisor                                            (:146-150)
 *   estimated_contacts[l] = c_l >= 0.5                                                                  (:154-160)
 *
 * Chosen here, not restated:
 *   - The linear solve.  R is diagonal, so the 28 measurements are applied one after the other as scalar updates
 *     (for row c with variance r: v = c P, s = v c' + r, x += v' (y - c x) / s, P -= v' v / s), in the order of y
 *     above.  In exact arithmetic this IS the block update with S^-1 (the reference: fullPivHouseholderQr); no 28 x
 *     28 matrix is formed or factored.  Every row of C has at most two entries, +-1, so v is a difference of two
 *     rows of P and s a sum of at most three numbers.  P -= (v_r v_j) / s keeps P symmetric to the bit, so the
 *     symmetrisation (:143) is the identity and is not executed; Pbar is formed so that it is symmetric to the bit
 *     as well.  P must be symmetric on entry (lmpc_est_init's is; an update's output is).
 *   - Leg kinematics: fk and J_leg qd come from lmpc_rbd_common.h's leg_pass on the lmpc_rbd_model with the base at the
 *     origin and at rest (the reference's commented-out Pinocchio route), not from A1Kinematics' fitted parameters.
 *   - lmpc_est_out's world feet use the estimate of the SAME tick (the reference's sensor_update computes them
 *     before the filter runs, from the previous tick's): foot_pos_world = R fk + x[0:3], foot_vel_world = R (J_leg
 *     qd) + x[3:6] + R (imu_ang_vel x fk) (BaseInterface.cpp:299-301).
 *   - BasicKF's movement-mode rule (:81-82, contact = 1 for every foot while standing) is applied by whoever fills
 *     lmpc_est_sensors: lmpc_est_sensors_from_plant's `stand` flag.
 *
 * Status per robot.  0 = updated.  1 = a non-positive innovation variance s, a non-finite result, or a filter that
 * was never initialised (inited == 0): the filter is left unchanged, state_est and lmpc_est_out are zero except for
 * the status (and so are the shadow lmpc_sim_out's foot_pos, foot_vel and touch).
 *
 * Sensor model (lmpc_est_sensors_from_plant): what an ideal IMU and encoders read on the plant,
 *   imu_acc = R' (sim_out.qdd[0:3] + (0, 0, model.gravity)), imu_ang_vel = R' state.omega, euler / joint_pos /
 *   joint_vel copied, contact = touch (or 1 with `stand`),
 * plus optional additive Gaussian noise: sigma per channel in cfg, drawn from Philox4x32-10 (lmpc_common.h) on a
 * stream of its own, keyed by (cfg.seed, robot_index, tick) and drawn in the order acc, gyro, euler, joint_pos,
 * joint_vel -- the host and the device draw the same numbers; a channel whose sigma is 0 draws nothing and adds
 * nothing, so with every sigma 0 the sensors are exact and do not depend on the seed.  With the plant's substeps > 1
 * qdd is the LAST substep's (v+ - v) / dt, not the mean over the tick: a sampling effect of this sensor model.
 *
 * Every sum runs in a fixed order on the host and on the device: a robot's result does not depend on its place in
 * the batch, and the two sides differ only through sin / cos (and log / sqrt of the noise).  fp64 throughout.
 * Return codes and the stream convention are lmpc.h's.  The device functions take no context and allocate nothing.
 */
#ifndef LMPC_EST_H
#define LMPC_EST_H

#include <stddef.h>
#include <stdint.h>

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rbd.h"
#include "lmpc/lmpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_EST_ABI_VERSION 1
#define LMPC_EST_NX 18
#define LMPC_EST_NY 28

/* what the reference's `fbk` carries into the filter, 37 doubles */
typedef struct {
    double imu_acc[3];     /* body-frame specific force */
    double imu_ang_vel[3]; /* body frame */
    double euler[3];       /* ZYX: yaw, pitch, roll (lmpc_rbd_state's order) */
    double joint_pos[12];
    double joint_vel[12];
    double contact[4];     /* foot_contact_flag in [0, 1] */
} lmpc_est_sensors;

typedef struct {
    double dt;                   /* the filter's period, > 0 */
    double noise_pimu;           /* PROCESS_NOISE_PIMU 0.01          (BasicKF.h:15-20) */
    double noise_vimu;           /* PROCESS_NOISE_VIMU 0.01 */
    double noise_pfoot;          /* PROCESS_NOISE_PFOOT 0.01 */
    double noise_pimu_rel_foot;  /* SENSOR_NOISE_PIMU_REL_FOOT 0.001 */
    double noise_vimu_rel_foot;  /* SENSOR_NOISE_VIMU_REL_FOOT 0.1 */
    double noise_zfoot;          /* SENSOR_NOISE_ZFOOT 0.001 */
    double gravity;              /* 9.81 (BasicKF.cpp:78) */
    double drift_threshold;      /* 1e-6 (:146) */
    double drift_divisor;        /* 10 (:149) */
    double init_P;               /* 3 (:61) */
    double sigma_acc;            /* sensor-noise sigmas of lmpc_est_sensors_from_plant, all 0 by default */
    double sigma_gyro;
    double sigma_euler;
    double sigma_joint_pos;
    double sigma_joint_vel;
    uint64_t seed;
    int32_t assume_flat_ground;  /* 1 */
    int32_t reserved;            /* 0 */
} lmpc_est_cfg;

/* per-robot persistent state; lives in HBM between calls.  P is the full 18 x 18, both triangles (row-major, and
 * symmetric to the bit, so column-major just as well): 2744 bytes. */
typedef struct {
    double x[LMPC_EST_NX];
    double P[LMPC_EST_NX * LMPC_EST_NX];
    int32_t inited; /* 0 until lmpc_est_init */
    int32_t ticks;  /* updates taken since init */
} lmpc_est_filter;

typedef struct {
    double foot_pos_rel[12];       /* fk, body frame, leg-major xyz */
    double foot_pos_world[12];     /* R fk + estimated pos */
    double foot_vel_world[12];     /* BaseInterface.cpp:300-301 on the estimated velocity */
    int32_t estimated_contacts[4]; /* contact >= 0.5 */
    int32_t status;                /* 0 updated, 1 failed */
    int32_t reserved;              /* 0 */
} lmpc_est_out;

int lmpc_est_abi_version(void);
int lmpc_est_sensors_size(void);
int lmpc_est_cfg_size(void);
int lmpc_est_filter_size(void);
int lmpc_est_out_size(void);
/* dt = 0.00125 and the reference's constants; sigmas 0, seed 0 */
void lmpc_est_cfg_default(lmpc_est_cfg* cfg);

/* ---- one robot, host.  NULL required pointers, or a cfg->dt that is not positive and finite (a negative sigma for
 * the sensor model): LMPC_ERR_ARG. */
int lmpc_est_sensors_from_plant(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg, const lmpc_rbd_state* state,
                                const lmpc_sim_out* sim_out, int32_t robot_index, uint32_t tick, int stand,
                                lmpc_est_sensors* sensors);
/* BasicKF::init_state: P = init_P 1, x = 0 but pos = pos0 (NULL: the reference's (0, 0, 0.09)) and feet = R fk + pos;
 * inited = 1, ticks = 0. */
int lmpc_est_init(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg, const lmpc_est_sensors* sensors,
                  const double* pos0, lmpc_est_filter* filter);
/* state_est and out of a filter as it stands (what an update reports after it): euler, joint_pos, joint_vel from the
 * sensors, omega = R imu_ang_vel (BaseInterface.cpp:218), pos / lin_vel = x[0:3] / x[3:6].  Either output may be
 * NULL.  out->status = 0. */
int lmpc_est_report(const lmpc_rbd_model* model, const lmpc_est_sensors* sensors, const lmpc_est_filter* filter,
                    lmpc_rbd_state* state_est, lmpc_est_out* out);
/* BasicKF::update_estimation, in place; then lmpc_est_report.  state_est and out may be NULL.  The robot's status is
 * returned in out->status; the return value is LMPC_OK whatever the status. */
int lmpc_est_update(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg, const lmpc_est_sensors* sensors,
                    lmpc_est_filter* filter, lmpc_rbd_state* state_est, lmpc_est_out* out);
/* The loop's feedback: *shadow = *sim_out with foot_pos / foot_vel = out's world feet and touch =
 * estimated_contacts.  shadow may alias sim_out. */
int lmpc_est_feedback(const lmpc_sim_out* sim_out, const lmpc_est_out* out, lmpc_sim_out* shadow);

/* ---- a batch on the device: every buffer resident in HBM, asynchronous on `stream`.  batch == 0: LMPC_OK, nothing
 * done.  A NULL required pointer with a positive batch, a negative batch, a stride below its minimum or a bad cfg:
 * LMPC_ERR_ARG. */

/* Robot b is keyed (cfg->seed, index0 + b, tick).  d_gait (may be NULL): robot b's gait at d_gait + b * gait_stride
 * (int32s; lmpc_stack_robot's rb.cmd.gait with stride sizeof(lmpc_stack_robot) / 4); LMPC_GAIT_STAND there is
 * `stand`. */
int lmpc_est_sensors_from_plant_device(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg,
                                       const lmpc_rbd_state* d_state, const lmpc_sim_out* d_sim_out, int batch,
                                       int32_t index0, uint32_t tick, const int32_t* d_gait, int64_t gait_stride,
                                       lmpc_est_sensors* d_sensors, void* stream);
/* d_pos0 (may be NULL: the reference's default): robot b's three doubles at d_pos0 + b * pos0_stride (doubles, >= 3;
 * lmpc_rbd_state.pos with stride 36).  d_state_est, d_out may be NULL; d_shadow may be NULL, else d_sim_out is
 * required (lmpc_est_feedback). */
int lmpc_est_init_device(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg, const lmpc_est_sensors* d_sensors,
                         const double* d_pos0, int64_t pos0_stride, int batch, lmpc_est_filter* d_filter,
                         lmpc_rbd_state* d_state_est, lmpc_est_out* d_out, const lmpc_sim_out* d_sim_out,
                         lmpc_sim_out* d_shadow, void* stream);
/* One update of every robot, and in the same launch lmpc_est_feedback when d_shadow is given (d_sim_out is then
 * required; d_shadow must not alias it).  d_state_est, d_out may be NULL. */
int lmpc_est_update_device(const lmpc_rbd_model* model, const lmpc_est_cfg* cfg, const lmpc_est_sensors* d_sensors,
                           int batch, lmpc_est_filter* d_filter, lmpc_rbd_state* d_state_est, lmpc_est_out* d_out,
                           const lmpc_sim_out* d_sim_out, lmpc_sim_out* d_shadow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_EST_H */
