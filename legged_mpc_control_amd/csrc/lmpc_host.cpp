// lmpc_host.cpp -- host-side pieces of the convex-MPC QP path that sit either
// side of the device solve: robot presets, the gait-FSM contact schedule, the
// calc_mpc_reference record packing and the synthetic batch generator.
//
// Reference anchors (relative to src/legged_ctrl):
//   presets              config/gazebo_go1_convex.yaml:39-71, config/gazebo_a1_convex.yaml:40-72,133-140,
//                        src/LeggedState.cpp:146,155-160 (mass / inertia defaults)
//   gait tables          src/utils/LeggedContactFSM.cpp:93-212
//   predict_contact      src/utils/LeggedContactFSM.cpp:280-294
//   bound schedule       src/mpc_ctrl/convex_mpc/ConvexQPSolver.cpp:329-346
//   reference trajectory src/mpc_ctrl/convex_mpc/ConvexQPSolver.cpp:256-276
#include <cmath>
#include <cstring>

#include "lmpc/lmpc.h"
#include "lmpc_common.h"


extern "C" {

void lmpc_params_go1(lmpc_params* p) {
    static const double q[12] = {50.0, 100.0, 0.0, 0.0, 0.0, 3500.0, 0.01, 0.01, 10.0, 15.0, 15.0, 20.0};
    std::memset(p, 0, sizeof(*p));
    for (int i = 0; i < 12; ++i) {
        p->q_weights[i] = q[i];
        p->r_weights[i] = 1e-4;
    }
    p->robot_mass = 13.0;  // LeggedState.cpp:146 default (the Go1 sim YAML omits it)
    p->trunk_inertia[0] = 0.0158533;
    p->trunk_inertia[4] = 0.0377999;
    p->trunk_inertia[8] = 0.0456542;
    p->mu = 0.3;
    p->f_max = 180.0;
    p->gravity = 9.8;
    p->dt = 10.0 / 1000.0;
}

void lmpc_params_a1(lmpc_params* p) {
    static const double q[12] = {60.0, 100.0, 0.0, 0.0, 0.0, 450.0, 0.15, 0.15, 100.0, 3.0, 3.0, 5.0};
    lmpc_params_go1(p);
    for (int i = 0; i < 12; ++i) p->q_weights[i] = q[i];
}

void lmpc_options_default(lmpc_options* o) {
    o->max_iter = 40;
    // Hand-over to the polish at a mean complementarity of 1e-4 (was 1e-8 until round 3): with the faces
    // classified active where z > 1e-3 s (LMPC_ACT_RATIO) the polish verifies in 1.1-1.5 rounds on average,
    // so the interior point stops ~3 iterations earlier for the same verified optimum; the polish budget of
    // 8 rounds keeps the rare QP that needs 5-8 off the retry (tools/ab_opts.sh, profiles/r03/handover/).
    // Round 6: 2e-4 (profiles/r06/tol/): with the range-space polish rounds (round 5) one more round costs less than
    // the interior-point iteration it saves on the Riccati kernel -- configs 3 / 4 / 5 -1.1 / -1.4 / -2.4 %, config 2
    // unchanged over three 1024-QP windows, the same verified optima (3e-4: config 3 +7 %).
    o->max_rounds = 8;
    o->max_attempts = 3;
    o->tol_mu = 2e-4;
    o->tol_p = 1e-9;
    o->tol_d = 1e-9;
    o->gi_max_steps = 240;
    o->dense_iter_cap = 0;
    o->dense_polish_iter = 40;  // = max_iter: the polish only once the interior point has converged
    o->warm_rounds = 12;        // tools/tick_latency sweep: 4 -> 0.59 ms, 12 -> 0.35 ms per tick at H = 30
    // the certificate's dynamics check: its rounding level is <= 2e-10 of the state scale over configs 2-5 (reduced-input
    // polish stages whose W pivots sit near 1e-6 of their diagonal; tools/kkt_diag.py), a real inconsistency is O(1)
    o->tol_x = 1e-8;
}

int lmpc_record_len(int horizon) { return 33 + 12 * horizon; }
int lmpc_abi_version(void) { return LMPC_ABI_VERSION; }

const char* lmpc_strerror(int code) {
    switch (code) {
    case LMPC_OK: return "ok";
    case LMPC_ERR_ARG: return "invalid argument";
    case LMPC_ERR_DEVICE: return "HIP device error";
    case LMPC_ERR_ALLOC: return "device allocation failed";
    case LMPC_ERR_LAUNCH: return "kernel launch failed";
    case LMPC_ERR_NOT_BUILT: return "device code not available for this GPU";
    default: return "unknown error";
    }
}

int lmpc_predict_contact(int gait, int leg, double gait_phase, double gait_speed, double dt) {
    return lmpc_common::predict_contact(gait, leg, gait_phase, gait_speed, dt);
}

int lmpc_current_contact(int gait, int leg, double gait_phase) {
    return lmpc_common::current_contact(gait, leg, gait_phase);
}

int lmpc_contact_schedule(int gait, double gait_phase, double gait_speed, double dt, int horizon,
                          const uint8_t plan_contacts[4], uint8_t* contact) {
    if (horizon < 1 || !plan_contacts || !contact) return LMPC_ERR_ARG;
    for (int j = 0; j < 4; ++j) contact[j] = plan_contacts[j] ? 1 : 0;
    for (int i = 1; i < horizon; ++i)
        for (int j = 0; j < 4; ++j)
            contact[4 * i + j] = (uint8_t)lmpc_predict_contact(gait, j, gait_phase, gait_speed, i * dt);
    return LMPC_OK;
}

int lmpc_contact_schedule_legs(int gait, const double gait_phase[4], double gait_speed, double dt, int horizon,
                               const uint8_t plan_contacts[4], uint8_t* contact) {
    if (horizon < 1 || !gait_phase || !plan_contacts || !contact) return LMPC_ERR_ARG;
    for (int j = 0; j < 4; ++j) contact[j] = plan_contacts[j] ? 1 : 0;
    for (int i = 1; i < horizon; ++i)
        for (int j = 0; j < 4; ++j)
            contact[4 * i + j] = (uint8_t)lmpc_predict_contact(gait, j, gait_phase[j], gait_speed, i * dt);
    return LMPC_OK;
}

int lmpc_pack_record(const lmpc_params* p, int horizon, const lmpc_state_in* st, double* rec,
                     double lin_vel_d_world[3]) {
    if (!p || !st || !rec || horizon < 1) return LMPC_ERR_ARG;
    double* x0 = rec + LMPC_REC_X0;
    for (int k = 0; k < 3; ++k) {
        x0[k] = st->root_euler[k];
        x0[3 + k] = st->root_pos[k];
        x0[6 + k] = st->root_ang_vel[k];
        x0[9 + k] = st->root_lin_vel[k];
    }
    std::memcpy(rec + LMPC_REC_ROT, st->root_rot_mat, 9 * sizeof(double));
    std::memcpy(rec + LMPC_REC_FEET, st->foot_pos_abs, 12 * sizeof(double));
    // root_lin_vel_d_world = root_rot_mat * root_lin_vel_d_rel (ConvexQPSolver.cpp:260)
    double vdw[3];
    for (int r = 0; r < 3; ++r)
        vdw[r] = st->root_rot_mat[3 * r + 0] * st->root_lin_vel_d_rel[0] +
                 st->root_rot_mat[3 * r + 1] * st->root_lin_vel_d_rel[1] +
                 st->root_rot_mat[3 * r + 2] * st->root_lin_vel_d_rel[2];
    if (lin_vel_d_world)
        for (int r = 0; r < 3; ++r) lin_vel_d_world[r] = vdw[r];
    const double dt = p->dt;
    for (int i = 0; i < horizon; ++i) {  // ConvexQPSolver.cpp:262-276
        double* xr = rec + LMPC_REC_XREF + 12 * i;
        xr[0] = st->root_euler_d[0];
        xr[1] = st->root_euler_d[1];
        xr[2] = st->root_euler[2] + st->root_ang_vel_d_rel[2] * dt * (i);
        xr[3] = st->root_pos[0] + vdw[0] * dt * (i);
        xr[4] = st->root_pos[1] + vdw[1] * dt * (i);
        xr[5] = st->root_pos_d[2];
        xr[6] = st->root_ang_vel_d_rel[0];
        xr[7] = st->root_ang_vel_d_rel[1];
        xr[8] = st->root_ang_vel_d_rel[2];
        xr[9] = vdw[0];
        xr[10] = vdw[1];
        xr[11] = 0.0;
    }
    return LMPC_OK;
}

void lmpc_synth_cfg_go1(lmpc_synth_cfg* c) {
    // gazebo_go1_convex.yaml:18-35
    static const double feet[12] = {0.17, 0.12, -0.3, 0.17, -0.17, -0.3, -0.17, 0.17, -0.3, -0.17, -0.12, -0.3};
    std::memset(c, 0, sizeof(*c));
    c->gait = LMPC_GAIT_TROT;
    c->gait_speed = 4.0;
    std::memcpy(c->default_feet, feet, sizeof(feet));
    c->standing = 0;
}

void lmpc_synth_cfg_a1_standing(lmpc_synth_cfg* c) {
    // gazebo_a1_convex.yaml:19-36
    static const double feet[12] = {0.17, 0.17, -0.3, 0.17, -0.17, -0.3, -0.17, 0.17, -0.3, -0.17, -0.17, -0.3};
    std::memset(c, 0, sizeof(*c));
    c->gait = LMPC_GAIT_TROT;
    c->gait_speed = 3.5;
    std::memcpy(c->default_feet, feet, sizeof(feet));
    c->standing = 1;
}

int lmpc_command_to_record(const lmpc_params* p, int horizon, const lmpc_command* cmd, double* rec,
                           uint8_t* contact) {
    if (!p || !cmd || !rec || !contact || horizon < 1) return LMPC_ERR_ARG;
    lmpc_pack_record(p, horizon, &cmd->state, rec, nullptr);
    return lmpc_contact_schedule_legs(cmd->gait, cmd->gait_phase, cmd->gait_speed, p->dt, horizon, cmd->plan_contacts,
                                      contact);
}

int lmpc_synth_commands(const lmpc_synth_cfg* cfg, uint64_t seed, int64_t first_index, int count, lmpc_command* cmd) {
    if (!cfg || !cmd || count < 0) return LMPC_ERR_ARG;
    for (int b = 0; b < count; ++b) lmpc_common::synth_command(*cfg, seed, (uint64_t)(first_index + b), cmd[b]);
    return LMPC_OK;
}

int lmpc_synth_fill(const lmpc_params* p, const lmpc_synth_cfg* cfg, int horizon, uint64_t seed,
                    int64_t first_index, int count, double* rec, uint8_t* contact) {
    if (!p || !cfg || !rec || !contact || horizon < 1 || count < 0) return LMPC_ERR_ARG;
    const int rl = lmpc_record_len(horizon);
    for (int b = 0; b < count; ++b) {
        lmpc_command c;
        lmpc_common::synth_command(*cfg, seed, (uint64_t)(first_index + b), c);
        lmpc_command_to_record(p, horizon, &c, rec + (size_t)b * rl, contact + (size_t)b * 4 * horizon);
    }
    return LMPC_OK;
}

void lmpc_terrain_frame(const double nin[3], double R[9]) {
    // minimal rotation e_z -> n (Rodrigues about e_z x n, closed form); n = e_z gives I exactly
    const double nn = std::sqrt(nin[0] * nin[0] + nin[1] * nin[1] + nin[2] * nin[2]);
    const double nx = nin[0] / nn, ny = nin[1] / nn, c = nin[2] / nn;
    const double h = 1.0 / (1.0 + c);
    R[0] = 1.0 - nx * nx * h; R[1] = -nx * ny * h;      R[2] = nx;
    R[3] = -nx * ny * h;      R[4] = 1.0 - ny * ny * h; R[5] = ny;
    R[6] = -nx;               R[7] = -ny;               R[8] = c;
}

void lmpc_leg_kin_default(lmpc_leg_kin* k) {
    // BaseInterface.cpp:76-97 (and LOWER_LEG_LENGTH, LeggedParams.h:24); legs FL FR RL RR
    static const double ox[4] = {0.1805, 0.1805, -0.1805, -0.1805};
    static const double oy[4] = {0.047, -0.047, 0.047, -0.047};
    static const double mo[4] = {0.0838, -0.0838, 0.0838, -0.0838};
    for (int i = 0; i < 4; ++i) {
        k->rho_fix[i][0] = ox[i];
        k->rho_fix[i][1] = oy[i];
        k->rho_fix[i][2] = mo[i];
        k->rho_fix[i][3] = 0.21;
        k->rho_fix[i][4] = 0.21;
        k->rho_opt[i][0] = k->rho_opt[i][1] = k->rho_opt[i][2] = 0.0;
    }
}

void lmpc_foot_jacobian(const lmpc_leg_kin* k, int leg, const double q[3], double J[9]) {
    lmpc_common::foot_jacobian(k->rho_fix[leg & 3], k->rho_opt[leg & 3], q, J);
}

int lmpc_grf_to_torque(const lmpc_leg_kin* k, const double rot[9], const double joint_pos[12], const double grf0[12],
                       double tau[12]) {
    if (!k || !rot || !joint_pos || !grf0 || !tau) return LMPC_ERR_ARG;
    for (int i = 0; i < 4; ++i)
        lmpc_common::leg_torque(k->rho_fix[i], k->rho_opt[i], rot, joint_pos + 3 * i, grf0 + 3 * i, tau + 3 * i);
    return LMPC_OK;
}

// ---- the closed-loop tick on the host (include/lmpc/lmpc_rollout.h) --------
int lmpc_rollout_abi_version(void) { return LMPC_ROLLOUT_ABI_VERSION; }
int lmpc_robot_size(void) { return (int)sizeof(lmpc_robot); }

void lmpc_rollout_cfg_go1(lmpc_rollout_cfg* c) {
    lmpc_synth_cfg s;
    lmpc_synth_cfg_go1(&s);
    std::memset(c, 0, sizeof(*c));
    std::memcpy(c->default_feet, s.default_feet, sizeof(s.default_feet));
    c->swing_clearance = 0.23f;  // LeggedParams.h:27 defines it as a float
    c->foot_delta_limit[0] = c->foot_delta_limit[1] = 0.8;
    c->ground_z = 0.0;
}

int lmpc_robot_init(const lmpc_rollout_cfg* cfg, const double x0[12], const double vel_d[2], double yaw_rate,
                    double height, int gait, double gait_speed, lmpc_robot* rb) {
    if (!cfg || !x0 || !vel_d || !rb || gait < LMPC_GAIT_TROT || gait > LMPC_GAIT_STAND || !(gait_speed > 0.0))
        return LMPC_ERR_ARG;
    std::memset(rb, 0, sizeof(*rb));
    lmpc_state_in& st = rb->cmd.state;
    for (int k = 0; k < 3; ++k) {
        st.root_euler[k] = x0[k];
        st.root_pos[k] = x0[3 + k];
        st.root_ang_vel[k] = x0[6 + k];
        st.root_lin_vel[k] = x0[9 + k];
    }
    st.root_euler_d[2] = x0[2];
    st.root_pos_d[2] = height;
    st.root_lin_vel_d_rel[0] = vel_d[0];
    st.root_lin_vel_d_rel[1] = vel_d[1];
    st.root_ang_vel_d_rel[2] = yaw_rate;
    rb->cmd.gait = gait;
    rb->cmd.gait_speed = gait_speed;
    lmpc_common::euler_zyx_to_rot(x0[0], x0[1], x0[2], st.root_rot_mat);
    const double cy = std::cos(x0[2]), sy = std::sin(x0[2]);
    for (int j = 0; j < 4; ++j) {
        const double* df = cfg->default_feet + 3 * j;
        double* f = rb->foot_pos_world + 3 * j;
        f[0] = (cy * df[0] - sy * df[1]) + x0[3];
        f[1] = (sy * df[0] + cy * df[1]) + x0[4];
        f[2] = cfg->ground_z;
        for (int a = 0; a < 3; ++a) {
            rb->swing_start_world[3 * j + a] = f[a];
            st.foot_pos_abs[3 * j + a] = f[a] - x0[3 + a];
        }
        // LeggedContactFSM::reset: phase 0, the pattern's first entry
        rb->cmd.plan_contacts[j] = (uint8_t)lmpc_common::gait_table(gait, j).state[0];
    }
    return LMPC_OK;
}

static lmpc_common::PlantParams plant_params(const lmpc_params* p) {
    lmpc_common::PlantParams pp;
    pp.mass = p->robot_mass;
    for (int i = 0; i < 9; ++i) pp.Ib[i] = p->trunk_inertia[i];
    pp.grav = p->gravity;
    pp.dt = p->dt;
    return pp;
}

int lmpc_robot_plant_step(const lmpc_params* p, lmpc_robot* rb, const double u0[12]) {
    if (!p || !rb || !u0) return LMPC_ERR_ARG;
    lmpc_common::plant_step(plant_params(p), *rb, u0);
    return LMPC_OK;
}

int lmpc_robot_advance(const lmpc_params* p, const lmpc_rollout_cfg* cfg, lmpc_robot* rb, const double* u0,
                       double* foot_target) {
    if (!p || !cfg || !rb) return LMPC_ERR_ARG;
    if (u0) lmpc_common::plant_step(plant_params(p), *rb, u0);
    double target[12];
    lmpc_common::robot_bookkeep(*cfg, p->dt, *rb, target);
    if (foot_target) std::memcpy(foot_target, target, sizeof(target));
    return LMPC_OK;
}

int lmpc_synth_normals(uint64_t seed, int64_t first_index, int count, double theta_max, double* normals) {
    if (!normals || count < 0 || !(theta_max >= 0.0) || theta_max >= 1.5707963267948966) return LMPC_ERR_ARG;
    for (int b = 0; b < count; ++b)
        lmpc_common::synth_normals(seed, (uint64_t)(first_index + b), theta_max, normals + (size_t)b * 12);
    return LMPC_OK;
}

}  // extern "C"
