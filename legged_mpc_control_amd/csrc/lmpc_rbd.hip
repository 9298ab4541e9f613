// lmpc_rbd.hip -- floating-base rigid-body dynamics for the WBC (include/lmpc/lmpc_rbd.h): robot state -> M, nle, J,
// dJv, base_accel, swing_acc, on the host (one robot) and on the device (a batch, four lanes per robot).
//
// The arithmetic is lmpc_rbd_common.h's, compiled for both sides.  Device mapping: lane 4 r + l of a wavefront owns
// leg l of the wavefront's r-th robot (16 robots per wavefront): its forward kinematics, composite
// bodies, the leg's 3 x 3 block of M, the 6 x 3 coupling block, its three Jacobian rows and dJv.  The base block and
// nle[0:6] need every leg's totals (16 doubles): the four lanes of a quad exchange them by shuffles and each sums
// trunk, FL, FR, RL, RR in that order, so all four hold the same bits and split the base block's stores between
// them.  Every entry of the output block is written (the structural zeros of M and J included), straight from
// registers: the kernel has no LDS, no scratch, and no 18 x 18 matrix in any lane.
#include <hip/hip_runtime.h>

#include "lmpc/lmpc_rbd.h"
#include "lmpc_rbd_common.h"
#include "lmpc_quad_device.h"

static_assert(sizeof(lmpc_rbd_model) == 179 * 8, "lmpc_rbd_model layout (legged_mpc_control_amd/_native.py)");
static_assert(sizeof(lmpc_rbd_state) == 36 * 8, "lmpc_rbd_state layout");
static_assert(sizeof(lmpc_wbc_target) == 352, "lmpc_wbc_target layout");
static_assert(sizeof(lmpc_rbd_terms) == 634 * 8, "lmpc_rbd_terms layout");
static_assert(sizeof(lmpc_wbc_input) == 4848, "lmpc_wbc_input layout");

namespace lmpc_rbd {
namespace {

constexpr int NQ = 18;
using lmpc_sim::BLOCK;  // the quad layout and its measurement: lmpc_quad_device.h
using lmpc_sim::BLOCK_ROBOTS;
using lmpc_sim::quad_grid;

// The part of an output block (lmpc_wbc_input or lmpc_rbd_terms: M, nle, J, dJv) that leg L alone determines.
template <class Out>
LMPC_HD inline void store_leg(Out& o, int L, const LegOut& g) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o.M[r * NQ + 6 + 3 * L + c] = g.Mbl[r][c];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int row = 6 + 3 * L + i;
#pragma unroll
        for (int c = 0; c < 6; ++c) o.M[row * NQ + c] = g.Mbl[c][i];
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int c = 0; c < 3; ++c) o.M[row * NQ + 6 + 3 * l + c] = l == L ? g.Mll[i][c] : 0.0;
        o.nle[row] = g.nle[i];
        const int jr = 3 * L + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) o.J[jr * NQ + c] = c == i ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) o.J[jr * NQ + 3 + c] = g.Jb[i][c];
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int c = 0; c < 3; ++c) o.J[jr * NQ + 6 + 3 * l + c] = l == L ? g.Jl[i][c] : 0.0;
    }
    o.dJv[3 * L] = g.dJv.x, o.dJv[3 * L + 1] = g.dJv.y, o.dJv[3 * L + 2] = g.dJv.z;
}

// Ab, row-major 6 x 6
LMPC_HD inline void centroidal_block(const BaseOut& b, double ab[36]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            ab[r * 6 + c] = b.Mbb[r][c];
            ab[(3 + r) * 6 + c] = c < 3 ? 0.0 : b.Aw[r][c - 3];
        }
}

// ---- host: one robot, the legs in a loop ---------------------------------------------------------------------
struct HostRobot {
    BaseKin bk;
    LegOut leg[4];
    BaseOut base;
};

void host_robot(const lmpc_rbd_model& md, const lmpc_rbd_state& st, HostRobot& h) {
    h.bk = base_kin(st);
    for (int l = 0; l < 4; ++l) leg_pass(md, st, h.bk, l, h.leg[l]);
    base_pass(h.bk, total_part(trunk_part(md, h.bk), h.leg[0].sum, h.leg[1].sum, h.leg[2].sum, h.leg[3].sum), h.base);
}

template <class Out>
void host_store_common(Out& o, const HostRobot& h) {
    for (int l = 0; l < 4; ++l) store_leg(o, l, h.leg[l]);
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) o.M[r * NQ + c] = h.base.Mbb[r][c];
        o.nle[r] = h.base.nle[r];
    }
}

// ---- device ----------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
using lmpc_sim::quad_get;

// v[0..N) is held identically by the four lanes of a quad: lane l stores the entries e = l, l + 4, ... at
// dst[(e / W) * ld + e % W] (a W-wide block of a matrix with leading dimension ld; W = N, ld = 0 for a vector)
template <int N, int W>
__device__ inline void quad_store(double* dst, int ld, const double* v, int l, bool active) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const double a = v[i], b = v[i + 1 < N ? i + 1 : i], c = v[i + 2 < N ? i + 2 : i], d = v[i + 3 < N ? i + 3 : i];
        const double pick = l == 0 ? a : l == 1 ? b : l == 2 ? c : d;
        const int e = i + l;
        if (active && e < N) dst[(e / W) * ld + e % W] = pick;
    }
}

// One lane per leg.  WBC = true: lmpc_wbc_input blocks (tg, the targets); false: lmpc_rbd_terms blocks.
template <bool WBC, class Out>
__global__ void __launch_bounds__(BLOCK) lmpc_rbd_kernel(const lmpc_rbd_model md, const lmpc_rbd_state* __restrict__ states,
                                                       const lmpc_wbc_target* __restrict__ targets, int batch,
                                                       Out* __restrict__ outs) {
    const int robot = blockIdx.x * BLOCK_ROBOTS + (threadIdx.x >> 2), L = threadIdx.x & 3;
    // a quad past the batch computes the last robot again and stores nothing: the shuffles below stay uniform
    const bool active = robot < batch;
    const int r = active ? robot : batch - 1;
    const lmpc_rbd_state& st = states[r];
    Out& o = outs[r];

    const BaseKin bk = base_kin(st);
    LegOut g;
    leg_pass(md, st, bk, L, g);
    if (active) store_leg(o, L, g);

    BaseOut base;
    base_pass(bk, total_part(trunk_part(md, bk), quad_get(g.sum, 0), quad_get(g.sum, 1), quad_get(g.sum, 2),
                             quad_get(g.sum, 3)), base);
    quad_store<36, 6>(o.M, NQ, &base.Mbb[0][0], L, active);
    quad_store<6, 6>(o.nle, 0, base.nle, L, active);

    const V3 pos = v3(st.pos[0], st.pos[1], st.pos[2]);
    const V3 foot = add(pos, g.foot);
    if constexpr (WBC) {
        const lmpc_wbc_target& t = targets[r];
        const V3 m = foot_moment(g.foot, base.com, &t.forces_des[3 * L]);
        const V3 mom = add(add(add(quad_get(m, 0), quad_get(m, 1)), quad_get(m, 2)), quad_get(m, 3));
        double b[6];
        base_accel(bk, base, md.gravity, t.forces_des, mom, b);
        quad_store<6, 6>(o.base_accel, 0, b, L, active);
        if (active) {
            const double kp = t.swing_kp, kd = t.swing_kd;
            o.swing_acc[3 * L] = swing_accel(kp, kd, t.foot_pos_des[3 * L], foot.x, t.foot_vel_des[3 * L], g.foot_vel.x);
            o.swing_acc[3 * L + 1] =
                swing_accel(kp, kd, t.foot_pos_des[3 * L + 1], foot.y, t.foot_vel_des[3 * L + 1], g.foot_vel.y);
            o.swing_acc[3 * L + 2] =
                swing_accel(kp, kd, t.foot_pos_des[3 * L + 2], foot.z, t.foot_vel_des[3 * L + 2], g.foot_vel.z);
#pragma unroll
            for (int i = 0; i < 3; ++i) o.forces_des[3 * L + i] = t.forces_des[3 * L + i];
            if (L < 3) o.torque_limits[L] = t.torque_limits[L];
            else o.mu = t.mu;
            o.contact[L] = t.contact[L];
        }
    } else {
        if (active) {
            o.foot_pos[3 * L] = foot.x, o.foot_pos[3 * L + 1] = foot.y, o.foot_pos[3 * L + 2] = foot.z;
            o.foot_vel[3 * L] = g.foot_vel.x, o.foot_vel[3 * L + 1] = g.foot_vel.y, o.foot_vel[3 * L + 2] = g.foot_vel.z;
        }
        double ab[36];
        centroidal_block(base, ab);
        quad_store<36, 36>(o.Ab, 0, ab, L, active);
        const V3 com = add(pos, base.com);
        const double tail[4] = {com.x, com.y, com.z, base.mass};
        // com[3] and mass are four doubles, 36 apart: one per lane
        if (active) (L < 3 ? o.com[L] : o.mass) = L == 0 ? tail[0] : L == 1 ? tail[1] : L == 2 ? tail[2] : tail[3];
    }
}
#endif

}  // namespace
}  // namespace lmpc_rbd

using namespace lmpc_rbd;

extern "C" int lmpc_rbd_abi_version(void) { return LMPC_RBD_ABI_VERSION; }
extern "C" int lmpc_rbd_model_size(void) { return (int)sizeof(lmpc_rbd_model); }
extern "C" int lmpc_rbd_state_size(void) { return (int)sizeof(lmpc_rbd_state); }
extern "C" int lmpc_wbc_target_size(void) { return (int)sizeof(lmpc_wbc_target); }
extern "C" int lmpc_rbd_terms_size(void) { return (int)sizeof(lmpc_rbd_terms); }

extern "C" void lmpc_wbc_target_default(lmpc_wbc_target* t) {
    if (!t) return;
    *t = lmpc_wbc_target{};
    t->torque_limits[0] = t->torque_limits[1] = t->torque_limits[2] = 33.5;
    t->mu = 0.3;
    t->swing_kp = 350.0;
    t->swing_kd = 37.0;
    for (int i = 0; i < 4; ++i) t->contact[i] = 1;
}

extern "C" int lmpc_rbd_compute(const lmpc_rbd_model* model, const lmpc_rbd_state* state, lmpc_rbd_terms* terms) {
    if (!model || !state || !terms) return LMPC_ERR_ARG;
    HostRobot h;
    host_robot(*model, *state, h);
    host_store_common(*terms, h);
    for (int l = 0; l < 4; ++l) {
        const V3 foot = add(v3(state->pos[0], state->pos[1], state->pos[2]), h.leg[l].foot);
        terms->foot_pos[3 * l] = foot.x, terms->foot_pos[3 * l + 1] = foot.y, terms->foot_pos[3 * l + 2] = foot.z;
        terms->foot_vel[3 * l] = h.leg[l].foot_vel.x, terms->foot_vel[3 * l + 1] = h.leg[l].foot_vel.y;
        terms->foot_vel[3 * l + 2] = h.leg[l].foot_vel.z;
    }
    const V3 com = add(v3(state->pos[0], state->pos[1], state->pos[2]), h.base.com);
    terms->com[0] = com.x, terms->com[1] = com.y, terms->com[2] = com.z;
    centroidal_block(h.base, terms->Ab);
    terms->mass = h.base.mass;
    return LMPC_OK;
}

extern "C" int lmpc_wbc_input_from_state(const lmpc_rbd_model* model, const lmpc_rbd_state* state,
                                         const lmpc_wbc_target* target, lmpc_wbc_input* in) {
    if (!model || !state || !target || !in) return LMPC_ERR_ARG;
    HostRobot h;
    host_robot(*model, *state, h);
    host_store_common(*in, h);
    const V3 pos = v3(state->pos[0], state->pos[1], state->pos[2]);
    V3 mom = foot_moment(h.leg[0].foot, h.base.com, &target->forces_des[0]);
    for (int l = 1; l < 4; ++l) mom = add(mom, foot_moment(h.leg[l].foot, h.base.com, &target->forces_des[3 * l]));
    base_accel(h.bk, h.base, model->gravity, target->forces_des, mom, in->base_accel);
    for (int l = 0; l < 4; ++l) {
        const V3 foot = add(pos, h.leg[l].foot);
        const double p[3] = {foot.x, foot.y, foot.z}, v[3] = {h.leg[l].foot_vel.x, h.leg[l].foot_vel.y, h.leg[l].foot_vel.z};
        for (int i = 0; i < 3; ++i)
            in->swing_acc[3 * l + i] = swing_accel(target->swing_kp, target->swing_kd, target->foot_pos_des[3 * l + i], p[i],
                                                   target->foot_vel_des[3 * l + i], v[i]);
        in->contact[l] = target->contact[l];
    }
    for (int i = 0; i < 12; ++i) in->forces_des[i] = target->forces_des[i];
    for (int i = 0; i < 3; ++i) in->torque_limits[i] = target->torque_limits[i];
    in->mu = target->mu;
    return LMPC_OK;
}

extern "C" int lmpc_wbc_inputs_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state,
                                      const lmpc_wbc_target* d_target, int batch, lmpc_wbc_input* d_in, void* stream) {
    if (batch < 0 || (batch > 0 && (!model || !d_state || !d_target || !d_in))) return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipLaunchKernelGGL((lmpc_rbd_kernel<true, lmpc_wbc_input>), quad_grid(batch), dim3(BLOCK), 0, (hipStream_t)stream,
                       *model, d_state, d_target, batch, d_in);
    return hipGetLastError() == hipSuccess ? LMPC_OK : LMPC_ERR_LAUNCH;
}

extern "C" int lmpc_rbd_compute_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state, int batch,
                                       lmpc_rbd_terms* d_terms, void* stream) {
    if (batch < 0 || (batch > 0 && (!model || !d_state || !d_terms))) return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipLaunchKernelGGL((lmpc_rbd_kernel<false, lmpc_rbd_terms>), quad_grid(batch), dim3(BLOCK), 0,
                       (hipStream_t)stream, *model, d_state, (const lmpc_wbc_target*)nullptr, batch, d_terms);
    return hipGetLastError() == hipSuccess ? LMPC_OK : LMPC_ERR_LAUNCH;
}

// ---- presets: tests/golden/rbd_model_go1.json / rbd_model_a1.json (tools/urdf_to_rbd.py on the reference's URDFs) ----
namespace {

struct LegLink {
    double mass, com[3], inertia[6];
};

// One robot from its trunk, the three links of the front-left leg and the mirror signs of the others: in both URDFs
// a right leg is the left one with y -> -y (com y, ixy, iyz change sign) and a rear hip is the front one with
// x -> -x (com x, ixy, ixz change sign); thighs and calves are shared front / rear.
void fill_model(lmpc_rbd_model* m, const LegLink& trunk, const LegLink (&fl)[3], const double (&hip_origin)[3],
                double thigh_y, double calf_z, double foot_z) {
    *m = lmpc_rbd_model{};
    m->gravity = 9.81;
    m->mass[0] = trunk.mass;
    for (int i = 0; i < 3; ++i) m->com[0][i] = trunk.com[i];
    for (int i = 0; i < 6; ++i) m->inertia[0][i] = trunk.inertia[i];
    for (int leg = 0; leg < 4; ++leg) {
        const double sy = (leg & 1) ? -1.0 : 1.0, sx = (leg & 2) ? -1.0 : 1.0;
        for (int k = 0; k < 3; ++k) {
            const int b = 1 + 3 * leg + k;
            const double fx = k == 0 ? sx : 1.0;  // only the hip link is mirrored front / rear
            m->mass[b] = fl[k].mass;
            m->com[b][0] = fx * fl[k].com[0], m->com[b][1] = sy * fl[k].com[1], m->com[b][2] = fl[k].com[2];
            m->inertia[b][0] = fl[k].inertia[0];
            m->inertia[b][1] = fx * sy * fl[k].inertia[1];
            m->inertia[b][2] = fx * fl[k].inertia[2];
            m->inertia[b][3] = fl[k].inertia[3];
            m->inertia[b][4] = sy * fl[k].inertia[4];
            m->inertia[b][5] = fl[k].inertia[5];
        }
        m->joint_origin[3 * leg][0] = sx * hip_origin[0];
        m->joint_origin[3 * leg][1] = sy * hip_origin[1];
        m->joint_origin[3 * leg][2] = hip_origin[2];
        m->joint_origin[3 * leg + 1][1] = sy * thigh_y;
        m->joint_origin[3 * leg + 2][2] = calf_z;
        m->foot[leg][2] = foot_z;
    }
}

}  // namespace

extern "C" void lmpc_rbd_model_go1(lmpc_rbd_model* m) {
    if (!m) return;
    const LegLink trunk = {5.205079999999997,
                           {0.022293292129996093, 0.00198686379460066, -0.0005012683570665583},
                           {0.016948277249411392, 0.0004609724963506115, 0.00023659727866468696, 0.06571881401409414,
                            3.628894887391443e-05, 0.07438866932990668}};
    const LegLink fl[3] = {
        {0.591, {-0.00541, -0.00074, 6e-06},
         {0.000374268192, 3.6844422e-05, -9.86754e-07, 0.000635923669, -1.172894e-06, 0.000457647394}},
        {0.92, {-0.003468, -0.018947, -0.032736},
         {0.005851561134, 1.783284e-06, 0.000328291374, 0.005596155105, 2.1430713e-05, 0.00107157026}},
        {0.191, {0.004311340314136125, 0.0008964240837696335, -0.15077088481675394},
         {0.0032876231855581152, 1.102803692565445e-06, -0.0001288298830825131, 0.0033057620060943454,
          -2.927775921267016e-05, 4.1569734689528786e-05}}};
    const double hip[3] = {0.1881, 0.04675, 0.0};
    fill_model(m, trunk, fl, hip, 0.08, -0.213, -0.213);
    // Go1's calf (with its foot lumped in) is the same link on all four legs, not mirrored
    for (int leg = 0; leg < 4; ++leg) {
        const int b = 3 + 3 * leg;
        m->com[b][1] = fl[2].com[1];
        m->inertia[b][1] = fl[2].inertia[1];
        m->inertia[b][4] = fl[2].inertia[4];
    }
}

extern "C" void lmpc_rbd_model_a1(lmpc_rbd_model* m) {
    if (!m) return;
    const LegLink trunk = {6.01,
                           {0.0, 0.004093178036605658, -0.0004991680532445924},
                           {0.01585447031613977, -3.66e-05, -6.11e-05, 0.03780090249584026, -2.7479534109816974e-05,
                            0.0456553678202995}};
    const LegLink fl[3] = {
        {0.595, {-0.003875, 0.001622, 4.2e-05}, {0.000402747, -8.709e-06, -2.97e-07, 0.000691123, -5.45e-07, 0.000487919}},
        {0.888, {-0.003574, -0.019529, -0.030323}, {0.005251806, -2.168e-06, 0.000346889, 0.005000475, -2.8174e-05, 0.0011102}},
        {0.211, {0.005084620853080569, -0.00017103791469194314, -0.1262411516587678},
         {0.0028104866460028437, 7.291346303317537e-08, -0.0001727183970478673, 0.002828648767188815,
          1.0577018852132702e-06, 4.292802655336493e-05}}};
    const double hip[3] = {0.1805, 0.047, 0.0};
    fill_model(m, trunk, fl, hip, 0.0838, -0.2, -0.2);
    // A1's calf is the same link on all four legs, not mirrored
    for (int leg = 0; leg < 4; ++leg) {
        const int b = 3 + 3 * leg;
        m->com[b][1] = fl[2].com[1];
        m->inertia[b][1] = fl[2].inertia[1];
        m->inertia[b][4] = fl[2].inertia[4];
    }
}
