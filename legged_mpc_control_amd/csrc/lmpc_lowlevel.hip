// lmpc_lowlevel.hip -- the joint-PD low-level controller (include/lmpc/lmpc_lowlevel.h) on the host and on the device.
//
//   lmpc_lowlevel_kernel   one lane per (robot, leg), 64 robots per block of 256: the lane loads the base's 12 doubles,
//                          its leg's 6 joint values and its leg's 9 target doubles, runs lmpc_ll::leg
//                          (csrc/lmpc_lowlevel_common.h) and writes its 12 output doubles and one flag word; with the
//                          plant's last lmpc_sim_out given it also writes its foot's candidate flag, so that the
//                          controller and lmpc_stack_candidates_kernel are one launch.  No LDS, no cross-lane traffic.
//
// The lane's part of the configuration (its leg's rho_fix, rho_opt and gains) is read from the kernel's argument block
// by the leg's number.  That number is made opaque (the empty asm, as lmpc_sim.hip does for its model): the compiler
// then loads those values by address; knowing that the index is threadIdx.x & 3 it would instead copy the whole block
// into a private array, which lives in scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "lmpc/lmpc_lowlevel.h"
#include "lmpc_launch.h"
#include "lmpc_lowlevel_common.h"

namespace lmpc_ll {
namespace {

using lmpc_launch::launch_rc;
using lmpc_launch::PtrScope;

constexpr int THREADS = 256;
constexpr int BLOCK_ROBOTS = THREADS / 4;  // one lane per leg

__global__ void __launch_bounds__(THREADS)
    lmpc_lowlevel_kernel(const lmpc_lowlevel_cfg cfg, const lmpc_rbd_state* __restrict__ states,
                         const lmpc_wbc_target* __restrict__ targets, const int32_t* __restrict__ gaits,
                         long long gait_stride, const lmpc_sim_out* __restrict__ sim_outs, int32_t* __restrict__ cand,
                         int batch, lmpc_lowlevel_out* __restrict__ outs) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= 4 * (long long)batch) return;
    const long long b = e >> 2;
    const int l = (int)(e & 3);
    int lo = l;
    asm volatile("" : "+v"(lo));
    LegCfg c;
    leg_cfg(cfg, lo, c);
    LegIn in;
    leg_in(states[b], targets[b], l, in);
    const int mode = gaits && gaits[b * gait_stride] == LMPC_GAIT_STAND ? 0 : 1;
    LegOut o;
    leg(c, in, mode, o);
    leg_store(o, l, outs[b]);
    if (cand) cand[e] = candidate(sim_outs[b].held[l], sim_outs[b].touch[l]);
}

void cfg_preset(lmpc_lowlevel_cfg* c, double kp, double kd) {
    std::memset(c, 0, sizeof(*c));
    lmpc_leg_kin_default(&c->kin);
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 3; ++k) c->kp[l][k] = kp, c->kd[l][k] = kd;
}

}  // namespace
}  // namespace lmpc_ll

using namespace lmpc_ll;

extern "C" {

int lmpc_lowlevel_abi_version(void) { return LMPC_LOWLEVEL_ABI_VERSION; }
int lmpc_lowlevel_cfg_size(void) { return (int)sizeof(lmpc_lowlevel_cfg); }
int lmpc_lowlevel_out_size(void) { return (int)sizeof(lmpc_lowlevel_out); }
int lmpc_lowlevel_block_robots(void) { return BLOCK_ROBOTS; }

void lmpc_lowlevel_cfg_go1(lmpc_lowlevel_cfg* c) {
    if (c) cfg_preset(c, 0.5, 0.3);  // gazebo_go1_convex.yaml:74-80
}
void lmpc_lowlevel_cfg_a1(lmpc_lowlevel_cfg* c) {
    if (c) cfg_preset(c, 15.0, 0.4);  // gazebo_a1_convex.yaml:75-81
}

int lmpc_leg_kin_from_model(const lmpc_rbd_model* m, lmpc_leg_kin* kin) {
    if (!m || !kin) return LMPC_ERR_ARG;
    lmpc_leg_kin k;
    for (int l = 0; l < 4; ++l) {
        const double* hip = m->joint_origin[3 * l];
        const double* thigh = m->joint_origin[3 * l + 1];
        const double* calf = m->joint_origin[3 * l + 2];
        const double* foot = m->foot[l];
        const double rest[7] = {hip[2], thigh[0], thigh[2], calf[0], calf[1], foot[0], foot[1]};
        for (double r : rest)
            if (!(std::fabs(r) <= 1e-12)) return LMPC_ERR_ARG;
        k.rho_fix[l][0] = hip[0], k.rho_fix[l][1] = hip[1], k.rho_fix[l][2] = thigh[1];
        k.rho_fix[l][3] = -calf[2], k.rho_fix[l][4] = -foot[2];
        k.rho_opt[l][0] = k.rho_opt[l][1] = k.rho_opt[l][2] = 0.0;
    }
    *kin = k;
    return LMPC_OK;
}

int lmpc_leg_fk(const lmpc_leg_kin* kin, int leg, const double q[3], double p[3]) {
    if (!kin || !q || !p || leg < 0 || leg > 3) return LMPC_ERR_ARG;
    const double qq[3] = {q[0], q[1], q[2]};
    fk(kin->rho_fix[leg], kin->rho_opt[leg], qq, p);
    return LMPC_OK;
}

int lmpc_leg_inv_kin(const lmpc_leg_kin* kin, int leg, const double p[3], const double cur_q[3], double q[3]) {
    if (!kin || !p || !cur_q || !q || leg < 0 || leg > 3) return LMPC_ERR_ARG;
    const double pp[3] = {p[0], p[1], p[2]}, cur[3] = {cur_q[0], cur_q[1], cur_q[2]};
    inv_kin(kin->rho_fix[leg], pp, cur, q);
    return LMPC_OK;
}

int lmpc_lowlevel(const lmpc_lowlevel_cfg* cfg, const lmpc_rbd_state* state, const lmpc_wbc_target* target,
                  const int32_t* gait, lmpc_lowlevel_out* out) {
    if (!cfg || !state || !target || !out) return LMPC_ERR_ARG;
    const int mode = gait && *gait == LMPC_GAIT_STAND ? 0 : 1;
    lmpc_lowlevel_out r;  // a copy: `out` may overlap the inputs
    robot(*cfg, *state, *target, mode, r);
    *out = r;
    return LMPC_OK;
}

int lmpc_lowlevel_device(const lmpc_lowlevel_cfg* cfg, const lmpc_rbd_state* d_state, const lmpc_wbc_target* d_target,
                         const int32_t* d_gait, int64_t gait_stride, const lmpc_sim_out* d_sim_out,
                         int32_t* d_candidates, int batch, lmpc_lowlevel_out* d_out, void* stream) {
    if (batch < 0 || (batch > 0 && (!cfg || !d_state || !d_target || !d_out || (d_gait && gait_stride < 1) ||
                                    (d_sim_out == nullptr) != (d_candidates == nullptr))))
        return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipStream_t s = (hipStream_t)stream;
    PtrScope ps(d_state, s);
    if (!ps.ok) return LMPC_ERR_ARG;
    const long long n = 4 * (long long)batch;
    hipLaunchKernelGGL(lmpc_lowlevel_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, *cfg,
                       d_state, d_target, d_gait, (long long)gait_stride, d_sim_out, d_candidates, batch, d_out);
    return launch_rc(hipGetLastError());
}

}  // extern "C"
