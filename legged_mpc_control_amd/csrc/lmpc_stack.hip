// lmpc_stack.hip -- the MPC tick of the full loop (include/lmpc/lmpc_stack.h) on the host and on the device.
//
//   lmpc_stack_advance_kernel     one thread per robot on the first 16 lanes of a block: feedback from the measured
//                                 state and the plant's output, Raibert target, the leg FSMs with early touchdown and
//                                 their foot targets (csrc/lmpc_stack_common.h); then the block's 256 threads expand
//                                 its robots' commands into the records and contact schedules the solve reads, one
//                                 thread per element (what lmpc_records_kernel does, by the same lmpc_common
//                                 functions) -- the shape of lmpc_rollout.hip's lmpc_advance_kernel
//   lmpc_stack_targets_kernel     one thread per 8-byte word of lmpc_wbc_target: u_0 read by stride from the
//                                 solver's [B][H][12] output, the FSM targets, the template's constants, plan_contacts
//   lmpc_stack_candidates_kernel  one thread per foot: held | touch of the plant's last step
//
// All three are tiny HBM-bound maps between the solves (960 B in and out per robot and MPC tick for the advance).
// The entry points that use an MPC context's buffers (lmpc_stack_advance_device, lmpc_stack_solve_device,
// lmpc_stack_copy_records_device) are in lmpc_capi.cpp, where the context is defined.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "lmpc/lmpc_stack.h"
#include "lmpc_launch.h"
#include "lmpc_stack_common.h"

namespace lmpc {

constexpr int SADV_THREADS = 256;
constexpr int SADV_ROBOTS = 16;  // robots per block: their advance on the first 16 lanes, their expansion on all 256
constexpr int TGT_WORDS = (int)(sizeof(lmpc_wbc_target) / 8);  // 44

// Copies of the robot by 8-byte words: a struct assignment leaves the fields the advance never touches as byte blocks
// that travel from the load to the store through scratch; as words they stay in registers.
typedef unsigned long long __attribute__((may_alias)) word_t;
template <int BYTES>
__device__ inline void copy_words(void* dst, const void* src) {
    static_assert(BYTES % 8 == 0, "whole words");
#pragma unroll
    for (int i = 0; i < BYTES / 8; ++i) static_cast<word_t*>(dst)[i] = static_cast<const word_t*>(src)[i];
}

__global__ void __launch_bounds__(SADV_THREADS)
    lmpc_stack_advance_kernel(double dt, lmpc_rollout_cfg cfg, lmpc_stack_robot* __restrict__ robots,
                              const lmpc_rbd_state* __restrict__ states, const lmpc_sim_out* __restrict__ outs,
                              int batch, int H, double* __restrict__ rec, uint8_t* __restrict__ contact) {
    __shared__ lmpc_command sh[SADV_ROBOTS];
    const int base = blockIdx.x * SADV_ROBOTS;
    const int b = base + (int)threadIdx.x;
    if (threadIdx.x < SADV_ROBOTS && b < batch) {
        lmpc_stack_robot sr;
        copy_words<sizeof(lmpc_stack_robot)>(&sr, robots + b);
        const lmpc_rbd_state rs = states[b];
        double fp[12];
        int32_t tc[4];
#pragma unroll
        for (int e = 0; e < 12; ++e) fp[e] = outs[b].foot_pos[e];
#pragma unroll
        for (int l = 0; l < 4; ++l) tc[l] = outs[b].touch[l];
        lmpc_stack::advance(cfg, dt, sr, rs, fp, tc, nullptr);
        copy_words<sizeof(lmpc_command)>(sh + threadIdx.x, &sr.rb.cmd);
        copy_words<sizeof(lmpc_stack_robot)>(robots + b, &sr);
    }
    __syncthreads();
    const int n = batch - base < SADV_ROBOTS ? batch - base : SADV_ROBOTS;  // robots of this block
    const int RL = LMPC_REC_XREF + 12 * H, CL = 4 * H;
    for (int e = (int)threadIdx.x; e < n * (RL + CL); e += SADV_THREADS) {
        if (e < n * RL) {
            const int r = e / RL, i = e - r * RL;
            rec[(size_t)(base + r) * RL + i] = lmpc_common::record_element(sh[r].state, dt, i);
        } else {
            const int c = e - n * RL, r = c / CL, k = c - r * CL;
            contact[(size_t)(base + r) * CL + k] = lmpc_common::contact_element(sh[r], dt, k >> 2, k & 3);
        }
    }
}

__global__ void __launch_bounds__(256)
    lmpc_stack_targets_kernel(const lmpc_stack_robot* __restrict__ robots, const double* __restrict__ grf,
                              long long grf_stride, lmpc_wbc_target tmpl, int batch,
                              lmpc_wbc_target* __restrict__ targets) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)batch * TGT_WORDS) return;
    const int r = (int)(e / TGT_WORDS), w = (int)(e - (long long)r * TGT_WORDS);
    const lmpc_stack_robot& sr = robots[r];
    if (w < 42) {
        reinterpret_cast<double*>(targets + r)[w] = lmpc_stack::targets_word(sr, grf + (long long)r * grf_stride, tmpl, w);
    } else {
        const int l = 2 * (w - 42);
        targets[r].contact[l] = lmpc_stack::targets_contact(sr, l);
        targets[r].contact[l + 1] = lmpc_stack::targets_contact(sr, l + 1);
    }
}

__global__ void __launch_bounds__(256)
    lmpc_stack_candidates_kernel(const lmpc_sim_out* __restrict__ outs, int batch, int32_t* __restrict__ cand) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * batch) return;
    const lmpc_sim_out& o = outs[e >> 2];
    cand[e] = (o.held[e & 3] | o.touch[e & 3]) != 0 ? 1 : 0;
}

hipError_t launch_stack_advance(double dt, const lmpc_rollout_cfg& cfg, lmpc_stack_robot* robots,
                                const lmpc_rbd_state* states, const lmpc_sim_out* outs, int batch, int H, double* rec,
                                uint8_t* contact, hipStream_t stream) {
    hipLaunchKernelGGL(lmpc_stack_advance_kernel, dim3((batch + SADV_ROBOTS - 1) / SADV_ROBOTS), dim3(SADV_THREADS), 0,
                       stream, dt, cfg, robots, states, outs, batch, H, rec, contact);
    return hipGetLastError();
}

}  // namespace lmpc

using lmpc_launch::launch_rc;
using lmpc_launch::PtrScope;

extern "C" {

int lmpc_stack_abi_version(void) { return LMPC_STACK_ABI_VERSION; }
int lmpc_stack_robot_size(void) { return (int)sizeof(lmpc_stack_robot); }

int lmpc_stack_check_rates(const lmpc_params* p, const lmpc_sim_cfg* sc, int wbc_per_mpc, int substeps) {
    if (!p || !sc || wbc_per_mpc < 1 || substeps < 1) return LMPC_ERR_ARG;
    const double d = (double)wbc_per_mpc * (double)substeps * sc->dt - p->dt;
    return std::isfinite(d) && std::fabs(d) <= 1e-12 ? LMPC_OK : LMPC_ERR_ARG;
}

int lmpc_stack_robot_init(const lmpc_rollout_cfg* cfg, const lmpc_rbd_model* model, const lmpc_rbd_state* state,
                          const double vel_d[2], double yaw_rate, double height, int gait, double gait_speed,
                          lmpc_stack_robot* sr, lmpc_sim_out* first_out) {
    if (!cfg || !model || !state || !vel_d || !sr || !first_out || gait < LMPC_GAIT_TROT || gait > LMPC_GAIT_STAND ||
        !(gait_speed > 0.0))
        return LMPC_ERR_ARG;
    lmpc_rbd_terms terms;
    const int rc = lmpc_rbd_compute(model, state, &terms);
    if (rc != LMPC_OK) return rc;
    std::memset(sr, 0, sizeof(*sr));
    std::memset(first_out, 0, sizeof(*first_out));
    lmpc_command& c = sr->rb.cmd;
    lmpc_state_in& st = c.state;
    st.root_euler[0] = state->euler[2];
    st.root_euler[1] = state->euler[1];
    st.root_euler[2] = state->euler[0];
    for (int k = 0; k < 3; ++k) {
        st.root_pos[k] = state->pos[k];
        st.root_ang_vel[k] = state->omega[k];
        st.root_lin_vel[k] = state->lin_vel[k];
    }
    st.root_euler_d[2] = state->euler[0];
    st.root_pos_d[2] = height;
    st.root_lin_vel_d_rel[0] = vel_d[0];
    st.root_lin_vel_d_rel[1] = vel_d[1];
    st.root_ang_vel_d_rel[2] = yaw_rate;
    c.gait = gait;
    c.gait_speed = gait_speed;
    lmpc_common::euler_zyx_to_rot(st.root_euler[0], st.root_euler[1], st.root_euler[2], st.root_rot_mat);
    for (int j = 0; j < 4; ++j) {
        for (int a = 0; a < 3; ++a) {
            const double f = terms.foot_pos[3 * j + a];
            first_out->foot_pos[3 * j + a] = f;
            sr->rb.foot_pos_world[3 * j + a] = f;
            sr->rb.swing_start_world[3 * j + a] = f;
            sr->swing_end_world[3 * j + a] = f;
            sr->fsm_pos_target[3 * j + a] = f;
            st.foot_pos_abs[3 * j + a] = f - state->pos[a];
        }
        const int on = terms.foot_pos[3 * j + 2] <= cfg->ground_z + 1e-9 ? 1 : 0;
        first_out->touch[j] = first_out->held[j] = on;
        // LeggedContactFSM::reset: phase 0, the pattern's first entry
        c.plan_contacts[j] = (uint8_t)lmpc_common::gait_table(gait, j).state[0];
    }
    return LMPC_OK;
}

int lmpc_stack_advance(const lmpc_params* p, const lmpc_rollout_cfg* cfg, lmpc_stack_robot* sr,
                       const lmpc_rbd_state* state, const lmpc_sim_out* out, double* foot_target) {
    if (!p || !cfg || !sr || !state || !out || !(p->dt > 0.0)) return LMPC_ERR_ARG;
    // copies: `state` / `out` may be read after the robot has been written
    const lmpc_rbd_state rs = *state;
    double fp[12];
    int32_t tc[4];
    std::memcpy(fp, out->foot_pos, sizeof(fp));
    std::memcpy(tc, out->touch, sizeof(tc));
    lmpc_stack::advance(*cfg, p->dt, *sr, rs, fp, tc, foot_target);
    return LMPC_OK;
}

int lmpc_stack_targets(const lmpc_stack_robot* sr, const double u0[12], const lmpc_wbc_target* tmpl,
                       lmpc_wbc_target* target) {
    if (!sr || !u0 || !tmpl || !target) return LMPC_ERR_ARG;
    lmpc_wbc_target t;
    double* w = reinterpret_cast<double*>(&t);
    for (int i = 0; i < 42; ++i) w[i] = lmpc_stack::targets_word(*sr, u0, *tmpl, i);
    for (int l = 0; l < 4; ++l) t.contact[l] = lmpc_stack::targets_contact(*sr, l);
    *target = t;
    return LMPC_OK;
}

int lmpc_stack_targets_device(const lmpc_stack_robot* d_robots, const double* d_grf, int64_t grf_stride,
                              const lmpc_wbc_target* tmpl, int batch, lmpc_wbc_target* d_target, void* stream) {
    if (batch < 0 || (batch > 0 && (!d_robots || !d_grf || !tmpl || !d_target || grf_stride < 12))) return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipStream_t s = (hipStream_t)stream;
    PtrScope ps(d_robots, s);
    if (!ps.ok) return LMPC_ERR_ARG;
    const long long n = (long long)batch * lmpc::TGT_WORDS;
    hipLaunchKernelGGL(lmpc::lmpc_stack_targets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_robots, d_grf,
                       (long long)grf_stride, *tmpl, batch, d_target);
    return launch_rc(hipGetLastError());
}

int lmpc_stack_candidates_device(const lmpc_sim_out* d_sim_out, int batch, int32_t* d_candidates, void* stream) {
    if (batch < 0 || (batch > 0 && (!d_sim_out || !d_candidates))) return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipStream_t s = (hipStream_t)stream;
    PtrScope ps(d_sim_out, s);
    if (!ps.ok) return LMPC_ERR_ARG;
    hipLaunchKernelGGL(lmpc::lmpc_stack_candidates_kernel, dim3((unsigned)((4 * (long long)batch + 255) / 256)), dim3(256),
                       0, s, d_sim_out, batch, d_candidates);
    return launch_rc(hipGetLastError());
}

}  // extern "C"
