// lmpc_rollout.hip -- the closed-loop tick on the device (include/lmpc/lmpc_rollout.h).
//
//   lmpc_advance_kernel   one thread per robot: the plant step on the previous tick's u_0 (the QP's own stage-0
//                         transition, ConvexQPSolver.cpp:198-228,294-297), then the bookkeeping before the next QP
//                         (ConvexMpc.cpp:24-108, LeggedContactFSM.cpp:16-84,214-278, Utils.cpp:136-192,
//                         BaseInterface.cpp:358-399); then the block expands its robots' commands into the records
//                         and contact schedules the solve reads, one thread per element (what lmpc_records_kernel
//                         does, by the same lmpc_common functions: one launch less per tick)
//   lmpc_shift_kernel     one thread per byte: the verified active set one MPC step later (lmpc_shift_active_set)
//
// The arithmetic is lmpc_common.h, shared with the host (lmpc_robot_advance), which differs only through sin, cos
// and sqrt.  Both kernels are tiny HBM-bound maps between the solves of a rollout (656 B in and out per robot and
// tick, 33 + 12 H doubles and 4 H bytes out per record).
#include <hip/hip_runtime.h>

#include "lmpc/lmpc.h"
#include "lmpc/lmpc_rollout.h"
#include "lmpc_common.h"

namespace lmpc {

constexpr int ADV_THREADS = 256;
constexpr int ADV_ROBOTS = 16;  // robots per block: their advance on the first 16 lanes, their expansion on all 256

// grf: the previous solve's output [batch][H][12] (u_0 = its first 12), or nullptr: no plant step (the first tick
// of a call).  book = 0: the plant step only (the last launch of a call; rec / contact unused).  cmd_out [batch] or
// nullptr: the command after the bookkeeping (the log).  log_u0 / log_x [batch][12]: the previous tick's slices of
// the log, or nullptr.  rec [batch][33+12H], contact [batch][H][4]: the expansion.
__global__ void __launch_bounds__(ADV_THREADS)
    lmpc_advance_kernel(lmpc_common::PlantParams pp, lmpc_rollout_cfg cfg, lmpc_robot* __restrict__ robots, int batch,
                        const double* __restrict__ grf, int H, int book, lmpc_command* __restrict__ cmd_out,
                        double* __restrict__ log_u0, double* __restrict__ log_x, double* __restrict__ rec,
                        uint8_t* __restrict__ contact) {
    __shared__ lmpc_command sh[ADV_ROBOTS];
    const int base = blockIdx.x * ADV_ROBOTS;
    const int b = base + (int)threadIdx.x;
    if (threadIdx.x < ADV_ROBOTS && b < batch) {
        lmpc_robot rb = robots[b];
        if (grf) {
            double u0[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) u0[k] = grf[(size_t)b * 12 * H + k];
            lmpc_common::plant_step(pp, rb, u0);
            if (log_u0) {
#pragma unroll
                for (int k = 0; k < 12; ++k) log_u0[(size_t)b * 12 + k] = u0[k];
            }
            if (log_x) {
                const lmpc_state_in& st = rb.cmd.state;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    log_x[(size_t)b * 12 + k] = st.root_euler[k];
                    log_x[(size_t)b * 12 + 3 + k] = st.root_pos[k];
                    log_x[(size_t)b * 12 + 6 + k] = st.root_ang_vel[k];
                    log_x[(size_t)b * 12 + 9 + k] = st.root_lin_vel[k];
                }
            }
        }
        if (book) {
            double target[12];
            lmpc_common::robot_bookkeep(cfg, pp.dt, rb, target);
            sh[threadIdx.x] = rb.cmd;
            if (cmd_out) cmd_out[b] = rb.cmd;
        }
        robots[b] = rb;
    }
    if (!book) return;  // uniform over the grid
    __syncthreads();
    const int n = batch - base < ADV_ROBOTS ? batch - base : ADV_ROBOTS;  // robots of this block
    const int RL = LMPC_REC_XREF + 12 * H, CL = 4 * H;
    for (int e = (int)threadIdx.x; e < n * (RL + CL); e += ADV_THREADS) {
        if (e < n * RL) {
            const int r = e / RL, i = e - r * RL;
            rec[(size_t)(base + r) * RL + i] = lmpc_common::record_element(sh[r].state, pp.dt, i);
        } else {
            const int c = e - n * RL, r = c / CL, k = c - r * CL;
            contact[(size_t)(base + r) * CL + k] = lmpc_common::contact_element(sh[r], pp.dt, k >> 2, k & 3);
        }
    }
}

__global__ void __launch_bounds__(256) lmpc_shift_kernel(const uint8_t* __restrict__ act, size_t n, int H,
                                                         uint8_t* __restrict__ shifted) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int k = (int)((e >> 2) % (size_t)H);  // stage of byte e in [batch][H][4]
    shifted[e] = act[k + 1 < H ? e + 4 : e];
}

hipError_t launch_advance(const lmpc_common::PlantParams& pp, const lmpc_rollout_cfg& cfg, lmpc_robot* robots,
                          int batch, const double* grf, int H, int book, lmpc_command* cmd_out, double* log_u0,
                          double* log_x, double* rec, uint8_t* contact, hipStream_t stream) {
    hipLaunchKernelGGL(lmpc_advance_kernel, dim3((batch + ADV_ROBOTS - 1) / ADV_ROBOTS), dim3(ADV_THREADS), 0, stream,
                       pp, cfg, robots, batch, grf, H, book, cmd_out, log_u0, log_x, rec, contact);
    return hipGetLastError();
}

hipError_t launch_shift(const uint8_t* act, int batch, int H, uint8_t* shifted, hipStream_t stream) {
    const size_t n = (size_t)batch * 4 * H;
    hipLaunchKernelGGL(lmpc_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, act, n, H, shifted);
    return hipGetLastError();
}

}  // namespace lmpc
