// lmpc_lowsim.hip -- the low-level ticks of an MPC tick as one launch (include/lmpc/lmpc_lowsim.h): the joint-PD
// controller and the rigid-body plant fused over `ticks` low-level ticks, on the host (one robot) and on the device.
//
//   lmpc_lowsim_kernel   lmpc_sim_kernel's shape: 64 threads, 16 robots per block, lane 4 r + l owns leg l of the block's
//                        r-th robot; a quad past the batch recomputes the last robot and stores nothing.  The lane keeps
//                        the base's state, its own joints and its foot's held / touch flags in registers over all the
//                        ticks.  Per tick it runs its leg's controller (lmpc_ll::leg, no cross-lane traffic, free to
//                        diverge) on those registers and stores the controller's output and the candidate word at once
//                        (into the log row; on the last tick into the buffers) -- only tau3 and the candidate bit are
//                        carried into the plant, which has no registers to spare --
//                        and then runs `substeps` plant substeps (lmpc_sim::step_lane, lmpc_sim_device.h), whose quad
//                        shuffles all 64 lanes reach together: the controller's branches have rejoined by then, and the
//                        tick and substep counts are uniform.
//
// The leg's part of the controller's configuration and its 9 target doubles are loaded anew in every tick, the
// configuration behind an opaque leg index (as lmpc_lowlevel.hip): neither is held across the plant step.  The buffers
// are written on the last tick alone, so they end as the unfused loop leaves them.
#include <hip/hip_runtime.h>

#include "lmpc/lmpc_lowsim.h"
#include "lmpc_launch.h"
#include "lmpc_lowsim_common.h"
#include "lmpc_quad_device.h"
#include "lmpc_sim_device.h"

namespace lmpc_lowsim {
namespace {

using lmpc_sim::BLOCK;
using lmpc_sim::BLOCK_ROBOTS;

#if defined(__HIPCC__)
using lmpc_sim::store_out;
using lmpc_sim::store_state;

__global__ void __launch_bounds__(BLOCK)
    lmpc_lowsim_kernel(const lmpc_rbd_model md, const lmpc_lowlevel_cfg cfg, lmpc_rbd_state* states,
                       const lmpc_wbc_target* __restrict__ targets, const int32_t* __restrict__ gaits,
                       long long gait_stride, lmpc_sim_out* sim_outs, int32_t* __restrict__ cands,
                       lmpc_lowlevel_out* __restrict__ ll_outs, int batch, int ticks, int substeps, double dt,
                       double ground_z, int unilateral, const lmpc_lowsim_log log) {
    const int robot = blockIdx.x * BLOCK_ROBOTS + (threadIdx.x >> 2), L = threadIdx.x & 3;
    // a quad past the batch computes the last robot again and stores nothing: the plant's shuffles stay uniform
    const bool active = robot < batch;
    const int r = active ? robot : batch - 1;

    lmpc_rbd_state ls;  // the base's state, and the lane's own joints in slot 0
    lmpc_sim::load_lane_state(states[r], L, ls);
    const int mode = gaits && gaits[(long long)r * gait_stride] == LMPC_GAIT_STAND ? 0 : 1;
    // the flags of the plant's last step, from here on in registers
    int32_t held = sim_outs[r].held[L], touch = sim_outs[r].touch[L];

    for (int tick = 0; tick < ticks; ++tick) {
        const int32_t cand = lmpc_ll::candidate(held, touch);
        double tau3[3];
        {
            // the leg's number and the robot's are made opaque in every tick (the empty asm): the loads of the
            // configuration and of the target, and the addresses of the stores, then cannot move out of the tick loop,
            // where they would be held in registers through the plant step
            int lo = L, ro = r;
            asm volatile("" : "+v"(lo), "+v"(ro));
            const long long row = (long long)tick * batch + ro;
            lmpc_ll::LegCfg c;
            lmpc_ll::leg_cfg(cfg, lo, c);
            const lmpc_wbc_target& tg = targets[ro];
            lmpc_ll::LegIn in;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                in.euler[i] = ls.euler[i], in.pos[i] = ls.pos[i], in.lin_vel[i] = ls.lin_vel[i];
                in.q[i] = ls.joint_pos[i], in.qd[i] = ls.joint_vel[i];
                in.f[i] = tg.forces_des[3 * L + i], in.p_des[i] = tg.foot_pos_des[3 * L + i];
                in.v_des[i] = tg.foot_vel_des[3 * L + i];
            }
            lmpc_ll::LegOut o;
            lmpc_ll::leg(c, in, mode, o);
#pragma unroll
            for (int i = 0; i < 3; ++i) tau3[i] = o.tau[i];
            if (active) {
                if (tick == ticks - 1) {  // the buffers keep the last tick's
                    lmpc_ll::leg_store(o, L, ll_outs[ro]);
                    cands[4 * (long long)ro + L] = cand;
                }
                if (log.ll_outs) lmpc_ll::leg_store(o, L, log.ll_outs[row]);
                if (log.candidates) log.candidates[4 * row + L] = cand;
            }
        }

        bool failed = false;  // quad-uniform; every tick starts afresh, as every launch of the unfused loop does
        for (int step = 0; step < substeps; ++step) {
            lmpc_sim::LaneOut o;
            bool h;
            int otouch;
            lmpc_sim::step_lane<true>(md, L, ls, tau3, cand != 0, dt, ground_z, unilateral, o, h, otouch, failed);
            if (step == substeps - 1) {
                int ro = r;
                asm volatile("" : "+v"(ro));
                const long long row = (long long)tick * batch + ro;
                held = h && !failed ? 1 : 0, touch = otouch;
                if (tick == ticks - 1) store_out(sim_outs[ro], o, held, touch, failed ? 1 : 0, L, active);
                if (log.outs) store_out(log.outs[row], o, held, touch, failed ? 1 : 0, L, active);
            }
        }
        if (log.states) {
            int ro = r;
            asm volatile("" : "+v"(ro));
            store_state(log.states[(long long)tick * batch + ro], ls, L, active);
        }
    }
    store_state(states[r], ls, L, active);
}
#endif

using lmpc_launch::launch_rc;
using lmpc_launch::PtrScope;

}  // namespace
}  // namespace lmpc_lowsim

using namespace lmpc_lowsim;

extern "C" {

int lmpc_lowsim_abi_version(void) { return LMPC_LOWSIM_ABI_VERSION; }
int lmpc_lowsim_block_robots(void) { return BLOCK_ROBOTS; }

int lmpc_lowsim_run(const lmpc_rbd_model* model, const lmpc_sim_cfg* sim_cfg, const lmpc_lowlevel_cfg* ll_cfg,
                    lmpc_rbd_state* state, const lmpc_wbc_target* target, const int32_t* gait, lmpc_sim_out* sim_out,
                    int32_t* candidates, lmpc_lowlevel_out* ll_out, int ticks, int substeps, const lmpc_lowsim_log* log) {
    return run_robot(model, sim_cfg, ll_cfg, state, target, gait, sim_out, candidates, ll_out, ticks, substeps, log);
}

int lmpc_lowsim_run_device(const lmpc_rbd_model* model, const lmpc_sim_cfg* sim_cfg, const lmpc_lowlevel_cfg* ll_cfg,
                           lmpc_rbd_state* d_state, const lmpc_wbc_target* d_target, const int32_t* d_gait,
                           int64_t gait_stride, lmpc_sim_out* d_sim_out, int32_t* d_candidates,
                           lmpc_lowlevel_out* d_ll_out, int batch, int ticks, int substeps, const lmpc_lowsim_log* log,
                           void* stream) {
    if (batch < 0 || ticks < 0) return LMPC_ERR_ARG;
    if (batch == 0 || ticks == 0) return LMPC_OK;
    if (!model || !sim_cfg || !ll_cfg || !d_state || !d_target || !d_sim_out || !d_candidates || !d_ll_out ||
        (d_gait && gait_stride < 1) || substeps < 1 || !good_dt(sim_cfg->dt))
        return LMPC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    PtrScope ps(d_state, s);
    if (!ps.ok) return LMPC_ERR_ARG;
    const lmpc_lowsim_log lg = log ? *log : lmpc_lowsim_log{nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(lmpc_lowsim_kernel, lmpc_sim::quad_grid(batch), dim3(BLOCK), 0, s,
                       *model, *ll_cfg, d_state, d_target, d_gait, (long long)gait_stride, d_sim_out, d_candidates, d_ll_out,
                       batch, ticks, substeps, sim_cfg->dt, sim_cfg->ground_z, (int)sim_cfg->unilateral, lg);
    return launch_rc(hipGetLastError());
}

}  // extern "C"
