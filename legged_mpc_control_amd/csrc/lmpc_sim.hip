// lmpc_sim.hip -- the batched rigid-body plant of include/lmpc/lmpc_sim.h: contact-constrained forward dynamics and
// the time-stepping integrator, on the host (one robot) and on the device (a batch, four lanes per robot).
//
// The arithmetic is lmpc_rbd_common.h's (leg_pass / base_pass) and lmpc_sim_common.h's (the elimination), compiled
// for both sides.  The step itself is written in lmpc_sim_common.h (host: solve_robot()) and lmpc_sim_device.h (device:
// substep()), as halves around the contact solve that lmpc_contact.hip's plant shares; this file holds the kernel's
// loop and the entry points.  Device mapping, as lmpc_rbd.hip's (lmpc_quad_device.h): lane 4 r + l of a wavefront owns
// leg l of the wavefront's r-th robot.  One kernel does everything: the lane runs leg_pass for its leg, the quad
// exchanges the legs' totals for base_pass, the lane eliminates its leg's joints (27 doubles for the base), the quad
// exchanges those and every lane factors the same 6 x 6 base block (the same bits in all four); the 12 x 12 J M^-1 J'
// is spread over the quad, lane l holding block row l, and factored by a block Cholesky whose 3 x 3 blocks travel by
// quad shuffles; then the lane back-substitutes its own leg.  The unilateral rule repeats only that last factorisation
// with the shrunken set; the substeps loop with the state in registers.  No LDS, no scratch, no workspace, no 18 x 18
// matrix anywhere.
//
// leg_pass indexes the model and the state by the leg's number.  Here each lane copies its leg's part of the model
// and its own joints into slot 0 of a private model / state and calls leg_pass(..., leg 0): every index is then a
// compile-time constant and the private structs live in registers; the values, and so the arithmetic, are the same.
#include <hip/hip_runtime.h>

#include "lmpc/lmpc_sim.h"
#include "lmpc_sim_common.h"
#include "lmpc_quad_device.h"
#include "lmpc_sim_device.h"

static_assert(sizeof(lmpc_sim_cfg) == 24, "lmpc_sim_cfg layout (legged_mpc_control_amd/_native.py)");
static_assert(sizeof(lmpc_sim_out) == 472, "lmpc_sim_out layout");

namespace lmpc_sim {
namespace {

#if defined(__HIPCC__)
// STEP = false: the forward dynamics (substeps = 1, dt and ground_z unused, nexts unused).
template <bool STEP>
__global__ void __launch_bounds__(BLOCK)
    lmpc_sim_kernel(const lmpc_rbd_model md, const lmpc_rbd_state* states, const double* __restrict__ taus,
                    long long tau_stride, const int32_t* __restrict__ contacts, long long contact_stride, int batch,
                    int substeps, double dt, double ground_z, int unilateral, lmpc_rbd_state* nexts, lmpc_sim_out* outs) {
    const int robot = blockIdx.x * BLOCK_ROBOTS + (threadIdx.x >> 2), L = threadIdx.x & 3;
    // a quad past the batch computes the last robot again and stores nothing: the shuffles below stay uniform
    const bool active = robot < batch;
    const int r = active ? robot : batch - 1;

    lmpc_rbd_state ls;  // the base's state, and the lane's own joints in slot 0
    load_lane_state(states[r], L, ls);
    const double* tp = taus + (long long)r * tau_stride + 3 * L;
    const double tau3[3] = {tp[0], tp[1], tp[2]};
    const bool candidate = contacts[(long long)r * contact_stride + L] != 0;

    bool failed = false;  // quad-uniform; once set the state is frozen

    const int nsub = STEP ? substeps : 1;
    for (int step = 0; step < nsub; ++step) {
        // the substep itself: lmpc_sim_device.h (the fused controller + plant kernel of lmpc_lowsim.hip runs the same one)
        LaneOut o;
        bool held;
        int otouch;
        step_lane<STEP>(md, L, ls, tau3, candidate, dt, ground_z, unilateral, o, held, otouch, failed);
        if (outs && step == nsub - 1) store_out(outs[r], o, held && !failed ? 1 : 0, otouch, failed ? 1 : 0, L, active);
    }

    if (STEP) store_state(nexts[r], ls, L, active);
}
#endif

}  // namespace
}  // namespace lmpc_sim

using namespace lmpc_sim;

extern "C" int lmpc_sim_abi_version(void) { return LMPC_SIM_ABI_VERSION; }
extern "C" int lmpc_sim_cfg_size(void) { return (int)sizeof(lmpc_sim_cfg); }
extern "C" int lmpc_sim_out_size(void) { return (int)sizeof(lmpc_sim_out); }
extern "C" size_t lmpc_sim_work_bytes(int batch) {
    (void)batch;
    return 0;
}

extern "C" void lmpc_sim_cfg_default(lmpc_sim_cfg* cfg) {
    if (!cfg) return;
    *cfg = lmpc_sim_cfg{};
    cfg->dt = 0.002;
    cfg->ground_z = 0.0;
    cfg->unilateral = 1;
}

extern "C" int lmpc_rbd_forward_dynamics(const lmpc_rbd_model* model, const lmpc_rbd_state* state, const double* tau,
                                         const int32_t* contact, int unilateral, lmpc_sim_out* out) {
    if (!model || !state || !tau || !contact || !out) return LMPC_ERR_ARG;
    solve_robot(*model, *state, tau, contact, unilateral != 0, false, 0.0, 0.0, nullptr, *out);
    return LMPC_OK;
}

extern "C" int lmpc_sim_step(const lmpc_rbd_model* model, const lmpc_sim_cfg* cfg, const lmpc_rbd_state* state,
                             const double* tau, const int32_t* contact, lmpc_rbd_state* next_state, lmpc_sim_out* out) {
    if (!model || !cfg || !state || !tau || !contact || !next_state || !out || !good_dt(cfg->dt)) return LMPC_ERR_ARG;
    solve_robot(*model, *state, tau, contact, cfg->unilateral != 0, true, cfg->dt, cfg->ground_z, next_state, *out);
    return LMPC_OK;
}

extern "C" int lmpc_rbd_forward_dynamics_device(const lmpc_rbd_model* model, const lmpc_rbd_state* d_state,
                                                const double* d_tau, int64_t tau_stride, const int32_t* d_contact,
                                                int64_t contact_stride, int batch, int unilateral, lmpc_sim_out* d_out,
                                                void* stream) {
    if (batch < 0 || (batch > 0 && (!model || !d_state || !d_tau || !d_contact || !d_out || tau_stride < 12 ||
                                    contact_stride < 4)))
        return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipLaunchKernelGGL((lmpc_sim_kernel<false>), quad_grid(batch), dim3(BLOCK), 0,
                       (hipStream_t)stream, *model, d_state, d_tau, (long long)tau_stride, d_contact,
                       (long long)contact_stride, batch, 1, 0.0, 0.0, unilateral, (lmpc_rbd_state*)nullptr, d_out);
    return hipGetLastError() == hipSuccess ? LMPC_OK : LMPC_ERR_LAUNCH;
}

extern "C" int lmpc_sim_step_device(const lmpc_rbd_model* model, const lmpc_sim_cfg* cfg, const lmpc_rbd_state* d_state,
                                    const double* d_tau, int64_t tau_stride, const int32_t* d_contact,
                                    int64_t contact_stride, int batch, int substeps, lmpc_rbd_state* d_next,
                                    lmpc_sim_out* d_out, void* d_work, size_t work_bytes, void* stream) {
    (void)d_work, (void)work_bytes;
    if (batch < 0 || (batch > 0 && (!model || !cfg || !d_state || !d_tau || !d_contact || !d_next || tau_stride < 12 ||
                                    contact_stride < 4 || substeps < 1 || !good_dt(cfg->dt))))
        return LMPC_ERR_ARG;
    if (batch == 0) return LMPC_OK;
    hipLaunchKernelGGL((lmpc_sim_kernel<true>), quad_grid(batch), dim3(BLOCK), 0,
                       (hipStream_t)stream, *model, d_state, d_tau, (long long)tau_stride, d_contact,
                       (long long)contact_stride, batch, substeps, cfg->dt, cfg->ground_z, (int)cfg->unilateral, d_next,
                       d_out);
    return hipGetLastError() == hipSuccess ? LMPC_OK : LMPC_ERR_LAUNCH;
}
