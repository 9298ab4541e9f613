/*
 * lmpc_lowsim.h -- the low-level ticks of one MPC tick as one launch: the joint-PD controller (lmpc_lowlevel.h) and the
 * rigid-body plant (lmpc_sim.h) fused over `ticks` low-level ticks (library liblmpc.so).
 *
 * Between two low-level ticks of the joint-PD loop only the robot's state and the plant's held / touch flags travel;
 * the target and the gait word are constant for the whole MPC tick.  Per robot and per tick i = 0 .. ticks - 1 this is,
 * bit for bit, the sequence
 *
 *   candidates[l] = held[l] | touch[l] of sim_out            lmpc_lowlevel_device's candidate rule
 *   ll_out        = lmpc_lowlevel(ll_cfg, state, target, gait)
 *   state, sim_out = lmpc_sim_step(model, sim_cfg, state, ll_out.tau, candidates), `substeps` times with tau and the
 *                    candidates held (lmpc_sim_step_device's `substeps`)
 *
 * with the state and the flags kept in registers on the device: one launch instead of 2 * ticks.  The arithmetic is the
 * two headers' own (csrc/lmpc_lowlevel_common.h, csrc/lmpc_sim_common.h and the plant's substep of
 * csrc/lmpc_sim_device.h, no FMA contraction), so the results are the unfused sequence's bits.  A robot whose plant
 * step fails (lmpc_sim_out.status 1) goes on from its unchanged state and a zeroed lmpc_sim_out on the next tick, as in
 * the unfused loop, where every launch starts afresh.
 *
 * Not fused here: the state estimator and the frictional contact plant, which sit between the ticks.
 *
 * Return codes, stream and ordering conventions are lmpc.h's / lmpc_stack.h's.
 */
#ifndef LMPC_LMPC_LOWSIM_H
#define LMPC_LMPC_LOWSIM_H

#include "lmpc/lmpc_lowlevel.h"
#include "lmpc/lmpc_rbd.h"
#include "lmpc/lmpc_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_LOWSIM_ABI_VERSION 1

/* Per-tick logs: row i of each array ([ticks][batch] elements) is what tick i left -- the state and lmpc_sim_out after
 * its plant step, its lmpc_lowlevel_out and its candidate words.  Each pointer may be NULL. */
typedef struct lmpc_lowsim_log {
    lmpc_rbd_state* states;
    lmpc_sim_out* outs;
    lmpc_lowlevel_out* ll_outs;
    int32_t* candidates; /* [ticks][batch][4] */
} lmpc_lowsim_log;

int lmpc_lowsim_abi_version(void);
/* robots per block of the device kernel (for tests that straddle a block's edge) */
int lmpc_lowsim_block_robots(void);

/* One robot, host.  state and sim_out are read and updated in place; candidates (4 words) and ll_out receive the last
 * tick's.  gait (may be NULL: mode 1): the robot's gait word.  log (may be NULL): rows of one robot, [ticks].
 * ticks == 0: LMPC_OK, nothing touched.  LMPC_ERR_ARG: a NULL required pointer, ticks < 0, substeps < 1, a
 * sim_cfg->dt that is not positive and finite. */
int lmpc_lowsim_run(const lmpc_rbd_model* model, const lmpc_sim_cfg* sim_cfg, const lmpc_lowlevel_cfg* ll_cfg,
                    lmpc_rbd_state* state, const lmpc_wbc_target* target, const int32_t* gait, lmpc_sim_out* sim_out,
                    int32_t* candidates, lmpc_lowlevel_out* ll_out, int ticks, int substeps, const lmpc_lowsim_log* log);

/* A batch on the device, one launch, asynchronous on `stream`.  d_state [batch] and d_sim_out [batch] are read and
 * updated in place; d_candidates [batch][4] and d_ll_out [batch] receive the last tick's -- the buffers, and the bits,
 * that `ticks` rounds of lmpc_lowlevel_device (with d_sim_out / d_candidates) and lmpc_sim_step_device (in place, tau read
 * from d_ll_out) leave.  d_gait (may be NULL: mode 1) with gait_stride as lmpc_lowlevel_device's.  log (may be NULL): a
 * host struct of device pointers.
 * ticks == 0 or batch == 0: LMPC_OK, nothing touched.  LMPC_ERR_ARG: a NULL required pointer, a negative batch or
 * ticks, substeps < 1, a sim_cfg->dt that is not positive and finite, a gait_stride below 1 with d_gait given, a stream
 * on another device than d_state's. */
int lmpc_lowsim_run_device(const lmpc_rbd_model* model, const lmpc_sim_cfg* sim_cfg, const lmpc_lowlevel_cfg* ll_cfg,
                           lmpc_rbd_state* d_state, const lmpc_wbc_target* d_target, const int32_t* d_gait,
                           int64_t gait_stride, lmpc_sim_out* d_sim_out, int32_t* d_candidates,
                           lmpc_lowlevel_out* d_ll_out, int batch, int ticks, int substeps, const lmpc_lowsim_log* log,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMPC_LMPC_LOWSIM_H */
