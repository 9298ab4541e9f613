// lmpc_lowsim_common.h -- the host side of include/lmpc/lmpc_lowsim.h: one robot's low-level ticks as the composition of
// lmpc_lowlevel_common.h (the controller, the candidate rule) and lmpc_sim_common.h (the plant step), in the order of the
// device loop.  Plain C++ with no HIP runtime call: lmpc_lowsim.hip's lmpc_lowsim_run is this function, and
// tests/cpp/lowsim_host_check.cpp runs it under the host compiler's sanitizers.
#pragma once
#include "lmpc/lmpc_lowsim.h"
#include "lmpc_lowlevel_common.h"
#include "lmpc_sim_common.h"

namespace lmpc_lowsim {

using lmpc_sim::good_dt;

// lmpc_lowsim_run.  Every tick works on copies, so `ll_out` and the log rows may not overlap the inputs but nothing is
// read after it was overwritten.
inline int run_robot(const lmpc_rbd_model* model, const lmpc_sim_cfg* sim_cfg, const lmpc_lowlevel_cfg* ll_cfg,
                     lmpc_rbd_state* state, const lmpc_wbc_target* target, const int32_t* gait, lmpc_sim_out* sim_out,
                     int32_t* candidates, lmpc_lowlevel_out* ll_out, int ticks, int substeps, const lmpc_lowsim_log* log) {
    if (ticks < 0) return LMPC_ERR_ARG;
    if (ticks == 0) return LMPC_OK;
    if (!model || !sim_cfg || !ll_cfg || !state || !target || !sim_out || !candidates || !ll_out || substeps < 1 ||
        !good_dt(sim_cfg->dt))
        return LMPC_ERR_ARG;
    const int mode = gait && *gait == LMPC_GAIT_STAND ? 0 : 1;
    for (int i = 0; i < ticks; ++i) {
        int32_t cand[4];
        for (int l = 0; l < 4; ++l) cand[l] = lmpc_ll::candidate(sim_out->held[l], sim_out->touch[l]);
        lmpc_lowlevel_out ll;
        lmpc_ll::robot(*ll_cfg, *state, *target, mode, ll);
        for (int s = 0; s < substeps; ++s)  // tau and the candidates held, as lmpc_sim_step_device's substeps
            lmpc_sim::solve_robot(*model, *state, ll.tau, cand, sim_cfg->unilateral != 0, true, sim_cfg->dt,
                                  sim_cfg->ground_z, state, *sim_out);
        for (int l = 0; l < 4; ++l) candidates[l] = cand[l];
        *ll_out = ll;
        if (log) {
            if (log->states) log->states[i] = *state;
            if (log->outs) log->outs[i] = *sim_out;
            if (log->ll_outs) log->ll_outs[i] = ll;
            if (log->candidates)
                for (int l = 0; l < 4; ++l) log->candidates[4 * i + l] = cand[l];
        }
    }
    return LMPC_OK;
}

}  // namespace lmpc_lowsim
