"""The low-level ticks of one MPC tick as one launch (include/lmpc/lmpc_lowsim.h).

The joint-PD controller (`lowlevel`) and the rigid-body plant (`sim`) fused over `ticks` low-level ticks: per tick the
candidates from the plant's last `held | touch`, the controller on the current state, then `substeps` plant substeps on
its torques.  On the device the state and the flags stay in registers between the ticks, so an MPC tick's low-level
ticks are one launch instead of two per tick; the results are the bits of the unfused sequence `lowlevel_device` (with
candidates) + `sim.step_device` (in place).

  * `run()` -- one robot on the host (the same arithmetic, compiled for the CPU);
  * `run_device()` -- a batch resident in HBM, one launch, asynchronous on a stream; optionally logs every tick;
  * `stack.StackLoop(..., low_level=cfg, fused_low_level=True)` closes the loop on it.

The device function is a HIP kernel; there is no CPU fallback behind it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from .lowlevel import OUT_BYTES as LL_OUT_BYTES
from .rbd import STATE_BYTES, TARGET_BYTES
from .sim import OUT_BYTES as SIM_OUT_BYTES

# the log arrays by the names of StackLoop's logs: (field of lmpc_lowsim_log, torch dtype name, trailing shape)
LOG_KEYS = {"states": ("states", "uint8", (STATE_BYTES,)), "out": ("outs", "uint8", (SIM_OUT_BYTES,)),
            "ll_out": ("ll_outs", "uint8", (LL_OUT_BYTES,)), "candidates": ("candidates", "int32", (4,))}


def run(model: N.LmpcRbdModel, sim_cfg: N.LmpcSimCfg, ll_cfg: N.LmpcLowlevelCfg, state: N.LmpcRbdState,
        target: N.LmpcWbcTarget, sim_out: N.LmpcSimOut, ticks: int, substeps: int = 1, gait=None, log: bool = False):
    """One robot on the host (lmpc_lowsim_run); `state` and `sim_out` are not modified.  gait: the robot's gait word
    (N.GAIT_STAND: movement mode 0), None: mode 1.  -> dict: `state`, `sim_out` (after the last tick), `candidates`
    (int32 [4]) and `ll_out` (the last tick's); with log=True also `states`, `outs`, `ll_outs` (ctypes arrays [ticks]) and
    `candidates_log` (int32 [ticks][4])."""
    n = max(int(ticks), 0)
    st = N.LmpcRbdState.from_buffer_copy(bytes(state))
    so = N.LmpcSimOut.from_buffer_copy(bytes(sim_out))
    cand = (ctypes.c_int32 * 4)()
    ll = N.LmpcLowlevelOut()
    g = None if gait is None else ctypes.byref(ctypes.c_int32(int(gait)))
    res, lg = {}, None
    if log:
        res = dict(states=(N.LmpcRbdState * n)(), outs=(N.LmpcSimOut * n)(), ll_outs=(N.LmpcLowlevelOut * n)())
        cl = np.zeros((n, 4), dtype=np.int32)
        lg = N.LmpcLowsimLog(ctypes.addressof(res["states"]), ctypes.addressof(res["outs"]),
                             ctypes.addressof(res["ll_outs"]), cl.ctypes.data)
        res["candidates_log"] = cl
    N.check(N.lib().lmpc_lowsim_run(ctypes.byref(model), ctypes.byref(sim_cfg), ctypes.byref(ll_cfg), ctypes.byref(st),
                                    ctypes.byref(target), g, ctypes.byref(so), cand, ctypes.byref(ll), int(ticks),
                                    int(substeps), None if lg is None else ctypes.byref(lg)), "lmpc_lowsim_run")
    res.update(state=st, sim_out=so, candidates=np.array(cand, dtype=np.int32), ll_out=ll)
    return res


def run_device(model: N.LmpcRbdModel, sim_cfg: N.LmpcSimCfg, ll_cfg: N.LmpcLowlevelCfg, d_state, d_target, d_sim_out,
               d_candidates, d_ll_out, ticks: int, substeps: int = 1, d_gait=None, logs: dict = None, stream=None):
    """A batch on the device (lmpc_lowsim_run_device), one launch: d_state uint8 [B][288] and d_sim_out uint8 [B][472]
    are updated in place; d_target uint8 [B][352]; d_candidates int32 [B][4] and d_ll_out uint8 [B][400] receive the last
    tick's; d_gait int32 [B] (a view with any stride, e.g. `est.gait_view(d_robots)`; None: mode 1).  logs: a dict of
    tensors, any of `states` uint8 [ticks][B][288], `out` uint8 [ticks][B][472], `ll_out` uint8 [ticks][B][400] and
    `candidates` int32 [ticks][B][4]: row i is what tick i left."""
    import torch

    B, dev = D.batch("d_state", d_state)
    ticks = int(ticks)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_target", d_target, torch.uint8, (B, TARGET_BYTES), dev)
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, SIM_OUT_BYTES), dev)
    D.check("d_candidates", d_candidates, torch.int32, (B, 4), dev)
    D.check("d_ll_out", d_ll_out, torch.uint8, (B, LL_OUT_BYTES), dev)
    gs = D.view("d_gait", d_gait, torch.int32, B, None, dev, optional=True)
    lg = None
    if logs:
        unknown = set(logs) - set(LOG_KEYS)
        if unknown:
            raise ValueError(f"logs: unknown keys {sorted(unknown)}; expected some of {sorted(LOG_KEYS)}")
        lg = N.LmpcLowsimLog()
        for key, t in logs.items():
            field, dtype, tail = LOG_KEYS[key]
            D.check(f"logs[{key!r}]", t, getattr(torch, dtype), (max(ticks, 0), B) + tail, dev)
            setattr(lg, field, t.data_ptr())
    N.check(N.lib().lmpc_lowsim_run_device(
        ctypes.byref(model), ctypes.byref(sim_cfg), ctypes.byref(ll_cfg), d_state.data_ptr(), d_target.data_ptr(),
        D.ptr(d_gait), gs, d_sim_out.data_ptr(), d_candidates.data_ptr(), d_ll_out.data_ptr(), B, ticks, int(substeps),
        None if lg is None else ctypes.byref(lg), D.stream(stream, dev)), "lmpc_lowsim_run_device")
