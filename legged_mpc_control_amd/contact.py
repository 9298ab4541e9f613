"""Torques and a mask of feet -> contact forces inside the friction pyramid, contact modes and the next state
(include/lmpc/lmpc_contact.h).

The frictional contact model of the rigid-body plant: a second plant step next to `sim.step`, which per robot and step
solves the convex (Anitescu) relaxation of Coulomb friction on the friction pyramid, certifies the answer and reports
each foot's mode (sticking, sliding against a face or an edge, no force) and slip velocity.

  * `cfg()` -- `lmpc_contact_cfg` (the library's defaults unless given);
  * `solve()`, `step()` -- the bare problem (K, c, mask -> P) and one robot's step on the host (the same arithmetic,
    compiled for the CPU);
  * `solve_device()`, `step_device()` -- batches resident in HBM, asynchronous on a stream; `step_device` takes
    `sim.step_device`'s arguments (tau and the mask may be strided views) plus the extra out block.

The step writes `sim`'s 472-byte `lmpc_sim_out`, so `sim.out_dict` reads it; `out_dict` here reads `lmpc_contact_out`.
The device functions are HIP kernels; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from .rbd import STATE_BYTES
from .sim import OUT_BYTES as SIM_OUT_BYTES
from .sim import _tau_contact

CFG_BYTES = ctypes.sizeof(N.LmpcContactCfg)  # 72
OUT_BYTES = ctypes.sizeof(N.LmpcContactOut)  # 176
MODE_OFFSET = N.LmpcContactOut.mode.offset   # 144: mode[4] within lmpc_contact_out, in bytes
MODE_FREE, MODE_APEX, MODE_NONE = 0, 9, 10
MODE_NAMES = ("free", "face+x", "face-x", "face+y", "face-y", "edge++", "edge+-", "edge-+", "edge--", "apex", "none")

_FLOATS = ("dt", "ground_z", "mu", "recover_speed", "force_threshold", "tol_p", "tol_d")
_INTS = ("use_gap", "touch_rule", "max_sweeps", "max_polish")


def cfg(**kw) -> N.LmpcContactCfg:
    """`lmpc_contact_cfg` with the library's defaults; any field by keyword."""
    c = N.LmpcContactCfg()
    N.lib().lmpc_contact_cfg_default(ctypes.byref(c))
    for k, v in kw.items():
        if k in _FLOATS:
            setattr(c, k, float(v))
        elif k in _INTS:
            setattr(c, k, int(v))
        else:
            raise TypeError(f"lmpc_contact_cfg has no field {k!r}")
    return c


def out_dict(o: N.LmpcContactOut) -> dict:
    return dict(w=np.array(o.w, dtype=np.float64), gap=np.array(o.gap, dtype=np.float64),
                res_primal=float(o.res_primal), res_dual=float(o.res_dual), mode=np.array(o.mode, dtype=np.int32),
                sweeps=int(o.sweeps), polish=int(o.polish), status=int(o.status))


def solve(c: N.LmpcContactCfg, K, cvec, mask):
    """The bare problem on the host (lmpc_contact_solve): K 12 x 12, c (12), mask (4) -> (P (12), lmpc_contact_out)."""
    Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(12, 12))
    cd = np.ascontiguousarray(np.asarray(cvec, dtype=np.float64).reshape(12))
    m = (ctypes.c_int32 * 4)(*[int(bool(v)) for v in mask])
    P = np.zeros(12)
    o = N.LmpcContactOut()
    dp = ctypes.POINTER(ctypes.c_double)
    N.check(N.lib().lmpc_contact_solve(ctypes.byref(c), Kd.ctypes.data_as(dp), cd.ctypes.data_as(dp), m,
                                       P.ctypes.data_as(dp), ctypes.byref(o)), "lmpc_contact_solve")
    return P, o


def step(model, c: N.LmpcContactCfg, st, tau, mask, substeps: int = 1):
    """One robot's step on the host (lmpc_contact_step) -> (next state, lmpc_sim_out, lmpc_contact_out).  substeps > 1
    chains that many calls with tau and the mask held, as the device function's `substeps` does."""
    if substeps < 1:
        raise ValueError("substeps must be positive")
    t, k = _tau_contact(tau, mask)
    cur, o, co = st, N.LmpcSimOut(), N.LmpcContactOut()
    uncertified = False
    for _ in range(substeps):
        nxt = N.LmpcRbdState()
        N.check(N.lib().lmpc_contact_step(ctypes.byref(model), ctypes.byref(c), ctypes.byref(cur), t, k,
                                          ctypes.byref(nxt), ctypes.byref(o), ctypes.byref(co)), "lmpc_contact_step")
        cur = nxt
        uncertified = uncertified or co.status == 2
    if uncertified and co.status == 0:  # as the device's substeps: status 0 means every substep was certified
        o.status = co.status = 2
    return cur, o, co


def solve_device(c: N.LmpcContactCfg, d_K, d_c, d_mask, d_P, d_out=None, stream=None):
    """A batch of bare problems on the device (lmpc_contact_solve_device): d_K float64 [B][144], d_c float64 [B][12],
    d_mask int32 [B][4], d_P float64 [B][12], d_out uint8 [B][176] or None; all contiguous."""
    import torch

    B, dev = D.batch("d_K", d_K)
    D.check("d_K", d_K, torch.float64, (B, 144), dev)
    D.check("d_c", d_c, torch.float64, (B, 12), dev)
    D.check("d_mask", d_mask, torch.int32, (B, 4), dev)
    D.check("d_P", d_P, torch.float64, (B, 12), dev)
    D.check("d_out", d_out, torch.uint8, (B, OUT_BYTES), dev, optional=True)
    N.check(N.lib().lmpc_contact_solve_device(ctypes.byref(c), d_K.data_ptr(), d_c.data_ptr(), d_mask.data_ptr(), B,
                                              d_P.data_ptr(), D.ptr(d_out), D.stream(stream, dev)),
            "lmpc_contact_solve_device")


def work_bytes(batch: int) -> int:
    """Bytes of workspace the three-launch form of `step_device` needs for `batch` robots (lmpc_contact_work_bytes)."""
    return int(N.lib().lmpc_contact_work_bytes(int(batch)))


def step_device(model, c: N.LmpcContactCfg, d_state, d_tau, d_mask, d_next, d_out=None, d_cout=None, substeps: int = 1,
                stream=None, d_work=None):
    """A batch of steps on the device (lmpc_contact_step_device): d_state uint8 [B][288], d_tau float64 [B][12] and
    d_mask int32 [B][4] (views with any row stride), d_next uint8 [B][288] (may be d_state itself), d_out uint8
    [B][472] or None, d_cout uint8 [B][176] or None.  d_work: None runs the fused kernel; a uint8 device tensor of at
    least work_bytes(B) bytes runs the three-launch form (terms and K, the bare solve, the back-substitution), which
    gives the same bits."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    ts = D.view("d_tau", d_tau, torch.float64, B, 12, dev)
    ms = D.view("d_mask", d_mask, torch.int32, B, 4, dev)
    D.check("d_next", d_next, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_out", d_out, torch.uint8, (B, SIM_OUT_BYTES), dev, optional=True)
    D.check("d_cout", d_cout, torch.uint8, (B, OUT_BYTES), dev, optional=True)
    work = 0
    if d_work is not None:  # any length from work_bytes(B) up
        work, _ = D.batch("d_work", d_work)
        D.check("d_work", d_work, torch.uint8, (work,), dev)
        if work < work_bytes(B):
            raise ValueError(f"d_work: {work} bytes, {B} robots need {work_bytes(B)}")
    N.check(N.lib().lmpc_contact_step_device(
        ctypes.byref(model), ctypes.byref(c), d_state.data_ptr(), d_tau.data_ptr(), ts, d_mask.data_ptr(), ms, B,
        int(substeps), d_next.data_ptr(), D.ptr(d_out), D.ptr(d_cout), D.ptr(d_work), work, D.stream(stream, dev)),
        "lmpc_contact_step_device")
