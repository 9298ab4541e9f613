"""The reference's joint-PD low-level controller (include/lmpc/lmpc_lowlevel.h).

The path the reference flies in simulation (`tau_ctrl_update`, not its whole-body controller): per leg, the feed-forward
torque -J' R' f of the MPC's force, joint targets from the closed-form leg inverse kinematics of the FSM's foot target
and from J^-1 of its velocity, and tau = kp (angle target - q) + kd (rate target - qd) + feed-forward.

  * `cfg_go1()`, `cfg_a1()` -- `lmpc_lowlevel_cfg` with the gains of the reference's two Gazebo configurations; with a
    model, the kinematics are read off it (`leg_kin_from_model`), else they are the reference's (A1's link lengths);
  * `fk()`, `inv_kin()` -- one leg's kinematics on the host;
  * `lowlevel()` -- one robot on the host (the same arithmetic, compiled for the CPU);
  * `lowlevel_device()` -- a batch resident in HBM, one launch, asynchronous on a stream; with the plant's last
    `lmpc_sim_out` it also writes the plant's candidate contacts;
  * `stack.StackLoop(..., low_level=cfg_go1(model))` closes the loop on it instead of the whole-body controller.

The device function is a HIP kernel; there is no CPU fallback behind it.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from .rbd import STATE_BYTES, TARGET_BYTES
from .sim import OUT_BYTES as SIM_OUT_BYTES

CFG_BYTES = ctypes.sizeof(N.LmpcLowlevelCfg)  # 472
OUT_BYTES = ctypes.sizeof(N.LmpcLowlevelOut)  # 400
TAU_STRIDE = OUT_BYTES // 8                   # lmpc_lowlevel_out.tau of consecutive robots, in doubles
IK_NAN, VEL_NAN, TAU_NONFINITE, CLAMPED = N.LL_IK_NAN, N.LL_VEL_NAN, N.LL_TAU_NONFINITE, N.LL_CLAMPED

OUT_DTYPE = np.dtype([("tau", "12f8"), ("joint_tau_tgt", "12f8"), ("joint_ang_tgt", "12f8"), ("joint_vel_tgt", "12f8"),
                      ("flags", "4i4")])
assert OUT_DTYPE.itemsize == OUT_BYTES

_dp = ctypes.POINTER(ctypes.c_double)


def _vec(a, n):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(n)


def leg_kin_from_model(model: N.LmpcRbdModel) -> N.LmpcLegKin:
    """rho_fix / rho_opt read off a rigid-body model (lmpc_leg_kin_from_model); ValueError for a model outside
    A1Kinematics' class."""
    k = N.LmpcLegKin()
    if N.lib().lmpc_leg_kin_from_model(ctypes.byref(model), ctypes.byref(k)) != N.LMPC_OK:
        raise ValueError("the model's legs are not of A1Kinematics' class (an offset off the hip / thigh / calf axes)")
    return k


def _cfg(preset, model, kp, kd, tau_limit) -> N.LmpcLowlevelCfg:
    c = N.LmpcLowlevelCfg()
    preset(ctypes.byref(c))
    if model is not None:
        c.kin = leg_kin_from_model(model)
    for name, val in (("kp", kp), ("kd", kd)):
        if val is not None:
            g = np.broadcast_to(np.asarray(val, dtype=np.float64), (4, 3))
            for l in range(4):
                getattr(c, name)[l][:] = [float(v) for v in g[l]]
    if tau_limit is not None:
        c.tau_limit[:] = [float(v) for v in np.broadcast_to(np.asarray(tau_limit, dtype=np.float64), (3,))]
    return c


def cfg_go1(model: N.LmpcRbdModel = None, kp=None, kd=None, tau_limit=None) -> N.LmpcLowlevelCfg:
    """`lmpc_lowlevel_cfg_go1` (kp 0.5, kd 0.3, no clamp), then: kin from `model` when given; kp / kd (a scalar, [3] per
    joint or [4][3]); tau_limit (a scalar or [3]; <= 0: no clamp)."""
    return _cfg(N.lib().lmpc_lowlevel_cfg_go1, model, kp, kd, tau_limit)


def cfg_a1(model: N.LmpcRbdModel = None, kp=None, kd=None, tau_limit=None) -> N.LmpcLowlevelCfg:
    """`lmpc_lowlevel_cfg_a1` (kp 15, kd 0.4, no clamp), otherwise as `cfg_go1`."""
    return _cfg(N.lib().lmpc_lowlevel_cfg_a1, model, kp, kd, tau_limit)


def fk(kin: N.LmpcLegKin, leg: int, q) -> np.ndarray:
    """The body-frame foot position of one leg (lmpc_leg_fk)."""
    p = np.zeros(3)
    N.check(N.lib().lmpc_leg_fk(ctypes.byref(kin), int(leg), _vec(q, 3).ctypes.data_as(_dp), p.ctypes.data_as(_dp)),
            "lmpc_leg_fk")
    return p


def inv_kin(kin: N.LmpcLegKin, leg: int, p, cur_q) -> np.ndarray:
    """A1Kinematics::inv_kin of one leg (lmpc_leg_inv_kin); may hold NaNs."""
    q = np.zeros(3)
    N.check(N.lib().lmpc_leg_inv_kin(ctypes.byref(kin), int(leg), _vec(p, 3).ctypes.data_as(_dp),
                                     _vec(cur_q, 3).ctypes.data_as(_dp), q.ctypes.data_as(_dp)), "lmpc_leg_inv_kin")
    return q


def lowlevel(c: N.LmpcLowlevelCfg, state: N.LmpcRbdState, target: N.LmpcWbcTarget, gait=None) -> N.LmpcLowlevelOut:
    """One robot on the host (lmpc_lowlevel).  gait: the robot's gait word (N.GAIT_STAND: movement mode 0), None: mode
    1."""
    o = N.LmpcLowlevelOut()
    g = None if gait is None else ctypes.byref(ctypes.c_int32(int(gait)))
    N.check(N.lib().lmpc_lowlevel(ctypes.byref(c), ctypes.byref(state), ctypes.byref(target), g, ctypes.byref(o)),
            "lmpc_lowlevel")
    return o


def out_view(buf) -> np.ndarray:
    """uint8 [..., 400] (torch or NumPy) -> NumPy structured array [...] with the fields of lmpc_lowlevel_out."""
    return D.host_view(buf, OUT_DTYPE)


def tau_view(d_out):
    """The float64 [B][12] view of lmpc_lowlevel_out.tau inside packed outputs (uint8 [B][400]): what the plant reads."""
    import torch

    return d_out.view(torch.float64)[:, :12]


def flags_view(d_out):
    """The int32 [...][4] view of lmpc_lowlevel_out.flags inside packed outputs (uint8 [...][400])."""
    import torch

    return d_out.view(torch.int32)[..., N.LmpcLowlevelOut.flags.offset // 4:]


def lowlevel_device(c: N.LmpcLowlevelCfg, d_state, d_target, d_out, d_gait=None, d_sim_out=None, d_candidates=None,
                    stream=None):
    """A batch on the device (lmpc_lowlevel_device): d_state uint8 [B][288], d_target uint8 [B][352], d_out uint8
    [B][400]; d_gait int32 [B] (a view with any stride, e.g. `est.gait_view(d_robots)`; None: mode 1); d_sim_out uint8
    [B][472] with d_candidates int32 [B][4] (both or neither): the plant's candidate contacts from the same launch."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_target", d_target, torch.uint8, (B, TARGET_BYTES), dev)
    D.check("d_out", d_out, torch.uint8, (B, OUT_BYTES), dev)
    gs = D.view("d_gait", d_gait, torch.int32, B, None, dev, optional=True)
    if (d_sim_out is None) != (d_candidates is None):
        raise ValueError("d_sim_out and d_candidates: both or neither")
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, SIM_OUT_BYTES), dev, optional=True)
    D.check("d_candidates", d_candidates, torch.int32, (B, 4), dev, optional=True)
    N.check(N.lib().lmpc_lowlevel_device(ctypes.byref(c), d_state.data_ptr(), d_target.data_ptr(), D.ptr(d_gait), gs,
                                         D.ptr(d_sim_out), D.ptr(d_candidates), B, d_out.data_ptr(),
                                         D.stream(stream, dev)), "lmpc_lowlevel_device")
