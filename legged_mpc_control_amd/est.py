"""Sensors -> the base position and velocity the controllers see (include/lmpc/lmpc_est.h).

The reference's `BasicKF` (an 18-state, 28-measurement linear Kalman filter over IMU acceleration, leg kinematics and
the contact flags, with the orientation taken as known) and a sensor model that reads an ideal IMU and encoders off the
plant of `sim`, with optional Gaussian noise from the library's Philox generator.

  * `cfg()` -- `lmpc_est_cfg` with the reference's constants;
  * `sensors_from_plant()`, `init()`, `update()`, `report()`, `feedback()` -- one robot on the host (the same arithmetic,
    compiled for the CPU);
  * `sensors_from_plant_device()`, `init_device()`, `update_device()` -- a batch resident in HBM, asynchronous on a
    stream; the update writes the estimated `lmpc_rbd_state` (which drops into `WbcPipeline` and the stack's advance)
    and, on request, a shadow `lmpc_sim_out` whose feet and contact flags are the estimate's;
  * `stack.StackLoop(..., estimator=cfg())` closes the loop on that estimate.

The 28 measurements are applied as scalar updates (R is diagonal), not through a factorisation of the 28 x 28
innovation covariance; what else is chosen here rather than restated is listed in the header.  The device functions
are HIP kernels; there is no CPU fallback behind them.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from .rbd import STATE_BYTES
from .sim import OUT_BYTES as SIM_OUT_BYTES

SENSORS_BYTES = ctypes.sizeof(N.LmpcEstSensors)  # 296
CFG_BYTES = ctypes.sizeof(N.LmpcEstCfg)          # 144
FILTER_BYTES = ctypes.sizeof(N.LmpcEstFilter)    # 2744
OUT_BYTES = ctypes.sizeof(N.LmpcEstOut)          # 312
NX, NY = 18, 28
GAIT_OFFSET = N.LmpcCommand.gait.offset // 4     # lmpc_stack_robot.rb.cmd.gait, in int32s
GAIT_STRIDE = N.STACK_ROBOT_BYTES // 4

_dp = ctypes.POINTER(ctypes.c_double)

SENSORS_DTYPE = np.dtype([("imu_acc", "3f8"), ("imu_ang_vel", "3f8"), ("euler", "3f8"), ("joint_pos", "12f8"),
                          ("joint_vel", "12f8"), ("contact", "4f8")])
FILTER_DTYPE = np.dtype([("x", "18f8"), ("P", "(18,18)f8"), ("inited", "i4"), ("ticks", "i4")])
OUT_DTYPE = np.dtype([("foot_pos_rel", "12f8"), ("foot_pos_world", "12f8"), ("foot_vel_world", "12f8"),
                      ("estimated_contacts", "4i4"), ("status", "i4"), ("reserved", "i4")])
assert SENSORS_DTYPE.itemsize == SENSORS_BYTES and FILTER_DTYPE.itemsize == FILTER_BYTES
assert OUT_DTYPE.itemsize == OUT_BYTES


def cfg(dt=None, seed=None, assume_flat_ground=None, **fields) -> N.LmpcEstCfg:
    """`lmpc_est_cfg_default` (dt 1.25 ms, the reference's constants, exact sensors), then the given fields (any
    field of lmpc_est_cfg by name, e.g. sigma_acc=0.05)."""
    c = N.LmpcEstCfg()
    N.lib().lmpc_est_cfg_default(ctypes.byref(c))
    if dt is not None:
        c.dt = float(dt)
    if seed is not None:
        c.seed = int(seed)
    if assume_flat_ground is not None:
        c.assume_flat_ground = int(bool(assume_flat_ground))
    names = {f[0] for f in N.LmpcEstCfg._fields_}
    for k, v in fields.items():
        if k not in names or k == "reserved":
            raise TypeError(f"lmpc_est_cfg has no field {k!r}")
        setattr(c, k, float(v))
    return c


def sensors(imu_acc=(0.0, 0.0, 9.81), imu_ang_vel=(0.0, 0.0, 0.0), euler=(0.0, 0.0, 0.0), joint_pos=None, joint_vel=None,
            contact=(1.0, 1.0, 1.0, 1.0)) -> N.LmpcEstSensors:
    s = N.LmpcEstSensors()
    for name, val, n in (("imu_acc", imu_acc, 3), ("imu_ang_vel", imu_ang_vel, 3), ("euler", euler, 3),
                         ("joint_pos", joint_pos, 12), ("joint_vel", joint_vel, 12), ("contact", contact, 4)):
        a = np.zeros(n) if val is None else np.asarray(val, dtype=np.float64).reshape(n)
        getattr(s, name)[:] = [float(v) for v in a]
    return s


def sensors_from_plant(model, c: N.LmpcEstCfg, state, sim_out, robot_index: int = 0, tick: int = 0,
                       stand: bool = False) -> N.LmpcEstSensors:
    """What an ideal IMU and encoders read on one robot of the plant, plus cfg's noise keyed by (seed, robot_index,
    tick) (lmpc_est_sensors_from_plant)."""
    s = N.LmpcEstSensors()
    N.check(N.lib().lmpc_est_sensors_from_plant(ctypes.byref(model), ctypes.byref(c), ctypes.byref(state),
                                                ctypes.byref(sim_out), int(robot_index), int(tick), int(bool(stand)),
                                                ctypes.byref(s)), "lmpc_est_sensors_from_plant")
    return s


def init(model, c: N.LmpcEstCfg, s: N.LmpcEstSensors, pos0=None) -> N.LmpcEstFilter:
    """BasicKF::init_state (lmpc_est_init); pos0 None: the reference's (0, 0, 0.09)."""
    f = N.LmpcEstFilter()
    p = None
    if pos0 is not None:
        p = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pos0, dtype=np.float64).reshape(3)])
    N.check(N.lib().lmpc_est_init(ctypes.byref(model), ctypes.byref(c), ctypes.byref(s), p, ctypes.byref(f)),
            "lmpc_est_init")
    return f


def report(model, s: N.LmpcEstSensors, f: N.LmpcEstFilter):
    """(state_est, lmpc_est_out) of a filter as it stands (lmpc_est_report)."""
    se, o = N.LmpcRbdState(), N.LmpcEstOut()
    N.check(N.lib().lmpc_est_report(ctypes.byref(model), ctypes.byref(s), ctypes.byref(f), ctypes.byref(se),
                                    ctypes.byref(o)), "lmpc_est_report")
    return se, o


def update(model, c: N.LmpcEstCfg, s: N.LmpcEstSensors, f: N.LmpcEstFilter):
    """One BasicKF::update_estimation, `f` in place (lmpc_est_update) -> (state_est, lmpc_est_out); the robot's status
    is lmpc_est_out.status."""
    se, o = N.LmpcRbdState(), N.LmpcEstOut()
    N.check(N.lib().lmpc_est_update(ctypes.byref(model), ctypes.byref(c), ctypes.byref(s), ctypes.byref(f),
                                    ctypes.byref(se), ctypes.byref(o)), "lmpc_est_update")
    return se, o


def feedback(sim_out: N.LmpcSimOut, o: N.LmpcEstOut) -> N.LmpcSimOut:
    """The plant's block with the estimate's feet and contact flags (lmpc_est_feedback)."""
    sh = N.LmpcSimOut()
    N.check(N.lib().lmpc_est_feedback(ctypes.byref(sim_out), ctypes.byref(o), ctypes.byref(sh)), "lmpc_est_feedback")
    return sh


def filter_view(buf) -> np.ndarray:
    """uint8 [..., 2744] (torch or NumPy) or an LmpcEstFilter -> structured array with x, P [18, 18], inited, ticks."""
    if isinstance(buf, N.LmpcEstFilter):
        return np.frombuffer(bytes(buf), dtype=FILTER_DTYPE)[0]
    return D.host_view(buf, FILTER_DTYPE)


def sensors_view(buf) -> np.ndarray:
    return D.host_view(buf, SENSORS_DTYPE)


def out_view(buf) -> np.ndarray:
    return D.host_view(buf, OUT_DTYPE)


# ---- device ----------------------------------------------------------------------------------------------------------
def sensors_from_plant_device(model, c: N.LmpcEstCfg, d_state, d_sim_out, d_sensors, tick: int = 0, index0: int = 0,
                              d_gait=None, stream=None):
    """A batch of sensor readings on the device (lmpc_est_sensors_from_plant_device): d_state uint8 [B][288], d_sim_out
    uint8 [B][472], d_sensors uint8 [B][296]; robot b is keyed (cfg.seed, index0 + b, tick).  d_gait: int32 [B] (a view
    with any stride, e.g. `gait_view(d_robots)`), LMPC_GAIT_STAND there sets every contact flag."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, SIM_OUT_BYTES), dev)
    D.check("d_sensors", d_sensors, torch.uint8, (B, SENSORS_BYTES), dev)
    gs = D.view("d_gait", d_gait, torch.int32, B, None, dev, optional=True)
    if not 0 <= int(tick) < 2 ** 32:
        raise ValueError("tick outside 0..2^32 - 1")
    N.check(N.lib().lmpc_est_sensors_from_plant_device(
        ctypes.byref(model), ctypes.byref(c), d_state.data_ptr(), d_sim_out.data_ptr(), B, int(index0), int(tick),
        D.ptr(d_gait), gs, d_sensors.data_ptr(), D.stream(stream, dev)), "lmpc_est_sensors_from_plant_device")


def gait_view(d_robots):
    """The int32 [B] view of lmpc_stack_robot.rb.cmd.gait inside packed robots (uint8 [B][960])."""
    import torch

    return d_robots.view(torch.int32)[:, GAIT_OFFSET]


def init_device(model, c: N.LmpcEstCfg, d_sensors, d_filter, d_pos0=None, d_state_est=None, d_out=None, d_sim_out=None,
                d_shadow=None, stream=None):
    """A batch of BasicKF::init_state on the device (lmpc_est_init_device): d_sensors uint8 [B][296], d_filter uint8
    [B][2744]; d_pos0 float64 [B][3] (a view with any row stride; None: the reference's default); optionally the
    report into d_state_est uint8 [B][288], d_out uint8 [B][312] and the shadow of d_sim_out into d_shadow."""
    import torch

    B, dev = _filter_args(d_sensors, d_filter, d_state_est, d_out, d_sim_out, d_shadow)
    ps = D.view("d_pos0", d_pos0, torch.float64, B, 3, dev, optional=True)
    ptr = D.ptr
    N.check(N.lib().lmpc_est_init_device(
        ctypes.byref(model), ctypes.byref(c), ptr(d_sensors), ptr(d_pos0), ps, B, ptr(d_filter), ptr(d_state_est),
        ptr(d_out), ptr(d_sim_out), ptr(d_shadow), D.stream(stream, dev)), "lmpc_est_init_device")


def _filter_args(d_sensors, d_filter, d_state_est, d_out, d_sim_out, d_shadow):
    """The checks init_device and update_device share -> (B, device)."""
    import torch

    B, dev = D.batch("d_sensors", d_sensors)
    D.check("d_sensors", d_sensors, torch.uint8, (B, SENSORS_BYTES), dev)
    D.check("d_filter", d_filter, torch.uint8, (B, FILTER_BYTES), dev)
    D.check("d_state_est", d_state_est, torch.uint8, (B, STATE_BYTES), dev, optional=True)
    D.check("d_out", d_out, torch.uint8, (B, OUT_BYTES), dev, optional=True)
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, SIM_OUT_BYTES), dev, optional=True)
    D.check("d_shadow", d_shadow, torch.uint8, (B, SIM_OUT_BYTES), dev, optional=True)
    if d_shadow is not None and d_sim_out is None:
        raise ValueError("d_shadow needs d_sim_out")
    return B, dev


def update_device(model, c: N.LmpcEstCfg, d_sensors, d_filter, d_state_est=None, d_out=None, d_sim_out=None,
                  d_shadow=None, stream=None):
    """One filter update of every robot on the device (lmpc_est_update_device): d_filter in place; d_state_est uint8
    [B][288] and d_out uint8 [B][312] may be None; with d_shadow (uint8 [B][472], not d_sim_out itself) the same launch
    writes the plant's d_sim_out with the estimate's feet and contact flags."""
    B, dev = _filter_args(d_sensors, d_filter, d_state_est, d_out, d_sim_out, d_shadow)
    if d_shadow is not None and d_shadow.data_ptr() == d_sim_out.data_ptr():
        raise ValueError("d_shadow must not alias d_sim_out")
    ptr = D.ptr
    N.check(N.lib().lmpc_est_update_device(
        ctypes.byref(model), ctypes.byref(c), ptr(d_sensors), B, ptr(d_filter), ptr(d_state_est), ptr(d_out),
        ptr(d_sim_out), ptr(d_shadow), D.stream(stream, dev)), "lmpc_est_update_device")
