"""The device-resident closed-loop rollout (include/lmpc/lmpc_rollout.h): robot set-up on the host, the host tick
(lmpc_robot_advance, the restatement the device kernel shares its arithmetic with) and views of the logs.

    cfg = rollout.cfg_go1()
    robots = rollout.robots_init(cfg, x0, vel_d, yaw_rate, height, gait, gait_speed)      # ctypes array on the host
    d_robots = rollout.to_device(robots)                                                 # uint8 [B, ROBOT_BYTES]
    log = solver.rollout_device(d_robots, ticks, cfg=cfg, log=True)                      # BatchedConvexQPSolver
    x = log.x.cpu().numpy()                                                              # [ticks, B, 12]
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _device as D
from . import _native as N

_dp = ctypes.POINTER(ctypes.c_double)


def _d(a):
    return a.ctypes.data_as(_dp)


def cfg_go1() -> N.LmpcRolloutCfg:
    c = N.LmpcRolloutCfg()
    N.lib().lmpc_rollout_cfg_go1(ctypes.byref(c))
    return c


def robot_init(cfg: N.LmpcRolloutCfg, x0, vel_d=(0.0, 0.0), yaw_rate: float = 0.0, height: float = 0.30,
               gait: int = N.GAIT_TROT, gait_speed: float = 4.0) -> N.LmpcRobot:
    """One robot at x0 = [euler, pos, omega, v] with its FSMs at reset (lmpc_robot_init)."""
    rb = N.LmpcRobot()
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(12)
    vd = np.ascontiguousarray(vel_d, dtype=np.float64).reshape(2)
    N.check(N.lib().lmpc_robot_init(ctypes.byref(cfg), _d(x0), _d(vd), float(yaw_rate), float(height), int(gait),
                                    float(gait_speed), ctypes.byref(rb)), "lmpc_robot_init")
    return rb


def robots_init(cfg: N.LmpcRolloutCfg, x0, vel_d, yaw_rate, height, gait, gait_speed):
    """A batch of robots -> ctypes array of LmpcRobot.  x0 [B, 12]; every other argument a scalar or one value per
    robot (vel_d: [2] or [B, 2])."""
    x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
    B = x0.shape[0]
    vd = np.broadcast_to(np.asarray(vel_d, dtype=np.float64), (B, 2))
    yr, hg, gs = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)) for v in (yaw_rate, height, gait_speed))
    gt = np.broadcast_to(np.asarray(gait, dtype=np.int64), (B,))
    arr = (N.LmpcRobot * B)()
    for b in range(B):
        arr[b] = robot_init(cfg, x0[b], vd[b], yr[b], hg[b], int(gt[b]), gs[b])
    return arr


def plant_step(p: N.LmpcParams, robot: N.LmpcRobot, u0) -> None:
    u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(12)
    N.check(N.lib().lmpc_robot_plant_step(ctypes.byref(p), ctypes.byref(robot), _d(u0)), "lmpc_robot_plant_step")


def advance(p: N.LmpcParams, cfg: N.LmpcRolloutCfg, robot: N.LmpcRobot, u0=None) -> np.ndarray:
    """One robot's tick on the host, in place (lmpc_robot_advance) -> the Raibert foot targets [4, 3] (world)."""
    tgt = np.zeros(12)
    uptr = None
    if u0 is not None:
        u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(12)
        uptr = _d(u0)
    N.check(N.lib().lmpc_robot_advance(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(robot), uptr, _d(tgt)),
            "lmpc_robot_advance")
    return tgt.reshape(4, 3)


def robot_state(robot: N.LmpcRobot) -> np.ndarray:
    """[euler, pos, omega, v] of a robot."""
    s = robot.cmd.state
    return np.array(list(s.root_euler) + list(s.root_pos) + list(s.root_ang_vel) + list(s.root_lin_vel))


# ---- host <-> device and log views -------------------------------------------------------------------------------
def to_bytes(structs) -> np.ndarray:
    """ctypes array of LmpcRobot / LmpcCommand -> uint8 [B, sizeof] (a copy)."""
    n = len(structs)
    return np.frombuffer(bytes(structs), dtype=np.uint8).reshape(n, -1).copy()


def to_device(structs, device=None):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return torch.from_numpy(to_bytes(structs)).to(dev)


def robots_from(buf):
    """uint8 [B, ROBOT_BYTES] (torch or NumPy) -> ctypes array of LmpcRobot (a copy on the host)."""
    return D.host_structs(buf, N.LmpcRobot)


def commands_from(buf):
    """uint8 [..., COMMAND_BYTES] (torch or NumPy) -> flat ctypes array of LmpcCommand (a copy on the host)."""
    return D.host_structs(buf, N.LmpcCommand)


ROBOT_DTYPE = np.dtype({
    "names": ["euler", "pos", "omega", "vel", "rot", "foot_abs", "euler_d", "pos_d", "vel_d_rel", "omega_d_rel",
              "gait_phase", "gait_speed", "gait", "plan_contacts", "foot_pos_world", "swing_start_world", "fsm_start",
              "fsm_index", "tick"],
    "formats": ["3f8", "3f8", "3f8", "3f8", "9f8", "12f8", "3f8", "3f8", "3f8", "3f8", "4f8", "f8", "i4", "4u1",
                "12f8", "12f8", "4f8", "4i4", "i4"],
    "offsets": [0, 24, 48, 72, 96, 168, 264, 288, 312, 336, 360, 392, 400, 404, 408, 504, 600, 632, 648],
    "itemsize": 656,
})
COMMAND_DTYPE = np.dtype({"names": ROBOT_DTYPE.names[:14], "formats": [ROBOT_DTYPE[n] for n in ROBOT_DTYPE.names[:14]],
                          "offsets": [ROBOT_DTYPE.fields[n][1] for n in ROBOT_DTYPE.names[:14]], "itemsize": 408})


def robots_view(buf) -> np.ndarray:
    """uint8 [..., ROBOT_BYTES] -> NumPy structured array [...] with the fields of lmpc_robot (ROBOT_DTYPE)."""
    return D.host_view(buf, ROBOT_DTYPE)


def commands_view(buf) -> np.ndarray:
    """uint8 [..., COMMAND_BYTES] -> NumPy structured array [...] with the fields of lmpc_command."""
    return D.host_view(buf, COMMAND_DTYPE)


@dataclass
class RolloutLog:
    """Device tensors of one rollout, [ticks, batch, ...] (lmpc_rollout_log)."""
    cmd: "object"     # uint8 [ticks, B, COMMAND_BYTES]
    u0: "object"      # f64 [ticks, B, 12]
    x: "object"       # f64 [ticks, B, 12], after the plant step
    status: "object"  # i32 [ticks, B]
    iters: "object"   # i32 [ticks, B]: interior-point iterations | polish rounds << 16

    def struct(self) -> N.LmpcRolloutLog:
        return N.LmpcRolloutLog(self.cmd.data_ptr(), self.u0.data_ptr(), self.x.data_ptr(), self.status.data_ptr(),
                                self.iters.data_ptr())

    def numpy(self) -> dict:
        return dict(cmd=commands_view(self.cmd), u0=self.u0.cpu().numpy(), x=self.x.cpu().numpy(),
                    status=self.status.cpu().numpy(), iters=self.iters.cpu().numpy())


def alloc_log(ticks: int, batch: int, device) -> RolloutLog:
    import torch

    return RolloutLog(cmd=torch.zeros((ticks, batch, N.COMMAND_BYTES), dtype=torch.uint8, device=device),
                      u0=torch.zeros((ticks, batch, 12), dtype=torch.float64, device=device),
                      x=torch.zeros((ticks, batch, 12), dtype=torch.float64, device=device),
                      status=torch.zeros((ticks, batch), dtype=torch.int32, device=device),
                      iters=torch.zeros((ticks, batch), dtype=torch.int32, device=device))
