"""Robot state -> the WBC's dynamics terms -> torques (include/lmpc/lmpc_rbd.h).

The reference takes the mass matrix, the nonlinear effects, the foot Jacobians and dJ v from Pinocchio
(wbc.cpp:59-91) and derives the base-acceleration and swing-leg targets from them (wbc.cpp:177-246).  Here a batched
floating-base rigid-body dynamics kernel (lmpc_rbd.hip) produces all of them from `measured_rbd_state`, as the
`lmpc_wbc_input` blocks that `wbc.records_device` turns into hierarchical-QP records:

  * `model_go1()`, `model_a1()`, `model_from_json()` -- the robot (`lmpc_rbd_model`);
  * `state()`, `target()` -- one robot's `lmpc_rbd_state` / `lmpc_wbc_target`; `pack()` -- a batch of either as the
    uint8 array the device functions take;
  * `compute()`, `wbc_input_from_state()` -- one robot on the host (the same arithmetic, compiled for the CPU);
  * `compute_device()`, `wbc_inputs_device()` -- a batch resident in HBM, asynchronous on a stream;
  * `WbcPipeline` -- state -> inputs -> records -> hierarchical solve on one stream, x = [qdd (18), F (12), tau (12)].

Coordinates, definitions and the Euler singularity (|pitch| < pi/2): include/lmpc/lmpc_rbd.h.  The device functions
are HIP kernels; there is no CPU fallback behind them.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import _device as D
from . import _native as N
from .hoqp import HoqpBatch
from .wbc import WBC_RECORD_LEN

MODEL_BYTES = ctypes.sizeof(N.LmpcRbdModel)    # 1432
STATE_BYTES = ctypes.sizeof(N.LmpcRbdState)    # 288
TARGET_BYTES = ctypes.sizeof(N.LmpcWbcTarget)  # 352
TERMS_BYTES = ctypes.sizeof(N.LmpcRbdTerms)    # 5072
INPUT_BYTES = ctypes.sizeof(N.LmpcWbcInput)    # 4848


def model_go1() -> N.LmpcRbdModel:
    m = N.LmpcRbdModel()
    N.lib().lmpc_rbd_model_go1(ctypes.byref(m))
    return m


def model_a1() -> N.LmpcRbdModel:
    m = N.LmpcRbdModel()
    N.lib().lmpc_rbd_model_a1(ctypes.byref(m))
    return m


def model_from_json(path_or_dict) -> N.LmpcRbdModel:
    """A model written by tools/urdf_to_rbd.py."""
    d = path_or_dict if isinstance(path_or_dict, dict) else json.load(open(path_or_dict))
    m = N.LmpcRbdModel()
    m.mass[:] = d["mass"]
    for name in ("com", "inertia", "joint_origin", "foot"):
        rows = getattr(m, name)
        for i, row in enumerate(d[name]):
            rows[i][:] = row
    m.gravity = d.get("gravity", 9.81)
    return m


def state(euler_zyx, pos, joint_pos, omega_world, lin_vel_world, joint_vel) -> N.LmpcRbdState:
    """measured_rbd_state (BaseInterface.cpp:511-518): euler = (yaw, pitch, roll); joints in the order FL FR RL RR."""
    s = N.LmpcRbdState()
    s.euler[:] = [float(v) for v in euler_zyx]
    s.pos[:] = [float(v) for v in pos]
    s.joint_pos[:] = [float(v) for v in joint_pos]
    s.omega[:] = [float(v) for v in omega_world]
    s.lin_vel[:] = [float(v) for v in lin_vel_world]
    s.joint_vel[:] = [float(v) for v in joint_vel]
    return s


def state_from_vector(x) -> N.LmpcRbdState:
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(36)
    return N.LmpcRbdState.from_buffer_copy(x.tobytes())


def target(forces_des=None, foot_pos_des=None, foot_vel_des=None, contact=(1, 1, 1, 1), torque_limits=None, mu=None,
           swing_kp=None, swing_kd=None) -> N.LmpcWbcTarget:
    """lmpc_wbc_target with config/task.info's constants (lmpc_wbc_target_default) unless given."""
    t = N.LmpcWbcTarget()
    N.lib().lmpc_wbc_target_default(ctypes.byref(t))
    for name, v in (("forces_des", forces_des), ("foot_pos_des", foot_pos_des), ("foot_vel_des", foot_vel_des)):
        if v is not None:
            getattr(t, name)[:] = [float(x) for x in np.asarray(v, dtype=np.float64).reshape(12)]
    if torque_limits is not None:
        t.torque_limits[:] = [float(v) for v in torque_limits]
    if mu is not None:
        t.mu = float(mu)
    if swing_kp is not None:
        t.swing_kp = float(swing_kp)
    if swing_kd is not None:
        t.swing_kd = float(swing_kd)
    t.contact[:] = [int(bool(c)) for c in contact]
    return t


def pack(structs) -> np.ndarray:
    """A list of equal ctypes structs (states, targets) -> uint8 [B][sizeof]: `torch.from_numpy(...).to(device)`."""
    size = ctypes.sizeof(structs[0])
    out = np.empty((len(structs), size), dtype=np.uint8)
    for i, s in enumerate(structs):
        out[i] = np.frombuffer(bytes(s), dtype=np.uint8)
    return out


def _fields(struct, shapes) -> dict:
    return {k: np.array(getattr(struct, k), dtype=np.float64).reshape(shp) if shp != () else float(getattr(struct, k))
            for k, shp in shapes.items()}


TERMS_SHAPES = {"M": (18, 18), "nle": (18,), "J": (12, 18), "dJv": (12,), "foot_pos": (12,), "foot_vel": (12,),
                "com": (3,), "Ab": (6, 6), "mass": ()}
INPUT_SHAPES = {"M": (18, 18), "nle": (18,), "J": (12, 18), "dJv": (12,), "base_accel": (6,), "swing_acc": (12,),
                "forces_des": (12,), "torque_limits": (3,), "mu": ()}


def terms_dict(t: N.LmpcRbdTerms) -> dict:
    return _fields(t, TERMS_SHAPES)


def input_dict(s: N.LmpcWbcInput) -> dict:
    d = _fields(s, INPUT_SHAPES)
    d["contact"] = np.array(s.contact, dtype=np.int32)
    return d


def compute(model: N.LmpcRbdModel, st: N.LmpcRbdState) -> N.LmpcRbdTerms:
    """One robot's dynamics terms on the host (lmpc_rbd_compute)."""
    t = N.LmpcRbdTerms()
    N.check(N.lib().lmpc_rbd_compute(ctypes.byref(model), ctypes.byref(st), ctypes.byref(t)), "lmpc_rbd_compute")
    return t


def wbc_input_from_state(model: N.LmpcRbdModel, st: N.LmpcRbdState, tg: N.LmpcWbcTarget) -> N.LmpcWbcInput:
    """One robot's WBC input block on the host (lmpc_wbc_input_from_state)."""
    s = N.LmpcWbcInput()
    N.check(N.lib().lmpc_wbc_input_from_state(ctypes.byref(model), ctypes.byref(st), ctypes.byref(tg), ctypes.byref(s)),
            "lmpc_wbc_input_from_state")
    return s


def wbc_inputs_device(model, d_state, d_target, d_inputs, stream=None):
    """A batch of WBC input blocks on the device (lmpc_wbc_inputs_device): d_state uint8 [B][288], d_target uint8
    [B][352], d_inputs uint8 [B][4848], all in HBM; asynchronous on `stream` (default: torch's current)."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_target", d_target, torch.uint8, (B, TARGET_BYTES), dev)
    D.check("d_inputs", d_inputs, torch.uint8, (B, INPUT_BYTES), dev)
    N.check(N.lib().lmpc_wbc_inputs_device(ctypes.byref(model), d_state.data_ptr(), d_target.data_ptr(), B,
                                           d_inputs.data_ptr(), D.stream(stream, dev)), "lmpc_wbc_inputs_device")


def compute_device(model, d_state, d_terms, stream=None):
    """A batch of dynamics terms on the device (lmpc_rbd_compute_device): d_state uint8 [B][288], d_terms uint8
    [B][5072]."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_terms", d_terms, torch.uint8, (B, TERMS_BYTES), dev)
    N.check(N.lib().lmpc_rbd_compute_device(ctypes.byref(model), d_state.data_ptr(), B, d_terms.data_ptr(),
                                            D.stream(stream, dev)), "lmpc_rbd_compute_device")


class WbcPipeline:
    """state -> lmpc_wbc_input -> WBC records -> hierarchical QP, device-resident, on one stream.

    The intermediate buffers (inputs, records, every level's x, slacks) are allocated once for `max_batch` robots.

    warm=True: the hierarchical solve starts every level from the active set the robot's previous solve left
    (lmpc_hoqp_solve_device_warm).  The pipeline owns the blocks (`d_act`, zeroed = no set); `reset_warm()` zeroes
    them, and so does a call with another batch size (the rows then belong to other robots)."""

    def __init__(self, model: N.LmpcRbdModel, max_batch: int, device: int = 0, warm: bool = False):
        import torch

        if max_batch < 1:
            raise ValueError("max_batch must be positive")
        self.model = model
        self.max_batch = int(max_batch)
        self.device = device
        dev = torch.device("cuda", device)
        dims = N.LmpcHoqpDims()
        N.lib().lmpc_hoqp_dims_wbc(ctypes.byref(dims))
        self.solver = HoqpBatch(dims, self.max_batch, device)
        self.d_inputs = torch.empty((self.max_batch, INPUT_BYTES), dtype=torch.uint8, device=dev)
        self.d_records = torch.empty((self.max_batch, WBC_RECORD_LEN), dtype=torch.float64, device=dev)
        self.d_levels = torch.empty((self.max_batch, dims.num_levels, dims.num_vars), dtype=torch.float64, device=dev)
        self.d_slack = torch.empty((self.max_batch, max(self.solver.slack_len, 1)), dtype=torch.float64, device=dev)
        self.d_status = torch.empty(self.max_batch, dtype=torch.int32, device=dev)
        self.d_iters = torch.empty((self.max_batch, dims.num_levels), dtype=torch.int32, device=dev)
        self.warm = bool(warm)
        self.d_act = None
        self._warm_batch = 0
        if self.warm:
            self.d_act = torch.zeros((self.max_batch, self.solver.act_len), dtype=torch.int64, device=dev)

    def reset_warm(self):
        """Forget every robot's carried active sets: the next solve is a cold one."""
        if self.d_act is not None:
            self.d_act.zero_()

    def close(self):
        self.solver.close()

    def solve_device(self, d_state, d_target, stream=None):
        """d_state uint8 [B][288], d_target uint8 [B][352] (B <= max_batch) -> (x [B][42], status [B]): views of the
        pipeline's own buffers, valid until the next call, ready when `stream` reaches this point."""
        import torch
        from .wbc import records_device

        B, dev = D.batch("d_state", d_state, self.max_batch, self.device)
        s = D.torch_stream(stream, dev)
        wbc_inputs_device(self.model, d_state, d_target, self.d_inputs[:B], s)
        records_device(self.d_inputs[:B], self.d_records[:B], s)
        d_act = None
        if self.warm:
            if B != self._warm_batch:
                with torch.cuda.stream(s):
                    self.d_act.zero_()
                self._warm_batch = B
            d_act = self.d_act[:B]
        self.solver.solve_device(self.d_records[:B], self.d_levels[:B], self.d_slack[:B], self.d_status[:B],
                                 self.d_iters[:B], s, d_act=d_act)
        return self.d_levels[:B, -1], self.d_status[:B]
