"""Torques and a contact set -> accelerations, contact forces and the next state (include/lmpc/lmpc_sim.h).

The rigid-body plant over the dynamics terms of `rbd`: a contact-constrained forward dynamics, a time-stepping
integrator on top of it, and a device loop that closes the whole-body controller around it.

  * `cfg()` -- `lmpc_sim_cfg` (dt 0.002, ground_z 0, unilateral on unless given);
  * `forward_dynamics()`, `step()` -- one robot on the host (the same arithmetic, compiled for the CPU);
  * `forward_dynamics_device()`, `step_device()` -- a batch resident in HBM, asynchronous on a stream; tau and the
    candidate contacts may be strided views (the WBC's x, the packed targets): no gather;
  * `WbcSim` -- per tick, on one stream and without a host synchronisation: state -> WBC torques -> plant step.

The contact rule is fixed and deterministic, not a complementarity solution: feet whose normal force comes out
negative are released and never re-added within a step, the friction cone is not enforced, and held feet drift by
O(dt^2) per step (include/lmpc/lmpc_sim.h).  The plant step that does solve a friction-cone complementarity problem is
`contact.step` / `contact.step_device` (include/lmpc/lmpc_contact.h); `WbcSim(..., contact=contact.cfg())` runs on it.
The device functions are HIP kernels; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from .rbd import STATE_BYTES, TARGET_BYTES, WbcPipeline

CFG_BYTES = ctypes.sizeof(N.LmpcSimCfg)  # 24
OUT_BYTES = ctypes.sizeof(N.LmpcSimOut)  # 472
TAU_OFFSET = 30                          # tau within x = [qdd (18), F (12), tau (12)]
CONTACT_OFFSET = N.LmpcWbcTarget.contact.offset // 4  # lmpc_wbc_target.contact, in int32s (84)

OUT_SHAPES = {"qdd": (18,), "force": (12,), "foot_pos": (12,), "foot_vel": (12,)}


def cfg(dt=None, ground_z=None, unilateral=None) -> N.LmpcSimCfg:
    c = N.LmpcSimCfg()
    N.lib().lmpc_sim_cfg_default(ctypes.byref(c))
    if dt is not None:
        c.dt = float(dt)
    if ground_z is not None:
        c.ground_z = float(ground_z)
    if unilateral is not None:
        c.unilateral = int(bool(unilateral))
    return c


def out_dict(o: N.LmpcSimOut) -> dict:
    d = {k: np.array(getattr(o, k), dtype=np.float64).reshape(shp) for k, shp in OUT_SHAPES.items()}
    d["held"] = np.array(o.held, dtype=np.int32)
    d["touch"] = np.array(o.touch, dtype=np.int32)
    d["status"] = int(o.status)
    return d


def _tau_contact(tau, contact):
    t = (ctypes.c_double * 12)(*[float(v) for v in np.asarray(tau, dtype=np.float64).reshape(12)])
    c = (ctypes.c_int32 * 4)(*[int(bool(v)) for v in contact])
    return t, c


def forward_dynamics(model, st, tau, contact, unilateral=True) -> N.LmpcSimOut:
    """One robot's contact-constrained forward dynamics on the host (lmpc_rbd_forward_dynamics)."""
    t, c = _tau_contact(tau, contact)
    o = N.LmpcSimOut()
    N.check(N.lib().lmpc_rbd_forward_dynamics(ctypes.byref(model), ctypes.byref(st), t, c, int(bool(unilateral)),
                                              ctypes.byref(o)), "lmpc_rbd_forward_dynamics")
    return o


def step(model, c: N.LmpcSimCfg, st, tau, contact, substeps: int = 1):
    """One robot's plant step on the host (lmpc_sim_step) -> (next state, lmpc_sim_out).  substeps > 1 chains that
    many calls with tau and the candidates held, as the device function's `substeps` does."""
    if substeps < 1:
        raise ValueError("substeps must be positive")
    t, k = _tau_contact(tau, contact)
    cur, o = st, N.LmpcSimOut()
    for _ in range(substeps):
        nxt = N.LmpcRbdState()
        N.check(N.lib().lmpc_sim_step(ctypes.byref(model), ctypes.byref(c), ctypes.byref(cur), t, k, ctypes.byref(nxt),
                                      ctypes.byref(o)), "lmpc_sim_step")
        cur = nxt
    return cur, o


def _common(d_state, d_tau, d_contact, d_out, out_optional):
    """The checks the two plant functions share -> (B, device, tau's row stride, the contacts' row stride)."""
    import torch

    B, dev = D.batch("d_state", d_state)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    ts = D.view("d_tau", d_tau, torch.float64, B, 12, dev)
    cs = D.view("d_contact", d_contact, torch.int32, B, 4, dev)
    D.check("d_out", d_out, torch.uint8, (B, OUT_BYTES), dev, optional=out_optional)
    return B, dev, ts, cs


def forward_dynamics_device(model, d_state, d_tau, d_contact, d_out, unilateral=True, stream=None):
    """A batch of forward dynamics on the device (lmpc_rbd_forward_dynamics_device): d_state uint8 [B][288], d_tau
    float64 [B][12] and d_contact int32 [B][4] (views with any row stride), d_out uint8 [B][472]."""
    B, dev, ts, cs = _common(d_state, d_tau, d_contact, d_out, False)
    N.check(N.lib().lmpc_rbd_forward_dynamics_device(
        ctypes.byref(model), d_state.data_ptr(), d_tau.data_ptr(), ts, d_contact.data_ptr(), cs, B,
        int(bool(unilateral)), d_out.data_ptr(), D.stream(stream, dev)), "lmpc_rbd_forward_dynamics_device")


def step_device(model, c: N.LmpcSimCfg, d_state, d_tau, d_contact, d_next, d_out=None, substeps: int = 1, stream=None):
    """A batch of plant steps on the device (lmpc_sim_step_device): as forward_dynamics_device, plus d_next uint8
    [B][288] (may be d_state itself); d_out may be None."""
    import torch

    B, dev, ts, cs = _common(d_state, d_tau, d_contact, d_out, True)
    D.check("d_next", d_next, torch.uint8, (B, STATE_BYTES), dev)
    N.check(N.lib().lmpc_sim_step_device(
        ctypes.byref(model), ctypes.byref(c), d_state.data_ptr(), d_tau.data_ptr(), ts, d_contact.data_ptr(), cs, B,
        int(substeps), d_next.data_ptr(), D.ptr(d_out), None, 0, D.stream(stream, dev)), "lmpc_sim_step_device")


def target_contacts(d_target):
    """The int32 [B][4] view of lmpc_wbc_target.contact inside packed targets (uint8 [B][352])."""
    import torch

    return d_target.view(torch.int32)[:, CONTACT_OFFSET:CONTACT_OFFSET + 4]


def flags_view(d_out):
    """The int32 [...][10] view of the tail of lmpc_sim_out inside packed outputs (uint8 [...][472]): held (4), touch
    (4), status, reserved."""
    import torch

    return d_out.view(torch.int32)[..., N.LmpcSimOut.held.offset // 4:]


class WbcSim:
    """The whole-body controller closed around the plant, device-resident: per tick `WbcPipeline.solve_device`
    (state -> torques), then `lmpc_sim_step_device` with tau read by stride from the pipeline's x and the candidate
    contacts by stride from the targets -- on one stream, with no host synchronisation in between."""

    def __init__(self, model: N.LmpcRbdModel, max_batch: int, c: N.LmpcSimCfg = None, device: int = 0, contact=None,
                 warm: bool = False):
        """contact: an `lmpc_contact_cfg` (contact.cfg(...)) steps the plant with the frictional contact model
        (`lmpc_contact_step_device`, the targets' contacts as its mask) and `c` is not used; None: the present plant.
        warm: `WbcPipeline(warm=True)`, every tick's hierarchical solve starts from the last tick's active sets."""
        import torch

        self.model = model
        self.cfg = c if c is not None else cfg()
        self.contact = contact
        self.max_batch = int(max_batch)
        self.device = device
        self.pipeline = WbcPipeline(model, max_batch, device, warm=warm)
        self.d_out = torch.empty((self.max_batch, OUT_BYTES), dtype=torch.uint8, device=torch.device("cuda", device))

    def close(self):
        self.pipeline.close()

    def run_device(self, d_state, d_target, ticks: int, substeps: int = 1, log: bool = False, stream=None):
        """`ticks` controller ticks of cfg.dt * substeps each; d_state (uint8 [B][288]) is updated in place.  The
        targets stay as given.  log=True -> dict of device tensors, one row per tick: states uint8 [ticks][B][288]
        (after the tick), held / touch int32 [ticks][B][4], wbc_status / sim_status int32 [ticks][B], x float64
        [ticks][B][42] (the tick's WBC solution) and wbc_iters int32 [ticks][B][3] (its iteration words)."""
        import torch

        B, dev = D.batch("d_state", d_state, self.max_batch, self.device)
        if ticks < 0:
            raise ValueError("ticks must not be negative")
        D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
        D.check("d_target", d_target, torch.uint8, (B, TARGET_BYTES), dev)
        s = D.torch_stream(stream, dev)
        d_contact = target_contacts(d_target)
        d_out = self.d_out[:B]
        logs = None
        if log:
            def buf(dtype, *tail):
                return torch.empty((ticks, B) + tail, dtype=dtype, device=dev)

            logs = dict(states=buf(torch.uint8, STATE_BYTES), held=buf(torch.int32, 4), touch=buf(torch.int32, 4),
                        wbc_status=buf(torch.int32), sim_status=buf(torch.int32),
                        x=buf(torch.float64, self.pipeline.d_levels.shape[2]),
                        wbc_iters=buf(torch.int32, self.pipeline.d_iters.shape[1]))
            flags = flags_view(d_out)
        with torch.cuda.stream(s):
            for t in range(ticks):
                d_x, d_status = self.pipeline.solve_device(d_state, d_target, s)
                if self.contact is None:
                    step_device(self.model, self.cfg, d_state, d_x[:, TAU_OFFSET:TAU_OFFSET + 12], d_contact, d_state,
                                d_out, substeps, s)
                else:
                    from . import contact as C

                    C.step_device(self.model, self.contact, d_state, d_x[:, TAU_OFFSET:TAU_OFFSET + 12], d_contact,
                                  d_state, d_out, None, substeps, s)
                if log:
                    logs["x"][t].copy_(d_x)
                    logs["wbc_iters"][t].copy_(self.pipeline.d_iters[:B])
                    logs["states"][t].copy_(d_state)
                    logs["held"][t].copy_(flags[:, 0:4])
                    logs["touch"][t].copy_(flags[:, 4:8])
                    logs["wbc_status"][t].copy_(d_status)
                    logs["sim_status"][t].copy_(flags[:, 8])
        return logs
