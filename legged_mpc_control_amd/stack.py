"""The full loop on the device: MPC -> whole-body controller -> rigid-body plant (include/lmpc/lmpc_stack.h).

  * `robot_init()`, `advance()`, `targets()` -- one robot's MPC tick on the host (the arithmetic the device kernels
    share): feedback from the measured state and the plant's `touch` flags, Raibert target, the leg FSMs with early
    touchdown and their foot targets; then the WBC's targets from the QP's u_0 and those FSM targets;
  * `advance_device()`, `solve_device()`, `targets_device()`, `candidates_device()` -- the same for a batch resident in
    HBM, asynchronous on a stream; the advance launch also expands the commands into the MPC context's record buffers;
  * `StackLoop` -- per MPC tick: advance, QP, targets, then `wbc_per_mpc` low-level ticks of `WbcPipeline.solve_device`
    and `lmpc_sim_step_device`, the plant's candidate contacts being `held | touch` of its previous step; one stream,
    no host synchronisation and no allocation inside the loop.  With `estimator=est.cfg()` the controllers no longer
    see the plant's state: after every plant step the loop reads sensors off the plant (`est.sensors_from_plant_device`)
    and runs the reference's Kalman filter (`est.update_device`); the advance and the WBC then read the estimated
    state and a shadow `lmpc_sim_out` with the estimate's feet and contact flags, while the plant and the candidate
    rule keep reading the true ones.  With `plant=contact.cfg()` the plant step is `lmpc_contact_step_device` (the
    frictional contact model, include/lmpc/lmpc_contact.h): every foot is in its mask on every step and the candidate
    launch is gone.  With `low_level=lowlevel.cfg_go1(model)` the low-level tick is the reference's joint-PD controller
    (`lmpc_lowlevel_device`, include/lmpc/lmpc_lowlevel.h) instead of the whole-body controller: one launch that also
    writes the candidates, then the plant, which reads the torques from the controller's output block by stride.  With
    `fused_low_level=True` on top of it the `wbc_per_mpc` controller + plant launches of an MPC tick are one launch
    (`lowsim.run_device`, include/lmpc/lmpc_lowsim.h) that leaves the same bits.

What is restated from the reference and what is this library's choice (zero latency, the candidate rule, `touch` as
the contact flag, the standing mode's foot targets, what a failed stage leaves): include/lmpc/lmpc_stack.h.  The
device functions are HIP kernels; there is no CPU fallback behind them.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _device as D
from . import _native as N
from . import contact as C
from . import est as E
from . import lowlevel as LL
from . import lowsim as LS
from . import sim as S
from .rbd import STATE_BYTES, TARGET_BYTES, WbcPipeline, target as wbc_target
from .solver import BatchedConvexQPSolver

ROBOT_BYTES = N.STACK_ROBOT_BYTES  # 960
_dp = ctypes.POINTER(ctypes.c_double)

STACK_ROBOT_DTYPE = np.dtype({
    "names": ["euler", "pos", "omega", "vel", "rot", "foot_abs", "euler_d", "pos_d", "vel_d_rel", "omega_d_rel",
              "gait_phase", "gait_speed", "gait", "plan_contacts", "foot_pos_world", "swing_start_world", "fsm_start",
              "fsm_index", "tick", "fsm_pos_target", "fsm_vel_target", "swing_end_world", "not_first_call"],
    "formats": ["3f8", "3f8", "3f8", "3f8", "9f8", "12f8", "3f8", "3f8", "3f8", "3f8", "4f8", "f8", "i4", "4u1",
                "12f8", "12f8", "4f8", "4i4", "i4", "12f8", "12f8", "12f8", "4i4"],
    "offsets": [0, 24, 48, 72, 96, 168, 264, 288, 312, 336, 360, 392, 400, 404, 408, 504, 600, 632, 648, 656, 752, 848,
                944],
    "itemsize": 960,
})


def _d(a):
    return a.ctypes.data_as(_dp)


def check_rates(params: N.LmpcParams, sim_cfg: N.LmpcSimCfg, wbc_per_mpc: int, substeps: int = 1) -> None:
    """ValueError unless wbc_per_mpc * substeps * sim_cfg.dt == params.dt to 1e-12 (lmpc_stack_check_rates)."""
    if N.lib().lmpc_stack_check_rates(ctypes.byref(params), ctypes.byref(sim_cfg), int(wbc_per_mpc), int(substeps)) != 0:
        raise ValueError(f"wbc_per_mpc {wbc_per_mpc} x substeps {substeps} x sim dt {sim_cfg.dt} is not the MPC's dt "
                         f"{params.dt}")


def robot_init(cfg: N.LmpcRolloutCfg, model: N.LmpcRbdModel, state: N.LmpcRbdState, vel_d=(0.0, 0.0),
               yaw_rate: float = 0.0, height: float = 0.30, gait: int = N.GAIT_TROT, gait_speed: float = 4.0):
    """One robot in `state` with its FSMs at reset -> (LmpcStackRobot, the first LmpcSimOut) (lmpc_stack_robot_init)."""
    rb, out = N.LmpcStackRobot(), N.LmpcSimOut()
    vd = np.ascontiguousarray(vel_d, dtype=np.float64).reshape(2)
    N.check(N.lib().lmpc_stack_robot_init(ctypes.byref(cfg), ctypes.byref(model), ctypes.byref(state), _d(vd),
                                          float(yaw_rate), float(height), int(gait), float(gait_speed), ctypes.byref(rb),
                                          ctypes.byref(out)), "lmpc_stack_robot_init")
    return rb, out


def advance(p: N.LmpcParams, cfg: N.LmpcRolloutCfg, robot: N.LmpcStackRobot, state: N.LmpcRbdState,
            out: N.LmpcSimOut) -> np.ndarray:
    """One robot's MPC tick before the solve, on the host, in place (lmpc_stack_advance) -> the Raibert foot targets
    [4, 3] (world)."""
    tgt = np.zeros(12)
    N.check(N.lib().lmpc_stack_advance(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(robot), ctypes.byref(state),
                                       ctypes.byref(out), _d(tgt)), "lmpc_stack_advance")
    return tgt.reshape(4, 3)


def targets(robot: N.LmpcStackRobot, u0, template: N.LmpcWbcTarget = None) -> N.LmpcWbcTarget:
    """One robot's WBC targets after the solve, on the host (lmpc_stack_targets)."""
    tmpl = template if template is not None else wbc_target()
    u0 = np.ascontiguousarray(u0, dtype=np.float64).reshape(12)
    t = N.LmpcWbcTarget()
    N.check(N.lib().lmpc_stack_targets(ctypes.byref(robot), _d(u0), ctypes.byref(tmpl), ctypes.byref(t)),
            "lmpc_stack_targets")
    return t


# ---- host <-> device ---------------------------------------------------------------------------------------------
def to_bytes(structs) -> np.ndarray:
    """A list or ctypes array of equal structs -> uint8 [B, sizeof] (a copy)."""
    return np.stack([np.frombuffer(bytes(s), dtype=np.uint8) for s in structs])


def robots_from(buf):
    """uint8 [B, 960] (torch or NumPy) -> ctypes array of LmpcStackRobot (a copy on the host)."""
    return D.host_structs(buf, N.LmpcStackRobot)


def robots_view(buf) -> np.ndarray:
    """uint8 [..., 960] -> NumPy structured array [...] with the fields of lmpc_stack_robot (STACK_ROBOT_DTYPE)."""
    return D.host_view(buf, STACK_ROBOT_DTYPE)


def advance_device(solver: BatchedConvexQPSolver, cfg: N.LmpcRolloutCfg, d_robots, d_state, d_sim_out, stream=None):
    """A batch of advances on the device (lmpc_stack_advance_device): d_robots uint8 [B][960] (in place), d_state uint8
    [B][288], d_sim_out uint8 [B][472].  The commands are expanded into `solver`'s own record buffers, which
    `solve_device` then solves."""
    import torch

    B, dev = D.batch("d_robots", d_robots, device=solver.device)
    D.check("d_robots", d_robots, torch.uint8, (B, ROBOT_BYTES), dev)
    D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, S.OUT_BYTES), dev)
    N.check(N.lib().lmpc_stack_advance_device(solver._ctx, ctypes.byref(cfg), d_robots.data_ptr(), d_state.data_ptr(),
                                              d_sim_out.data_ptr(), B, D.stream(stream, dev)),
            "lmpc_stack_advance_device")


def solve_device(solver: BatchedConvexQPSolver, d_grf, d_status=None, d_iters=None, stream=None):
    """Cold solves of the QPs the last `advance_device` left in `solver` (lmpc_stack_solve_device): d_grf float64
    [B][H][12], d_status / d_iters int32 [B] or None."""
    import torch

    B, dev = D.batch("d_grf", d_grf, device=solver.device)
    D.check("d_grf", d_grf, torch.float64, (B, solver.H, 12), dev)
    D.check("d_status", d_status, torch.int32, (B,), dev, optional=True)
    D.check("d_iters", d_iters, torch.int32, (B,), dev, optional=True)
    N.check(N.lib().lmpc_stack_solve_device(solver._ctx, B, d_grf.data_ptr(), D.ptr(d_status), D.ptr(d_iters),
                                            D.stream(stream, dev)), "lmpc_stack_solve_device")


def context_records(solver: BatchedConvexQPSolver, batch: int, stream=None):
    """Copies (device tensors, on the solver's device) of the first `batch` records [batch][33 + 12 H] and contact
    schedules [batch][H][4] in `solver`'s own buffers, as the last expansion left them
    (lmpc_stack_copy_records_device)."""
    import torch

    dev = torch.device("cuda", solver.device)
    d_rec = torch.empty((batch, solver.record_len), dtype=torch.float64, device=dev)
    d_con = torch.empty((batch, solver.H, 4), dtype=torch.uint8, device=dev)
    N.check(N.lib().lmpc_stack_copy_records_device(solver._ctx, int(batch), d_rec.data_ptr(), d_con.data_ptr(),
                                                   D.stream(stream, dev)), "lmpc_stack_copy_records_device")
    return d_rec, d_con


def targets_device(d_robots, d_grf, template: N.LmpcWbcTarget, d_target, stream=None):
    """A batch of WBC targets on the device (lmpc_stack_targets_device): d_robots uint8 [B][960]; d_grf float64
    [B][H][12] or [B][12] (u_0 is read by stride); d_target uint8 [B][352]."""
    import torch

    B, dev = D.batch("d_robots", d_robots)
    D.check("d_robots", d_robots, torch.uint8, (B, ROBOT_BYTES), dev)
    D.check("d_target", d_target, torch.uint8, (B, TARGET_BYTES), dev)
    horizon = tuple(getattr(d_grf, "shape", ()))[1:2]  # (H,) of a 3-d d_grf: any H
    D.check("d_grf", d_grf, torch.float64, (B, 12), dev, allow_shape=(B,) + horizon + (12,))
    N.check(N.lib().lmpc_stack_targets_device(d_robots.data_ptr(), d_grf.data_ptr(), d_grf.numel() // B,
                                              ctypes.byref(template), B, d_target.data_ptr(), D.stream(stream, dev)),
            "lmpc_stack_targets_device")


def candidates_device(d_sim_out, d_candidates, stream=None):
    """held | touch of the plant's last step -> the next step's candidate contacts (lmpc_stack_candidates_device):
    d_sim_out uint8 [B][472], d_candidates int32 [B][4]."""
    import torch

    B, dev = D.batch("d_sim_out", d_sim_out)
    D.check("d_sim_out", d_sim_out, torch.uint8, (B, S.OUT_BYTES), dev)
    D.check("d_candidates", d_candidates, torch.int32, (B, 4), dev)
    N.check(N.lib().lmpc_stack_candidates_device(d_sim_out.data_ptr(), B, d_candidates.data_ptr(),
                                                 D.stream(stream, dev)), "lmpc_stack_candidates_device")


class StackLoop:
    """The MPC, the whole-body controller and the plant closed into one device-resident loop.

    Owns an MPC context (cold solves on the context's normal routing), a `WbcPipeline` (or, with `low_level`, the
    joint-PD controller's output block) and the target / candidate / force buffers, all allocated once for `max_batch`
    robots."""

    def __init__(self, model: N.LmpcRbdModel, params: N.LmpcParams, horizon: int, max_batch: int,
                 rollout_cfg: N.LmpcRolloutCfg, sim_cfg: N.LmpcSimCfg, wbc_per_mpc: int, substeps: int = 1,
                 template: N.LmpcWbcTarget = None, device: int = 0, estimator: N.LmpcEstCfg = None,
                 plant: N.LmpcContactCfg = None, plant_split: bool = False, wbc_warm: bool = False,
                 low_level: N.LmpcLowlevelCfg = None, fused_low_level: bool = False):
        """estimator: an `lmpc_est_cfg` (est.cfg(dt=...)) closes the loop on the Kalman filter's estimate instead of the
        plant's own state; its dt must be the low-level tick's, substeps * sim_cfg.dt.  None: the plant's state is the
        feedback, exactly as without this option.

        plant: an `lmpc_contact_cfg` (contact.cfg(dt=...)) steps the plant with the frictional contact model
        (`lmpc_contact_step_device`) instead of `lmpc_sim_step_device`: every foot is in the mask on every step, so the
        candidate rule and its launch are gone; its dt and ground_z must be sim_cfg's.  None: the present plant,
        exactly as without this option.  plant_split: run that step in its three-launch form on a workspace the loop
        owns (the same bits; DESIGN.md 4h has the timings of both).

        wbc_warm: the WBC solves start from the active sets of the robot's previous low-level tick
        (`WbcPipeline(warm=True)`; DESIGN.md 4c "Warm start").  False: cold solves, exactly as without this option.

        low_level: an `lmpc_lowlevel_cfg` (lowlevel.cfg_go1(model)) runs the reference's joint-PD controller in place
        of the whole-body controller: no `WbcPipeline` is allocated, the template's WBC constants are not read, and
        `wbc_warm` cannot be combined with it.  None: the whole-body controller, exactly as without this option.

        fused_low_level: with `low_level`, the `wbc_per_mpc` low-level ticks of an MPC tick run as one launch
        (`lowsim.run_device`) with the state in registers between them; buffers and logs end bit for bit as without it.
        The estimator and the contact plant sit between the ticks and are not fused: it cannot be combined with
        `estimator` or `plant`.  False: the present loop, launch for launch."""
        import torch

        if fused_low_level and low_level is None:
            raise ValueError("fused_low_level fuses the joint-PD controller with the plant: it needs low_level")
        if fused_low_level and (estimator is not None or plant is not None):
            raise ValueError("fused_low_level: the estimator and the contact plant run between the low-level ticks and are "
                             "not fused")

        if low_level is not None and wbc_warm:
            raise ValueError("wbc_warm warm-starts the whole-body controller, which low_level replaces")
        if max_batch < 1:
            raise ValueError("max_batch must be positive")
        if wbc_per_mpc < 1 or substeps < 1:
            raise ValueError("wbc_per_mpc and substeps must be positive")
        check_rates(params, sim_cfg, wbc_per_mpc, substeps)
        if plant is None and not sim_cfg.unilateral:
            raise ValueError("the loop's candidate rule needs the plant's unilateral rule (sim_cfg.unilateral = 1)")
        if plant is not None and not (abs(plant.dt - sim_cfg.dt) <= 1e-12 and plant.ground_z == sim_cfg.ground_z):
            raise ValueError(f"plant dt {plant.dt} / ground_z {plant.ground_z} are not sim_cfg's {sim_cfg.dt} / "
                             f"{sim_cfg.ground_z}")
        self.plant = plant
        self.model, self.params, self.H = model, params, int(horizon)
        self.max_batch, self.device = int(max_batch), device
        self.rollout_cfg, self.sim_cfg = rollout_cfg, sim_cfg
        self.wbc_per_mpc, self.substeps = int(wbc_per_mpc), int(substeps)
        self.template = template if template is not None else wbc_target()
        dev = torch.device("cuda", device)
        self.solver = BatchedConvexQPSolver(params, self.H, max_batch=0, device=device)
        N.check(N.lib().lmpc_stack_reserve(self.solver._ctx, self.max_batch), "lmpc_stack_reserve")
        self.low_level, self.fused_low_level = low_level, bool(fused_low_level)
        self.pipeline = WbcPipeline(model, self.max_batch, device, warm=wbc_warm) if low_level is None else None
        if low_level is not None:
            self.d_ll_out = torch.zeros((self.max_batch, LL.OUT_BYTES), dtype=torch.uint8, device=dev)
        self.d_grf = torch.zeros((self.max_batch, self.H, 12), dtype=torch.float64, device=dev)
        self.d_qp_status = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self.d_qp_iters = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self.d_target = torch.zeros((self.max_batch, TARGET_BYTES), dtype=torch.uint8, device=dev)
        self.d_candidates = torch.zeros((self.max_batch, 4), dtype=torch.int32, device=dev)
        if plant is not None:
            self.d_candidates.fill_(1)  # the mask: every foot, on every step
            self.d_contact_out = torch.zeros((self.max_batch, C.OUT_BYTES), dtype=torch.uint8, device=dev)
        self.d_plant_work = None
        if plant is not None and plant_split:
            self.d_plant_work = torch.zeros(C.work_bytes(self.max_batch), dtype=torch.uint8, device=dev)
        self.estimator = estimator
        if estimator is not None:
            if not abs(estimator.dt - self.substeps * sim_cfg.dt) <= 1e-12:
                raise ValueError(f"estimator dt {estimator.dt} is not the low-level tick's, substeps {self.substeps} x sim "
                                 f"dt {sim_cfg.dt}")

            def buf(width):
                return torch.zeros((self.max_batch, width), dtype=torch.uint8, device=dev)

            self.d_sensors, self.d_filter = buf(E.SENSORS_BYTES), buf(E.FILTER_BYTES)
            self.d_state_est, self.d_est_out, self.d_shadow = buf(STATE_BYTES), buf(E.OUT_BYTES), buf(S.OUT_BYTES)
            self.reset_estimator()

    def reset_estimator(self):
        """The next `run_device` initialises every robot's filter anew (it does so by itself on the first call, and
        when the batch size changes)."""
        self._est_batch, self._est_tick = 0, 0

    def _init_estimator(self, d_robots, d_state, d_sim_out, B, s):
        """Filters from the robots' current sensors, with pos0 = the TRUE position: this library's choice -- the
        reference's default (0, 0, 0.09) is the height of a robot lying on the ground, and these robots start
        standing.  Also leaves the first estimated state and shadow block for the first advance."""
        import torch

        E.sensors_from_plant_device(self.model, self.estimator, d_state, d_sim_out, self.d_sensors[:B], 0, 0,
                                    E.gait_view(d_robots), s)
        E.init_device(self.model, self.estimator, self.d_sensors[:B], self.d_filter[:B],
                      d_state.view(torch.float64)[:, 3:6], self.d_state_est[:B], self.d_est_out[:B], d_sim_out,
                      self.d_shadow[:B], s)
        self._est_batch, self._est_tick = B, 0

    def close(self):
        if self.pipeline is not None:
            self.pipeline.close()
        self.solver.close()

    def run_device(self, d_robots, d_state, d_sim_out, mpc_ticks: int, log: bool = False, stream=None):
        """`mpc_ticks` MPC ticks of params.dt each, every one followed by `wbc_per_mpc` low-level ticks; d_robots (uint8
        [B][960]), d_state (uint8 [B][288]) and d_sim_out (uint8 [B][472]) are updated in place, so calls chain: n + m
        ticks in one call leave the bits of n ticks followed by m.

        log=True -> dict of device tensors.  Per MPC tick t: `robots` uint8 [T][B][960] (after the advance; its first
        408 bytes are the command the QP was built from -- `cmd` is that view), `u0` float64 [T][B][12], `qp_status` /
        `qp_iters` int32 [T][B], `target` uint8 [T][B][352].  Per low-level tick k = t * wbc_per_mpc + i: `states`
        uint8 [K][B][288] and `out` uint8 [K][B][472] (after the plant step; `held`, `touch` int32 [K][B][4] and
        `sim_status` int32 [K][B] are views of it), `tau` float64 [K][B][12], `candidates` int32 [K][B][4],
        `wbc_status` int32 [K][B], `wbc_iters` int32 [K][B][3] (the iteration words of lmpc_hoqp.h); with `low_level`, in
        place of those two, `ll_out` uint8 [K][B][400] (the controller's lmpc_lowlevel_out; `ll_flags` int32 [K][B][4]
        is a view of it).  With an estimator also, per low-level tick: `sensors` uint8 [K][B][296], `state_est`
        uint8 [K][B][288], `filter` uint8 [K][B][2744] (x and P after the update; est.filter_view), `est_out` uint8
        [K][B][312] (`est_status` int32 [K][B] is a view of it), `shadow` uint8 [K][B][472]; and `filter0`,
        `state_est0`, `shadow0` [B][...]: the estimator as this call found it.  `states` and `out` stay the TRUE ones;
        the noise of low-level tick n (counted from the filters' initialisation, from 1) is keyed (seed, robot, n)."""
        import torch

        B, dev = D.batch("d_robots", d_robots, self.max_batch, self.device)
        if mpc_ticks < 0:
            raise ValueError("mpc_ticks must not be negative")
        D.check("d_robots", d_robots, torch.uint8, (B, ROBOT_BYTES), dev)
        D.check("d_state", d_state, torch.uint8, (B, STATE_BYTES), dev)
        D.check("d_sim_out", d_sim_out, torch.uint8, (B, S.OUT_BYTES), dev)
        s = D.torch_stream(stream, dev)
        T, W = int(mpc_ticks), self.wbc_per_mpc
        d_grf, d_qst, d_qit = self.d_grf[:B], self.d_qp_status[:B], self.d_qp_iters[:B]
        d_target, d_cand = self.d_target[:B], self.d_candidates[:B]
        est, plant, ll = self.estimator, self.plant, self.low_level
        d_cout = self.d_contact_out[:B] if plant is not None else None
        d_fb_state, d_fb_out = d_state, d_sim_out  # what the advance and the WBC read
        if est is not None or ll is not None:
            d_gait = E.gait_view(d_robots)
        if est is not None:
            d_sens, d_filt, d_eout = self.d_sensors[:B], self.d_filter[:B], self.d_est_out[:B]
            d_fb_state, d_fb_out = self.d_state_est[:B], self.d_shadow[:B]
        if ll is not None:
            d_ll = self.d_ll_out[:B]
            d_tau = LL.tau_view(d_ll)
        logs = None
        if log:
            K = T * W

            def buf(rows, dtype, *tail):
                return torch.empty((rows, B) + tail, dtype=dtype, device=dev)

            logs = dict(robots=buf(T, torch.uint8, ROBOT_BYTES), u0=buf(T, torch.float64, 12),
                        qp_status=buf(T, torch.int32), qp_iters=buf(T, torch.int32),
                        target=buf(T, torch.uint8, TARGET_BYTES), states=buf(K, torch.uint8, STATE_BYTES),
                        out=buf(K, torch.uint8, S.OUT_BYTES), tau=buf(K, torch.float64, 12),
                        candidates=buf(K, torch.int32, 4))
            if ll is None:
                logs["wbc_status"] = buf(K, torch.int32)
                logs["wbc_iters"] = buf(K, torch.int32, self.pipeline.d_iters.shape[1])
            else:
                logs["ll_out"] = buf(K, torch.uint8, LL.OUT_BYTES)
            if plant is not None:
                logs["contact_out"] = buf(K, torch.uint8, C.OUT_BYTES)
            if est is not None:
                for name, width in (("sensors", E.SENSORS_BYTES), ("state_est", STATE_BYTES), ("filter", E.FILTER_BYTES),
                                    ("est_out", E.OUT_BYTES), ("shadow", S.OUT_BYTES)):
                    logs[name] = buf(K, torch.uint8, width)
        with torch.cuda.stream(s):
            if est is not None:
                if self._est_batch != B:
                    self._init_estimator(d_robots, d_state, d_sim_out, B, s)
                if log:
                    logs["filter0"], logs["state_est0"] = d_filt.clone(), d_fb_state.clone()
                    logs["shadow0"] = d_fb_out.clone()
            for t in range(T):
                advance_device(self.solver, self.rollout_cfg, d_robots, d_fb_state, d_fb_out, s)
                solve_device(self.solver, d_grf, d_qst, d_qit, s)
                targets_device(d_robots, d_grf, self.template, d_target, s)
                if log:
                    logs["robots"][t].copy_(d_robots)
                    logs["u0"][t].copy_(d_grf[:, 0])
                    logs["qp_status"][t].copy_(d_qst)
                    logs["qp_iters"][t].copy_(d_qit)
                    logs["target"][t].copy_(d_target)
                if self.fused_low_level:  # the W controller + plant ticks: one launch, logging its own rows
                    rows = None
                    if log:
                        rows = {k: logs[k][t * W:(t + 1) * W] for k in ("states", "out", "ll_out", "candidates")}
                    LS.run_device(self.model, self.sim_cfg, ll, d_state, d_target, d_sim_out, d_cand, d_ll, W, self.substeps,
                                  d_gait, rows, s)
                    if log:
                        logs["tau"][t * W:(t + 1) * W].copy_(LL.tau_view(rows["ll_out"].view(W * B, LL.OUT_BYTES))
                                                             .view(W, B, 12))
                    continue
                for i in range(W):
                    if ll is not None:  # the controller and, for this plant, its candidates: one launch
                        LL.lowlevel_device(ll, d_fb_state, d_target, d_ll, d_gait, d_sim_out if plant is None else None,
                                           d_cand if plant is None else None, s)
                    else:
                        if plant is None:
                            candidates_device(d_sim_out, d_cand, s)
                        d_x, d_wst = self.pipeline.solve_device(d_fb_state, d_target, s)
                        d_tau = d_x[:, S.TAU_OFFSET:S.TAU_OFFSET + 12]
                    if plant is None:
                        S.step_device(self.model, self.sim_cfg, d_state, d_tau, d_cand, d_state, d_sim_out, self.substeps, s)
                    else:
                        C.step_device(self.model, plant, d_state, d_tau, d_cand, d_state, d_sim_out, d_cout, self.substeps,
                                      s, self.d_plant_work)
                    if est is not None:
                        self._est_tick += 1
                        E.sensors_from_plant_device(self.model, est, d_state, d_sim_out, d_sens, self._est_tick, 0, d_gait, s)
                        E.update_device(self.model, est, d_sens, d_filt, d_fb_state, d_eout, d_sim_out, d_fb_out, s)
                    if log:
                        k = t * W + i
                        logs["states"][k].copy_(d_state)
                        logs["out"][k].copy_(d_sim_out)
                        logs["tau"][k].copy_(d_tau)
                        logs["candidates"][k].copy_(d_cand)
                        if ll is None:
                            logs["wbc_status"][k].copy_(d_wst)
                            logs["wbc_iters"][k].copy_(self.pipeline.d_iters[:B])
                        else:
                            logs["ll_out"][k].copy_(d_ll)
                        if plant is not None:
                            logs["contact_out"][k].copy_(d_cout)
                        if est is not None:
                            logs["sensors"][k].copy_(d_sens)
                            logs["state_est"][k].copy_(d_fb_state)
                            logs["filter"][k].copy_(d_filt)
                            logs["est_out"][k].copy_(d_eout)
                            logs["shadow"][k].copy_(d_fb_out)
        if log:
            flags = S.flags_view(logs["out"])
            logs["cmd"] = logs["robots"][..., :N.COMMAND_BYTES]
            logs["held"], logs["touch"], logs["sim_status"] = flags[..., 0:4], flags[..., 4:8], flags[..., 8]
            if ll is not None:
                logs["ll_flags"] = LL.flags_view(logs["ll_out"])
            if plant is not None:
                logs["mode"] = logs["contact_out"].view(torch.int32)[..., C.MODE_OFFSET // 4:C.MODE_OFFSET // 4 + 4]
            if est is not None:
                logs["est_status"] = logs["est_out"].view(torch.int32)[..., E.OUT_BYTES // 4 - 2]
        return logs
