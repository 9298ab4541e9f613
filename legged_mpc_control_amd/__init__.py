"""MI355X-native batched convex-MPC ground-reaction-force QP solver.

Drop-in for the convex-MPC QP path of zha0ming1e/legged_mpc_control
(src/legged_ctrl ConvexQPSolver / ConvexMpc::grf_update): the QP assembly and
the solve run as one fused HIP kernel for gfx950 behind the C-ABI in
include/lmpc/lmpc.h.
"""
from . import _native
from ._native import (GAIT_CRAWL, GAIT_STAND, GAIT_TROT, GAIT_TROT_WITH_STAND, LmpcCommand, LmpcEstCfg, LmpcEstFilter,
                      LmpcEstOut, LmpcEstSensors, LmpcLegKin, LmpcLowlevelCfg, LmpcLowlevelOut, LmpcOptions, LmpcParams, LmpcRbdModel, LmpcRbdState,
                      LmpcRbdTerms, LmpcRobot, LmpcRolloutCfg, LmpcRolloutLog, LmpcSimCfg, LmpcSimOut, LmpcStackRobot,
                      LmpcWbcTarget, NativeLibraryError)
from .solver import (BatchedConvexQPSolver, ConvexQPSolver, LeggedContactFSM, LeggedCtrl, LeggedFeedback,
                     LeggedParam, LeggedState, foot_jacobian, grf_to_torque, leg_kin_default, solver_options)
from . import est, lowlevel, rbd, rollout, sim, stack, synth
from .rbd import WbcPipeline
from .sim import WbcSim
from .stack import StackLoop

__all__ = [
    "BatchedConvexQPSolver", "ConvexQPSolver", "LeggedContactFSM", "LeggedState", "LeggedFeedback",
    "LeggedCtrl", "LeggedParam", "LmpcParams", "LmpcOptions", "NativeLibraryError", "synth",
    "GAIT_TROT", "GAIT_CRAWL", "GAIT_TROT_WITH_STAND", "GAIT_STAND", "LmpcCommand", "LmpcLegKin",
    "leg_kin_default", "foot_jacobian", "grf_to_torque", "solver_options",
    "rollout", "LmpcRobot", "LmpcRolloutCfg", "LmpcRolloutLog",
    "rbd", "WbcPipeline", "LmpcRbdModel", "LmpcRbdState", "LmpcRbdTerms", "LmpcWbcTarget",
    "sim", "WbcSim", "LmpcSimCfg", "LmpcSimOut",
    "stack", "StackLoop", "LmpcStackRobot",
    "est", "LmpcEstCfg", "LmpcEstSensors", "LmpcEstFilter", "LmpcEstOut",
    "lowlevel", "LmpcLowlevelCfg", "LmpcLowlevelOut",
]
