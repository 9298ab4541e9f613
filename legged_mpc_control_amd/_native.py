"""ctypes binding of the C-ABI in include/lmpc/lmpc.h (liblmpc.so, built in-tree).

The product path has no fallback: if the HIP library is missing or the device
code cannot run, calls raise instead of silently computing on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblmpc.so")

LMPC_OK = 0
LMPC_QP_CONVERGED = 0
LMPC_QP_MAX_ITER = 1
LMPC_QP_NAN = 2
LMPC_MAX_HORIZON = 32
GAIT_TROT, GAIT_CRAWL, GAIT_TROT_WITH_STAND, GAIT_STAND = 0, 1, 2, 3

# every symbol include/lmpc/lmpc.h declares (checked by tests/test_capi.py)
EXPORTED_SYMBOLS = (
    "lmpc_params_go1", "lmpc_params_a1", "lmpc_options_default", "lmpc_record_len",
    "lmpc_abi_version", "lmpc_strerror", "lmpc_create", "lmpc_destroy", "lmpc_set_options",
    "lmpc_set_params", "lmpc_reserve", "lmpc_solve_batch", "lmpc_solve_batch_device", "lmpc_sync",
    "lmpc_predict_contact", "lmpc_current_contact", "lmpc_contact_schedule", "lmpc_pack_record",
    "lmpc_synth_cfg_go1", "lmpc_synth_cfg_a1_standing", "lmpc_synth_fill",
    # ABI 2: terrain extension
    "lmpc_terrain_frame", "lmpc_solve_batch_ex", "lmpc_solve_batch_warm", "lmpc_shift_active_set", "lmpc_solve_batch_device_ex", "lmpc_synth_normals",
    # on-device input generation
    "lmpc_command_to_record", "lmpc_build_records_device", "lmpc_solve_commands_device",
    "lmpc_synth_commands", "lmpc_synth_commands_device", "lmpc_synth_normals_device",
    # GRF -> joint torque
    "lmpc_leg_kin_default", "lmpc_foot_jacobian", "lmpc_grf_to_torque", "lmpc_grf_to_torque_device",
    # ABI 3: dense-path selection
    "lmpc_set_dense_path", "lmpc_get_dense_path", "lmpc_set_riccati_path", "lmpc_get_riccati_path",
    # ABI 7: per-leg gait phases, warm-start workspace
    "lmpc_contact_schedule_legs", "lmpc_reserve_warm",
)
ABI_VERSION = 7
# include/lmpc/lmpc_hoqp.h: batched hierarchical QP (whole-body control)
HOQP_SYMBOLS = (
    "lmpc_hoqp_dims_wbc", "lmpc_hoqp_options_default", "lmpc_hoqp_record_len", "lmpc_hoqp_slack_len",
    "lmpc_hoqp_lds_bytes", "lmpc_hoqp_create", "lmpc_hoqp_destroy", "lmpc_hoqp_set_options", "lmpc_hoqp_solve_batch",
    "lmpc_hoqp_solve_device", "lmpc_hoqp_sync", "lmpc_wbc_tasks", "lmpc_wbc_tasks_device",
    "lmpc_hoqp_solve_batch_z", "lmpc_hoqp_solve_device_z",
    # ABI 2: warm start from the last solve's active sets
    "lmpc_hoqp_abi_version", "lmpc_hoqp_act_len", "lmpc_hoqp_solve_batch_warm", "lmpc_hoqp_solve_device_warm",
)
HOQP_ABI_VERSION = 2
HOQP_MAX_LEVELS = 4
# include/lmpc/lmpc_multi.h: one process, several GPUs (liblmpc_multi.so, RCCL scatter / gather)
MULTI_LIB_PATH = os.path.join(_HERE, "lib", "liblmpc_multi.so")
MULTI_SYMBOLS = (
    "lmpc_multi_abi_version", "lmpc_multi_shard", "lmpc_multi_create", "lmpc_multi_destroy", "lmpc_multi_num_devices",
    "lmpc_multi_set_options", "lmpc_multi_set_dense_path", "lmpc_multi_solve_commands_device",
    "lmpc_multi_solve_synth_device", "lmpc_multi_solve_commands",
)
MULTI_ABI_VERSION = 1
LMPC_ERR_COMM = -6
# include/lmpc/lmpc_rollout.h: the device-resident closed-loop rollout
ROLLOUT_SYMBOLS = (
    "lmpc_rollout_abi_version", "lmpc_robot_size", "lmpc_rollout_cfg_go1", "lmpc_robot_init", "lmpc_robot_plant_step",
    "lmpc_robot_advance", "lmpc_shift_active_set_device", "lmpc_solve_commands_warm_device", "lmpc_rollout_device",
)
ROLLOUT_ABI_VERSION = 1
# include/lmpc/lmpc_rbd.h: floating-base rigid-body dynamics for the WBC (robot state -> lmpc_wbc_input)
RBD_SYMBOLS = (
    "lmpc_rbd_abi_version", "lmpc_rbd_model_size", "lmpc_rbd_state_size", "lmpc_wbc_target_size", "lmpc_rbd_terms_size",
    "lmpc_rbd_model_go1", "lmpc_rbd_model_a1", "lmpc_wbc_target_default", "lmpc_rbd_compute",
    "lmpc_wbc_input_from_state", "lmpc_wbc_inputs_device", "lmpc_rbd_compute_device",
)
RBD_ABI_VERSION = 1
# include/lmpc/lmpc_sim.h: the rigid-body plant (torques and a contact set -> accelerations, forces, next state)
SIM_SYMBOLS = (
    "lmpc_sim_abi_version", "lmpc_sim_cfg_size", "lmpc_sim_out_size", "lmpc_sim_cfg_default", "lmpc_sim_work_bytes",
    "lmpc_rbd_forward_dynamics", "lmpc_sim_step", "lmpc_rbd_forward_dynamics_device", "lmpc_sim_step_device",
)
SIM_ABI_VERSION = 1
# include/lmpc/lmpc_stack.h: the full loop, MPC -> WBC -> plant
STACK_SYMBOLS = (
    "lmpc_stack_abi_version", "lmpc_stack_robot_size", "lmpc_stack_check_rates", "lmpc_stack_robot_init",
    "lmpc_stack_advance", "lmpc_stack_targets", "lmpc_stack_reserve", "lmpc_stack_advance_device", "lmpc_stack_solve_device",
    "lmpc_stack_copy_records_device", "lmpc_stack_targets_device", "lmpc_stack_candidates_device",
)
STACK_ABI_VERSION = 1
# include/lmpc/lmpc_est.h: the sensor model and the base-state Kalman filter
EST_SYMBOLS = (
    "lmpc_est_abi_version", "lmpc_est_sensors_size", "lmpc_est_cfg_size", "lmpc_est_filter_size", "lmpc_est_out_size",
    "lmpc_est_cfg_default", "lmpc_est_sensors_from_plant", "lmpc_est_init", "lmpc_est_report", "lmpc_est_update",
    "lmpc_est_feedback", "lmpc_est_sensors_from_plant_device", "lmpc_est_init_device", "lmpc_est_update_device",
)
EST_ABI_VERSION = 1
# include/lmpc/lmpc_contact.h: the frictional contact model of the plant
CONTACT_SYMBOLS = (
    "lmpc_contact_abi_version", "lmpc_contact_cfg_size", "lmpc_contact_out_size", "lmpc_contact_cfg_default",
    "lmpc_contact_work_bytes", "lmpc_contact_solve", "lmpc_contact_step", "lmpc_contact_solve_device",
    "lmpc_contact_step_device",
)
CONTACT_ABI_VERSION = 1
# include/lmpc/lmpc_lowlevel.h: the reference's joint-PD low-level controller
LOWLEVEL_SYMBOLS = (
    "lmpc_lowlevel_abi_version", "lmpc_lowlevel_cfg_size", "lmpc_lowlevel_out_size", "lmpc_lowlevel_block_robots",
    "lmpc_lowlevel_cfg_go1", "lmpc_lowlevel_cfg_a1", "lmpc_leg_kin_from_model", "lmpc_leg_fk", "lmpc_leg_inv_kin",
    "lmpc_lowlevel", "lmpc_lowlevel_device",
)
LOWLEVEL_ABI_VERSION = 1
LL_IK_NAN, LL_VEL_NAN, LL_TAU_NONFINITE, LL_CLAMPED = 1, 2, 4, 8
# include/lmpc/lmpc_lowsim.h: the low-level ticks of an MPC tick (controller + plant) as one launch
LOWSIM_SYMBOLS = ("lmpc_lowsim_abi_version", "lmpc_lowsim_block_robots", "lmpc_lowsim_run", "lmpc_lowsim_run_device")
LOWSIM_ABI_VERSION = 1


class LmpcParams(ctypes.Structure):
    _fields_ = [
        ("q_weights", ctypes.c_double * 12),
        ("r_weights", ctypes.c_double * 12),
        ("robot_mass", ctypes.c_double),
        ("trunk_inertia", ctypes.c_double * 9),
        ("mu", ctypes.c_double),
        ("f_max", ctypes.c_double),
        ("gravity", ctypes.c_double),
        ("dt", ctypes.c_double),
    ]


class LmpcOptions(ctypes.Structure):
    _fields_ = [
        ("max_iter", ctypes.c_int),
        ("max_rounds", ctypes.c_int),
        ("max_attempts", ctypes.c_int),
        ("tol_mu", ctypes.c_double),
        ("tol_p", ctypes.c_double),
        ("tol_d", ctypes.c_double),
        # ABI 5: the dense paths' caps and the warm-start budget
        ("gi_max_steps", ctypes.c_int),
        ("dense_iter_cap", ctypes.c_int),
        ("dense_polish_iter", ctypes.c_int),
        ("warm_rounds", ctypes.c_int),
        # ABI 7: the certificate's dynamics check (relative to the state scale)
        ("tol_x", ctypes.c_double),
    ]


class LmpcStateIn(ctypes.Structure):
    _fields_ = [
        ("root_euler", ctypes.c_double * 3),
        ("root_pos", ctypes.c_double * 3),
        ("root_ang_vel", ctypes.c_double * 3),
        ("root_lin_vel", ctypes.c_double * 3),
        ("root_rot_mat", ctypes.c_double * 9),
        ("foot_pos_abs", ctypes.c_double * 12),
        ("root_euler_d", ctypes.c_double * 3),
        ("root_pos_d", ctypes.c_double * 3),
        ("root_lin_vel_d_rel", ctypes.c_double * 3),
        ("root_ang_vel_d_rel", ctypes.c_double * 3),
    ]


class LmpcSynthCfg(ctypes.Structure):
    _fields_ = [
        ("gait", ctypes.c_int),
        ("gait_speed", ctypes.c_double),
        ("default_feet", ctypes.c_double * 12),
        ("standing", ctypes.c_int),
    ]


class LmpcCommand(ctypes.Structure):
    _fields_ = [
        ("state", LmpcStateIn),
        ("gait_phase", ctypes.c_double * 4),  # per leg (ABI 7)
        ("gait_speed", ctypes.c_double),
        ("gait", ctypes.c_int32),
        ("plan_contacts", ctypes.c_uint8 * 4),
    ]


COMMAND_BYTES = ctypes.sizeof(LmpcCommand)  # 408


class LmpcRolloutCfg(ctypes.Structure):
    _fields_ = [
        ("default_feet", ctypes.c_double * 12),
        ("swing_clearance", ctypes.c_double),
        ("foot_delta_limit", ctypes.c_double * 2),
        ("ground_z", ctypes.c_double),
    ]


class LmpcRobot(ctypes.Structure):
    """Everything one robot carries between the ticks of a rollout (lmpc_robot)."""
    _fields_ = [
        ("cmd", LmpcCommand),
        ("foot_pos_world", ctypes.c_double * 12),
        ("swing_start_world", ctypes.c_double * 12),
        ("fsm_start", ctypes.c_double * 4),
        ("fsm_index", ctypes.c_int32 * 4),
        ("tick", ctypes.c_int32),
    ]


ROBOT_BYTES = ctypes.sizeof(LmpcRobot)  # 656


class LmpcRolloutLog(ctypes.Structure):
    """Device pointers, each [ticks][batch]... or NULL (lmpc_rollout_log)."""
    _fields_ = [("cmd", ctypes.c_void_p), ("u0", ctypes.c_void_p), ("x", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("iters", ctypes.c_void_p)]


class LmpcLegKin(ctypes.Structure):
    _fields_ = [
        ("rho_fix", (ctypes.c_double * 5) * 4),
        ("rho_opt", (ctypes.c_double * 3) * 4),
    ]


class LmpcHoqpDims(ctypes.Structure):
    _fields_ = [
        ("num_vars", ctypes.c_int32),
        ("num_levels", ctypes.c_int32),
        ("eq_rows", ctypes.c_int32 * HOQP_MAX_LEVELS),
        ("ineq_rows", ctypes.c_int32 * HOQP_MAX_LEVELS),
    ]


class LmpcHoqpOptions(ctypes.Structure):
    _fields_ = [("max_iter", ctypes.c_int32), ("tol_mu", ctypes.c_double), ("tol_res", ctypes.c_double),
                ("crossover", ctypes.c_int32), ("warm_rounds", ctypes.c_int32)]


class LmpcWbcInput(ctypes.Structure):
    _fields_ = [
        ("M", ctypes.c_double * 324), ("nle", ctypes.c_double * 18), ("J", ctypes.c_double * 216),
        ("dJv", ctypes.c_double * 12), ("base_accel", ctypes.c_double * 6), ("swing_acc", ctypes.c_double * 12),
        ("forces_des", ctypes.c_double * 12), ("torque_limits", ctypes.c_double * 3), ("mu", ctypes.c_double),
        ("contact", ctypes.c_int32 * 4),
    ]


class LmpcRbdModel(ctypes.Structure):
    _fields_ = [
        ("mass", ctypes.c_double * 13), ("com", (ctypes.c_double * 3) * 13), ("inertia", (ctypes.c_double * 6) * 13),
        ("joint_origin", (ctypes.c_double * 3) * 12), ("foot", (ctypes.c_double * 3) * 4), ("gravity", ctypes.c_double),
    ]


class LmpcRbdState(ctypes.Structure):
    _fields_ = [
        ("euler", ctypes.c_double * 3), ("pos", ctypes.c_double * 3), ("joint_pos", ctypes.c_double * 12),
        ("omega", ctypes.c_double * 3), ("lin_vel", ctypes.c_double * 3), ("joint_vel", ctypes.c_double * 12),
    ]


class LmpcWbcTarget(ctypes.Structure):
    _fields_ = [
        ("forces_des", ctypes.c_double * 12), ("foot_pos_des", ctypes.c_double * 12),
        ("foot_vel_des", ctypes.c_double * 12), ("torque_limits", ctypes.c_double * 3), ("mu", ctypes.c_double),
        ("swing_kp", ctypes.c_double), ("swing_kd", ctypes.c_double), ("contact", ctypes.c_int32 * 4),
    ]


class LmpcRbdTerms(ctypes.Structure):
    _fields_ = [
        ("M", ctypes.c_double * 324), ("nle", ctypes.c_double * 18), ("J", ctypes.c_double * 216),
        ("dJv", ctypes.c_double * 12), ("foot_pos", ctypes.c_double * 12), ("foot_vel", ctypes.c_double * 12),
        ("com", ctypes.c_double * 3), ("Ab", ctypes.c_double * 36), ("mass", ctypes.c_double),
    ]


class LmpcSimCfg(ctypes.Structure):
    _fields_ = [("dt", ctypes.c_double), ("ground_z", ctypes.c_double), ("unilateral", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class LmpcSimOut(ctypes.Structure):
    _fields_ = [
        ("qdd", ctypes.c_double * 18), ("force", ctypes.c_double * 12), ("foot_pos", ctypes.c_double * 12),
        ("foot_vel", ctypes.c_double * 12), ("held", ctypes.c_int32 * 4), ("touch", ctypes.c_int32 * 4),
        ("status", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LmpcContactCfg(ctypes.Structure):
    _fields_ = [
        ("dt", ctypes.c_double), ("ground_z", ctypes.c_double), ("mu", ctypes.c_double),
        ("recover_speed", ctypes.c_double), ("force_threshold", ctypes.c_double), ("tol_p", ctypes.c_double),
        ("tol_d", ctypes.c_double), ("use_gap", ctypes.c_int32), ("touch_rule", ctypes.c_int32),
        ("max_sweeps", ctypes.c_int32), ("max_polish", ctypes.c_int32),
    ]


class LmpcContactOut(ctypes.Structure):
    _fields_ = [
        ("w", ctypes.c_double * 12), ("gap", ctypes.c_double * 4), ("res_primal", ctypes.c_double),
        ("res_dual", ctypes.c_double), ("mode", ctypes.c_int32 * 4), ("sweeps", ctypes.c_int32),
        ("polish", ctypes.c_int32), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LmpcStackRobot(ctypes.Structure):
    """Everything one robot's MPC carries between the ticks of the full loop (lmpc_stack_robot)."""
    _fields_ = [
        ("rb", LmpcRobot),
        ("fsm_pos_target", ctypes.c_double * 12),
        ("fsm_vel_target", ctypes.c_double * 12),
        ("swing_end_world", ctypes.c_double * 12),
        ("not_first_call", ctypes.c_int32 * 4),
    ]


STACK_ROBOT_BYTES = ctypes.sizeof(LmpcStackRobot)  # 960


class LmpcEstSensors(ctypes.Structure):
    _fields_ = [
        ("imu_acc", ctypes.c_double * 3), ("imu_ang_vel", ctypes.c_double * 3), ("euler", ctypes.c_double * 3),
        ("joint_pos", ctypes.c_double * 12), ("joint_vel", ctypes.c_double * 12), ("contact", ctypes.c_double * 4),
    ]


class LmpcEstCfg(ctypes.Structure):
    _fields_ = [
        ("dt", ctypes.c_double), ("noise_pimu", ctypes.c_double), ("noise_vimu", ctypes.c_double),
        ("noise_pfoot", ctypes.c_double), ("noise_pimu_rel_foot", ctypes.c_double),
        ("noise_vimu_rel_foot", ctypes.c_double), ("noise_zfoot", ctypes.c_double), ("gravity", ctypes.c_double),
        ("drift_threshold", ctypes.c_double), ("drift_divisor", ctypes.c_double), ("init_P", ctypes.c_double),
        ("sigma_acc", ctypes.c_double), ("sigma_gyro", ctypes.c_double), ("sigma_euler", ctypes.c_double),
        ("sigma_joint_pos", ctypes.c_double), ("sigma_joint_vel", ctypes.c_double), ("seed", ctypes.c_uint64),
        ("assume_flat_ground", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LmpcEstFilter(ctypes.Structure):
    _fields_ = [("x", ctypes.c_double * 18), ("P", ctypes.c_double * 324), ("inited", ctypes.c_int32),
                ("ticks", ctypes.c_int32)]


class LmpcEstOut(ctypes.Structure):
    _fields_ = [
        ("foot_pos_rel", ctypes.c_double * 12), ("foot_pos_world", ctypes.c_double * 12),
        ("foot_vel_world", ctypes.c_double * 12), ("estimated_contacts", ctypes.c_int32 * 4),
        ("status", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LmpcLowlevelCfg(ctypes.Structure):
    _fields_ = [
        ("kin", LmpcLegKin), ("kp", (ctypes.c_double * 3) * 4), ("kd", (ctypes.c_double * 3) * 4),
        ("tau_limit", ctypes.c_double * 3),
    ]


class LmpcLowlevelOut(ctypes.Structure):
    _fields_ = [
        ("tau", ctypes.c_double * 12), ("joint_tau_tgt", ctypes.c_double * 12), ("joint_ang_tgt", ctypes.c_double * 12),
        ("joint_vel_tgt", ctypes.c_double * 12), ("flags", ctypes.c_int32 * 4),
    ]


class LmpcLowsimLog(ctypes.Structure):
    """lmpc_lowsim_log: host pointers for lmpc_lowsim_run, device pointers for lmpc_lowsim_run_device; each may be None."""
    _fields_ = [("states", ctypes.c_void_p), ("outs", ctypes.c_void_p), ("ll_outs", ctypes.c_void_p),
                ("candidates", ctypes.c_void_p)]


class NativeLibraryError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None


def lib():
    """Load liblmpc.so (raises NativeLibraryError if it was not built)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = os.environ.get("LMPC_LIB") or LIB_PATH  # LMPC_LIB: diagnostic builds (tools/) only
        if not os.path.exists(path):
            raise NativeLibraryError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(path)
        vp, dp, i32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        pp = ctypes.POINTER(LmpcParams)
        L.lmpc_params_go1.argtypes = [pp]
        L.lmpc_params_a1.argtypes = [pp]
        L.lmpc_options_default.argtypes = [ctypes.POINTER(LmpcOptions)]
        L.lmpc_record_len.argtypes = [ctypes.c_int]
        L.lmpc_record_len.restype = ctypes.c_int
        L.lmpc_abi_version.restype = ctypes.c_int
        L.lmpc_strerror.argtypes = [ctypes.c_int]
        L.lmpc_strerror.restype = ctypes.c_char_p
        L.lmpc_create.argtypes = [pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.lmpc_create.restype = ctypes.c_int
        L.lmpc_destroy.argtypes = [vp]
        L.lmpc_destroy.restype = None
        L.lmpc_set_options.argtypes = [vp, ctypes.POINTER(LmpcOptions)]
        L.lmpc_set_options.restype = ctypes.c_int
        L.lmpc_set_params.argtypes = [vp, pp]
        L.lmpc_set_params.restype = ctypes.c_int
        L.lmpc_set_dense_path.argtypes = [vp, ctypes.c_int]
        L.lmpc_set_dense_path.restype = ctypes.c_int
        L.lmpc_get_dense_path.argtypes = [vp]
        L.lmpc_get_dense_path.restype = ctypes.c_int
        L.lmpc_set_riccati_path.argtypes = [vp, ctypes.c_int]
        L.lmpc_set_riccati_path.restype = ctypes.c_int
        L.lmpc_get_riccati_path.argtypes = [vp]
        L.lmpc_get_riccati_path.restype = ctypes.c_int
        L.lmpc_reserve.argtypes = [vp, ctypes.c_int]
        L.lmpc_reserve.restype = ctypes.c_int
        if hasattr(L, "lmpc_reserve_warm"):  # ABI 7
            L.lmpc_reserve_warm.argtypes = [vp, ctypes.c_int]
            L.lmpc_reserve_warm.restype = ctypes.c_int
        L.lmpc_solve_batch.argtypes = [vp, dp, u8p, ctypes.c_int, dp, i32p, i32p]
        L.lmpc_solve_batch.restype = ctypes.c_int
        L.lmpc_solve_batch_device.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        L.lmpc_solve_batch_device.restype = ctypes.c_int
        L.lmpc_sync.argtypes = [vp]
        L.lmpc_sync.restype = ctypes.c_int
        L.lmpc_predict_contact.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        L.lmpc_predict_contact.restype = ctypes.c_int
        L.lmpc_current_contact.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
        L.lmpc_current_contact.restype = ctypes.c_int
        L.lmpc_contact_schedule.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, u8p, u8p]
        L.lmpc_contact_schedule.restype = ctypes.c_int
        if hasattr(L, "lmpc_contact_schedule_legs"):  # ABI 7 (absent from a one-ABI-behind diagnostic build)
            L.lmpc_contact_schedule_legs.argtypes = [ctypes.c_int, dp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                     u8p, u8p]
            L.lmpc_contact_schedule_legs.restype = ctypes.c_int
        L.lmpc_pack_record.argtypes = [pp, ctypes.c_int, ctypes.POINTER(LmpcStateIn), dp, dp]
        L.lmpc_pack_record.restype = ctypes.c_int
        L.lmpc_synth_cfg_go1.argtypes = [ctypes.POINTER(LmpcSynthCfg)]
        L.lmpc_synth_cfg_a1_standing.argtypes = [ctypes.POINTER(LmpcSynthCfg)]
        L.lmpc_synth_fill.argtypes = [pp, ctypes.POINTER(LmpcSynthCfg), ctypes.c_int, ctypes.c_uint64,
                                      ctypes.c_int64, ctypes.c_int, dp, u8p]
        L.lmpc_synth_fill.restype = ctypes.c_int
        L.lmpc_terrain_frame.argtypes = [dp, dp]
        L.lmpc_terrain_frame.restype = None
        L.lmpc_solve_batch_ex.argtypes = [vp, dp, u8p, dp, ctypes.c_int, dp, i32p, i32p]
        L.lmpc_solve_batch_ex.restype = ctypes.c_int
        L.lmpc_solve_batch_warm.argtypes = [vp, dp, u8p, dp, ctypes.c_int, u8p, u8p, dp, i32p, i32p]
        L.lmpc_solve_batch_warm.restype = ctypes.c_int
        L.lmpc_shift_active_set.argtypes = [u8p, ctypes.c_int, ctypes.c_int, u8p]
        L.lmpc_shift_active_set.restype = None
        L.lmpc_solve_batch_device_ex.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        L.lmpc_solve_batch_device_ex.restype = ctypes.c_int
        L.lmpc_synth_normals.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, dp]
        L.lmpc_synth_normals.restype = ctypes.c_int
        cp = ctypes.POINTER(LmpcCommand)
        L.lmpc_command_to_record.argtypes = [pp, ctypes.c_int, cp, dp, u8p]
        L.lmpc_command_to_record.restype = ctypes.c_int
        L.lmpc_build_records_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        L.lmpc_build_records_device.restype = ctypes.c_int
        L.lmpc_solve_commands_device.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        L.lmpc_solve_commands_device.restype = ctypes.c_int
        L.lmpc_synth_commands.argtypes = [ctypes.POINTER(LmpcSynthCfg), ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, cp]
        L.lmpc_synth_commands.restype = ctypes.c_int
        L.lmpc_synth_commands_device.argtypes = [vp, ctypes.POINTER(LmpcSynthCfg), ctypes.c_uint64, ctypes.c_int64,
                                                 ctypes.c_int, vp, vp]
        L.lmpc_synth_commands_device.restype = ctypes.c_int
        L.lmpc_synth_normals_device.argtypes = [vp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, vp, vp]
        L.lmpc_synth_normals_device.restype = ctypes.c_int
        kp = ctypes.POINTER(LmpcLegKin)
        L.lmpc_leg_kin_default.argtypes = [kp]
        L.lmpc_leg_kin_default.restype = None
        L.lmpc_foot_jacobian.argtypes = [kp, ctypes.c_int, dp, dp]
        L.lmpc_foot_jacobian.restype = None
        L.lmpc_grf_to_torque.argtypes = [kp, dp, dp, dp, dp]
        L.lmpc_grf_to_torque.restype = ctypes.c_int
        L.lmpc_grf_to_torque_device.argtypes = [vp, kp, vp, vp, vp, ctypes.c_int, vp, vp]
        L.lmpc_grf_to_torque_device.restype = ctypes.c_int
        hdp, hop = ctypes.POINTER(LmpcHoqpDims), ctypes.POINTER(LmpcHoqpOptions)
        L.lmpc_hoqp_dims_wbc.argtypes = [hdp]
        L.lmpc_hoqp_dims_wbc.restype = None
        L.lmpc_hoqp_options_default.argtypes = [hop]
        L.lmpc_hoqp_options_default.restype = None
        L.lmpc_hoqp_record_len.argtypes = [hdp]
        L.lmpc_hoqp_record_len.restype = ctypes.c_int64
        L.lmpc_hoqp_lds_bytes.argtypes = [hdp]
        L.lmpc_hoqp_lds_bytes.restype = ctypes.c_int64
        L.lmpc_hoqp_slack_len.argtypes = [hdp]
        L.lmpc_hoqp_slack_len.restype = ctypes.c_int
        L.lmpc_hoqp_create.argtypes = [hdp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.lmpc_hoqp_create.restype = ctypes.c_int
        L.lmpc_hoqp_destroy.argtypes = [vp]
        L.lmpc_hoqp_destroy.restype = None
        L.lmpc_hoqp_set_options.argtypes = [vp, hop]
        L.lmpc_hoqp_set_options.restype = ctypes.c_int
        L.lmpc_hoqp_solve_batch.argtypes = [vp, dp, ctypes.c_int, dp, dp, i32p, i32p]
        L.lmpc_hoqp_solve_batch.restype = ctypes.c_int
        L.lmpc_hoqp_solve_device.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
        L.lmpc_hoqp_solve_device.restype = ctypes.c_int
        L.lmpc_hoqp_solve_batch_z.argtypes = [vp, dp, ctypes.c_int, dp, dp, i32p, i32p, dp, i32p]
        L.lmpc_hoqp_solve_batch_z.restype = ctypes.c_int
        L.lmpc_hoqp_solve_device_z.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.lmpc_hoqp_solve_device_z.restype = ctypes.c_int
        L.lmpc_hoqp_sync.argtypes = [vp]
        L.lmpc_hoqp_sync.restype = ctypes.c_int
        L.lmpc_hoqp_abi_version.restype = ctypes.c_int
        L.lmpc_hoqp_act_len.argtypes = [hdp]
        L.lmpc_hoqp_act_len.restype = ctypes.c_int64
        L.lmpc_hoqp_solve_batch_warm.argtypes = [vp, dp, ctypes.c_int, dp, dp, i32p, i32p, ctypes.POINTER(ctypes.c_uint64)]
        L.lmpc_hoqp_solve_batch_warm.restype = ctypes.c_int
        L.lmpc_hoqp_solve_device_warm.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        L.lmpc_hoqp_solve_device_warm.restype = ctypes.c_int
        L.lmpc_wbc_tasks.argtypes = [ctypes.POINTER(LmpcWbcInput), dp]
        L.lmpc_wbc_tasks.restype = ctypes.c_int
        L.lmpc_wbc_tasks_device.argtypes = [vp, ctypes.c_int, vp, vp]
        L.lmpc_wbc_tasks_device.restype = ctypes.c_int
        rcp, rbp = ctypes.POINTER(LmpcRolloutCfg), ctypes.POINTER(LmpcRobot)
        L.lmpc_rollout_abi_version.restype = ctypes.c_int
        L.lmpc_robot_size.restype = ctypes.c_int
        L.lmpc_rollout_cfg_go1.argtypes = [rcp]
        L.lmpc_rollout_cfg_go1.restype = None
        L.lmpc_robot_init.argtypes = [rcp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double, rbp]
        L.lmpc_robot_init.restype = ctypes.c_int
        L.lmpc_robot_plant_step.argtypes = [pp, rbp, dp]
        L.lmpc_robot_plant_step.restype = ctypes.c_int
        L.lmpc_robot_advance.argtypes = [pp, rcp, rbp, dp, dp]
        L.lmpc_robot_advance.restype = ctypes.c_int
        L.lmpc_shift_active_set_device.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        L.lmpc_shift_active_set_device.restype = ctypes.c_int
        L.lmpc_solve_commands_warm_device.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        L.lmpc_solve_commands_warm_device.restype = ctypes.c_int
        L.lmpc_rollout_device.argtypes = [vp, rcp, vp, vp, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(LmpcRolloutLog), vp]
        L.lmpc_rollout_device.restype = ctypes.c_int
        mp, sp, tp = ctypes.POINTER(LmpcRbdModel), ctypes.POINTER(LmpcRbdState), ctypes.POINTER(LmpcWbcTarget)
        for name in ("lmpc_rbd_abi_version", "lmpc_rbd_model_size", "lmpc_rbd_state_size", "lmpc_wbc_target_size",
                     "lmpc_rbd_terms_size"):
            getattr(L, name).restype = ctypes.c_int
        L.lmpc_rbd_model_go1.argtypes = [mp]
        L.lmpc_rbd_model_go1.restype = None
        L.lmpc_rbd_model_a1.argtypes = [mp]
        L.lmpc_rbd_model_a1.restype = None
        L.lmpc_wbc_target_default.argtypes = [tp]
        L.lmpc_wbc_target_default.restype = None
        L.lmpc_rbd_compute.argtypes = [mp, sp, ctypes.POINTER(LmpcRbdTerms)]
        L.lmpc_rbd_compute.restype = ctypes.c_int
        L.lmpc_wbc_input_from_state.argtypes = [mp, sp, tp, ctypes.POINTER(LmpcWbcInput)]
        L.lmpc_wbc_input_from_state.restype = ctypes.c_int
        L.lmpc_wbc_inputs_device.argtypes = [mp, vp, vp, ctypes.c_int, vp, vp]
        L.lmpc_wbc_inputs_device.restype = ctypes.c_int
        L.lmpc_rbd_compute_device.argtypes = [mp, vp, ctypes.c_int, vp, vp]
        L.lmpc_rbd_compute_device.restype = ctypes.c_int
        sizes = (L.lmpc_rbd_model_size(), L.lmpc_rbd_state_size(), L.lmpc_wbc_target_size(), L.lmpc_rbd_terms_size())
        mirrors = tuple(ctypes.sizeof(c) for c in (LmpcRbdModel, LmpcRbdState, LmpcWbcTarget, LmpcRbdTerms))
        if L.lmpc_rbd_abi_version() != RBD_ABI_VERSION or sizes != mirrors:
            raise NativeLibraryError(f"{path}: lmpc_rbd.h ABI {L.lmpc_rbd_abi_version()} with struct sizes {sizes}, "
                                     f"this binding is ABI {RBD_ABI_VERSION} with {mirrors}")
        cfp, sop = ctypes.POINTER(LmpcSimCfg), ctypes.POINTER(LmpcSimOut)
        for name in ("lmpc_sim_abi_version", "lmpc_sim_cfg_size", "lmpc_sim_out_size"):
            getattr(L, name).restype = ctypes.c_int
        L.lmpc_sim_cfg_default.argtypes = [cfp]
        L.lmpc_sim_cfg_default.restype = None
        L.lmpc_sim_work_bytes.argtypes = [ctypes.c_int]
        L.lmpc_sim_work_bytes.restype = ctypes.c_size_t
        L.lmpc_rbd_forward_dynamics.argtypes = [mp, sp, dp, i32p, ctypes.c_int, sop]
        L.lmpc_rbd_forward_dynamics.restype = ctypes.c_int
        L.lmpc_sim_step.argtypes = [mp, cfp, sp, dp, i32p, sp, sop]
        L.lmpc_sim_step.restype = ctypes.c_int
        L.lmpc_rbd_forward_dynamics_device.argtypes = [mp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int,
                                                       ctypes.c_int, vp, vp]
        L.lmpc_rbd_forward_dynamics_device.restype = ctypes.c_int
        L.lmpc_sim_step_device.argtypes = [mp, cfp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int,
                                           ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]
        L.lmpc_sim_step_device.restype = ctypes.c_int
        sim_sizes = (L.lmpc_sim_cfg_size(), L.lmpc_sim_out_size())
        sim_mirrors = (ctypes.sizeof(LmpcSimCfg), ctypes.sizeof(LmpcSimOut))
        if L.lmpc_sim_abi_version() != SIM_ABI_VERSION or sim_sizes != sim_mirrors:
            raise NativeLibraryError(f"{path}: lmpc_sim.h ABI {L.lmpc_sim_abi_version()} with struct sizes {sim_sizes}, "
                                     f"this binding is ABI {SIM_ABI_VERSION} with {sim_mirrors}")
        srp = ctypes.POINTER(LmpcStackRobot)
        L.lmpc_stack_abi_version.restype = ctypes.c_int
        L.lmpc_stack_robot_size.restype = ctypes.c_int
        L.lmpc_stack_check_rates.argtypes = [pp, cfp, ctypes.c_int, ctypes.c_int]
        L.lmpc_stack_check_rates.restype = ctypes.c_int
        L.lmpc_stack_robot_init.argtypes = [rcp, mp, sp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                            ctypes.c_double, srp, sop]
        L.lmpc_stack_robot_init.restype = ctypes.c_int
        L.lmpc_stack_advance.argtypes = [pp, rcp, srp, sp, sop, dp]
        L.lmpc_stack_advance.restype = ctypes.c_int
        L.lmpc_stack_targets.argtypes = [srp, dp, tp, tp]
        L.lmpc_stack_targets.restype = ctypes.c_int
        L.lmpc_stack_reserve.argtypes = [vp, ctypes.c_int]
        L.lmpc_stack_reserve.restype = ctypes.c_int
        L.lmpc_stack_advance_device.argtypes = [vp, rcp, vp, vp, vp, ctypes.c_int, vp]
        L.lmpc_stack_advance_device.restype = ctypes.c_int
        L.lmpc_stack_solve_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp]
        L.lmpc_stack_solve_device.restype = ctypes.c_int
        L.lmpc_stack_copy_records_device.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        L.lmpc_stack_copy_records_device.restype = ctypes.c_int
        L.lmpc_stack_targets_device.argtypes = [vp, vp, ctypes.c_int64, tp, ctypes.c_int, vp, vp]
        L.lmpc_stack_targets_device.restype = ctypes.c_int
        L.lmpc_stack_candidates_device.argtypes = [vp, ctypes.c_int, vp, vp]
        L.lmpc_stack_candidates_device.restype = ctypes.c_int
        if L.lmpc_stack_abi_version() != STACK_ABI_VERSION or L.lmpc_stack_robot_size() != STACK_ROBOT_BYTES:
            raise NativeLibraryError(f"{path}: lmpc_stack.h ABI {L.lmpc_stack_abi_version()} / lmpc_stack_robot of "
                                     f"{L.lmpc_stack_robot_size()} B, this binding is ABI {STACK_ABI_VERSION} / "
                                     f"{STACK_ROBOT_BYTES} B")
        esp, ecp = ctypes.POINTER(LmpcEstSensors), ctypes.POINTER(LmpcEstCfg)
        efp, eop = ctypes.POINTER(LmpcEstFilter), ctypes.POINTER(LmpcEstOut)
        for name in ("lmpc_est_abi_version", "lmpc_est_sensors_size", "lmpc_est_cfg_size", "lmpc_est_filter_size",
                     "lmpc_est_out_size"):
            getattr(L, name).restype = ctypes.c_int
        L.lmpc_est_cfg_default.argtypes = [ecp]
        L.lmpc_est_cfg_default.restype = None
        L.lmpc_est_sensors_from_plant.argtypes = [mp, ecp, sp, sop, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int, esp]
        L.lmpc_est_sensors_from_plant.restype = ctypes.c_int
        L.lmpc_est_init.argtypes = [mp, ecp, esp, dp, efp]
        L.lmpc_est_init.restype = ctypes.c_int
        L.lmpc_est_report.argtypes = [mp, esp, efp, sp, eop]
        L.lmpc_est_report.restype = ctypes.c_int
        L.lmpc_est_update.argtypes = [mp, ecp, esp, efp, sp, eop]
        L.lmpc_est_update.restype = ctypes.c_int
        L.lmpc_est_feedback.argtypes = [sop, eop, sop]
        L.lmpc_est_feedback.restype = ctypes.c_int
        L.lmpc_est_sensors_from_plant_device.argtypes = [mp, ecp, vp, vp, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32,
                                                         vp, ctypes.c_int64, vp, vp]
        L.lmpc_est_sensors_from_plant_device.restype = ctypes.c_int
        L.lmpc_est_init_device.argtypes = [mp, ecp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        L.lmpc_est_init_device.restype = ctypes.c_int
        L.lmpc_est_update_device.argtypes = [mp, ecp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        L.lmpc_est_update_device.restype = ctypes.c_int
        est_sizes = (L.lmpc_est_sensors_size(), L.lmpc_est_cfg_size(), L.lmpc_est_filter_size(), L.lmpc_est_out_size())
        est_mirrors = tuple(ctypes.sizeof(c) for c in (LmpcEstSensors, LmpcEstCfg, LmpcEstFilter, LmpcEstOut))
        if L.lmpc_est_abi_version() != EST_ABI_VERSION or est_sizes != est_mirrors:
            raise NativeLibraryError(f"{path}: lmpc_est.h ABI {L.lmpc_est_abi_version()} with struct sizes {est_sizes}, "
                                     f"this binding is ABI {EST_ABI_VERSION} with {est_mirrors}")
        ccp, cop = ctypes.POINTER(LmpcContactCfg), ctypes.POINTER(LmpcContactOut)
        for name in ("lmpc_contact_abi_version", "lmpc_contact_cfg_size", "lmpc_contact_out_size"):
            getattr(L, name).restype = ctypes.c_int
        L.lmpc_contact_cfg_default.argtypes = [ccp]
        L.lmpc_contact_cfg_default.restype = None
        L.lmpc_contact_work_bytes.argtypes = [ctypes.c_int]
        L.lmpc_contact_work_bytes.restype = ctypes.c_size_t
        L.lmpc_contact_solve.argtypes = [ccp, dp, dp, i32p, dp, cop]
        L.lmpc_contact_solve.restype = ctypes.c_int
        L.lmpc_contact_step.argtypes = [mp, ccp, sp, dp, i32p, sp, sop, cop]
        L.lmpc_contact_step.restype = ctypes.c_int
        L.lmpc_contact_solve_device.argtypes = [ccp, vp, vp, vp, ctypes.c_int, vp, vp, vp]
        L.lmpc_contact_solve_device.restype = ctypes.c_int
        L.lmpc_contact_step_device.argtypes = [mp, ccp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.lmpc_contact_step_device.restype = ctypes.c_int
        contact_sizes = (L.lmpc_contact_cfg_size(), L.lmpc_contact_out_size())
        contact_mirrors = (ctypes.sizeof(LmpcContactCfg), ctypes.sizeof(LmpcContactOut))
        if L.lmpc_contact_abi_version() != CONTACT_ABI_VERSION or contact_sizes != contact_mirrors:
            raise NativeLibraryError(f"{path}: lmpc_contact.h ABI {L.lmpc_contact_abi_version()} with struct sizes "
                                     f"{contact_sizes}, this binding is ABI {CONTACT_ABI_VERSION} with {contact_mirrors}")
        lcp, lop = ctypes.POINTER(LmpcLowlevelCfg), ctypes.POINTER(LmpcLowlevelOut)
        for name in ("lmpc_lowlevel_abi_version", "lmpc_lowlevel_cfg_size", "lmpc_lowlevel_out_size",
                     "lmpc_lowlevel_block_robots"):
            getattr(L, name).restype = ctypes.c_int
        L.lmpc_lowlevel_cfg_go1.argtypes = [lcp]
        L.lmpc_lowlevel_cfg_go1.restype = None
        L.lmpc_lowlevel_cfg_a1.argtypes = [lcp]
        L.lmpc_lowlevel_cfg_a1.restype = None
        L.lmpc_leg_kin_from_model.argtypes = [mp, kp]
        L.lmpc_leg_kin_from_model.restype = ctypes.c_int
        L.lmpc_leg_fk.argtypes = [kp, ctypes.c_int, dp, dp]
        L.lmpc_leg_fk.restype = ctypes.c_int
        L.lmpc_leg_inv_kin.argtypes = [kp, ctypes.c_int, dp, dp, dp]
        L.lmpc_leg_inv_kin.restype = ctypes.c_int
        L.lmpc_lowlevel.argtypes = [lcp, sp, tp, i32p, lop]
        L.lmpc_lowlevel.restype = ctypes.c_int
        L.lmpc_lowlevel_device.argtypes = [lcp, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp, vp]
        L.lmpc_lowlevel_device.restype = ctypes.c_int
        ll_sizes = (L.lmpc_lowlevel_cfg_size(), L.lmpc_lowlevel_out_size())
        ll_mirrors = (ctypes.sizeof(LmpcLowlevelCfg), ctypes.sizeof(LmpcLowlevelOut))
        if L.lmpc_lowlevel_abi_version() != LOWLEVEL_ABI_VERSION or ll_sizes != ll_mirrors:
            raise NativeLibraryError(f"{path}: lmpc_lowlevel.h ABI {L.lmpc_lowlevel_abi_version()} with struct sizes "
                                     f"{ll_sizes}, this binding is ABI {LOWLEVEL_ABI_VERSION} with {ll_mirrors}")
        lgp = ctypes.POINTER(LmpcLowsimLog)
        L.lmpc_lowsim_abi_version.restype = ctypes.c_int
        L.lmpc_lowsim_block_robots.restype = ctypes.c_int
        L.lmpc_lowsim_run.argtypes = [mp, ctypes.POINTER(LmpcSimCfg), lcp, sp, tp, i32p, ctypes.POINTER(LmpcSimOut), i32p, lop,
                                      ctypes.c_int, ctypes.c_int, lgp]
        L.lmpc_lowsim_run.restype = ctypes.c_int
        L.lmpc_lowsim_run_device.argtypes = [mp, ctypes.POINTER(LmpcSimCfg), lcp, vp, vp, vp, ctypes.c_int64, vp, vp, vp,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, lgp, vp]
        L.lmpc_lowsim_run_device.restype = ctypes.c_int
        if L.lmpc_lowsim_abi_version() != LOWSIM_ABI_VERSION:
            raise NativeLibraryError(f"{path}: lmpc_lowsim.h ABI {L.lmpc_lowsim_abi_version()}, this binding is ABI "
                                     f"{LOWSIM_ABI_VERSION}")
        if L.lmpc_rollout_abi_version() != ROLLOUT_ABI_VERSION or L.lmpc_robot_size() != ROBOT_BYTES:
            raise NativeLibraryError(f"{path}: lmpc_rollout.h ABI {L.lmpc_rollout_abi_version()} / lmpc_robot of "
                                     f"{L.lmpc_robot_size()} B, this binding is ABI {ROLLOUT_ABI_VERSION} / {ROBOT_BYTES} B")
        # exactly this ABI, diagnostic builds (LMPC_LIB) included: the command and options structs above are ABI-7
        # layouts, and an older library would read their fields at the wrong offsets without an error
        if L.lmpc_hoqp_abi_version() != HOQP_ABI_VERSION:
            raise NativeLibraryError(f"{path}: lmpc_hoqp.h ABI {L.lmpc_hoqp_abi_version()}, this binding is ABI "
                                     f"{HOQP_ABI_VERSION}")
        if L.lmpc_abi_version() != ABI_VERSION:
            raise NativeLibraryError(f"{path}: ABI version {L.lmpc_abi_version()}, this binding is ABI {ABI_VERSION}")
        _lib = L
        return L


_mlib = None


def multi_lib():
    """Load liblmpc_multi.so (raises NativeLibraryError if it was not built)."""
    global _mlib
    lib()  # liblmpc.so first: the multi-device library links it
    with _lock:
        if _mlib is not None:
            return _mlib
        if not os.path.exists(MULTI_LIB_PATH):
            raise NativeLibraryError(f"{MULTI_LIB_PATH} not found: build it with __graft_entry__.build()")
        M = ctypes.CDLL(MULTI_LIB_PATH)
        vp, i32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)
        pp = ctypes.POINTER(LmpcParams)
        M.lmpc_multi_abi_version.restype = ctypes.c_int
        M.lmpc_multi_shard.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, i32p]
        M.lmpc_multi_shard.restype = None
        M.lmpc_multi_create.argtypes = [pp, ctypes.c_int, i32p, ctypes.c_int, ctypes.POINTER(vp)]
        M.lmpc_multi_create.restype = ctypes.c_int
        M.lmpc_multi_destroy.argtypes = [vp]
        M.lmpc_multi_destroy.restype = None
        M.lmpc_multi_num_devices.argtypes = [vp]
        M.lmpc_multi_num_devices.restype = ctypes.c_int
        M.lmpc_multi_set_options.argtypes = [vp, ctypes.POINTER(LmpcOptions)]
        M.lmpc_multi_set_options.restype = ctypes.c_int
        M.lmpc_multi_set_dense_path.argtypes = [vp, ctypes.c_int]
        M.lmpc_multi_set_dense_path.restype = ctypes.c_int
        M.lmpc_multi_solve_commands_device.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        M.lmpc_multi_solve_commands_device.restype = ctypes.c_int
        M.lmpc_multi_solve_synth_device.argtypes = [vp, ctypes.POINTER(LmpcSynthCfg), ctypes.c_uint64, ctypes.c_int64,
                                                    ctypes.c_int, ctypes.c_double, vp, vp, vp]
        M.lmpc_multi_solve_synth_device.restype = ctypes.c_int
        M.lmpc_multi_solve_commands.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp]
        M.lmpc_multi_solve_commands.restype = ctypes.c_int
        if M.lmpc_multi_abi_version() != MULTI_ABI_VERSION:
            raise NativeLibraryError("liblmpc_multi.so ABI version mismatch")
        _mlib = M
        return M


def check(rc: int, what: str = "lmpc") -> None:
    if rc != LMPC_OK:
        msg = "RCCL communication failed" if rc == LMPC_ERR_COMM else lib().lmpc_strerror(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} ({rc})")
