"""ctypes binding of the C-ABI in include/lmpc/*.h (liblmpc.so and liblmpc_multi.so, built in-tree).

The product path has no fallback: if the HIP library is missing or the device
code cannot run, calls raise instead of silently computing on the CPU.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblmpc.so")
MULTI_LIB_PATH = os.path.join(_HERE, "lib", "liblmpc_multi.so")  # one process, several GPUs (RCCL scatter / gather)

LMPC_OK = 0
LMPC_ERR_COMM = -6
LMPC_QP_CONVERGED = 0
LMPC_QP_MAX_ITER = 1
LMPC_QP_NAN = 2
LMPC_MAX_HORIZON = 32
GAIT_TROT, GAIT_CRAWL, GAIT_TROT_WITH_STAND, GAIT_STAND = 0, 1, 2, 3
HOQP_MAX_LEVELS = 4
LL_IK_NAN, LL_VEL_NAN, LL_TAU_NONFINITE, LL_CLAMPED = 1, 2, 4, 8
# The ABI of each public header this binding is written for.  Exactly these, diagnostic builds (LMPC_LIB) included: the
# structures below are these ABIs' layouts, and an older library would read their fields at the wrong offsets without an
# error.
ABI_VERSION = 7           # lmpc.h
HOQP_ABI_VERSION = 2      # lmpc_hoqp.h: batched hierarchical QP (whole-body control)
ROLLOUT_ABI_VERSION = 1   # lmpc_rollout.h: the device-resident closed-loop rollout
RBD_ABI_VERSION = 1       # lmpc_rbd.h: floating-base rigid-body dynamics for the WBC (robot state -> lmpc_wbc_input)
SIM_ABI_VERSION = 1       # lmpc_sim.h: the rigid-body plant (torques and a contact set -> accelerations, forces, state)
STACK_ABI_VERSION = 1     # lmpc_stack.h: the full loop, MPC -> WBC -> plant
EST_ABI_VERSION = 1       # lmpc_est.h: the sensor model and the base-state Kalman filter
CONTACT_ABI_VERSION = 1   # lmpc_contact.h: the frictional contact model of the plant
LOWLEVEL_ABI_VERSION = 1  # lmpc_lowlevel.h: the reference's joint-PD low-level controller
LOWSIM_ABI_VERSION = 1    # lmpc_lowsim.h: the low-level ticks of an MPC tick (controller + plant) as one launch
MULTI_ABI_VERSION = 1     # lmpc_multi.h (liblmpc_multi.so)


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


# The binding itself: one record per public header -- its prototypes {function: (restype, argtypes)}, the function that
# reports its ABI with the version this binding is written for, and {size function: ctypes mirror} for the structures
# whose layout the library reports.  tests/test_native_bindings.py holds every prototype against its declaration.
_Header = collections.namedtuple("_Header", "name abi_fn abi sizes protos")
_P = ctypes.POINTER
_int, _u32, _i64, _u64, _f64, _size = (ctypes.c_int, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double,
                                       ctypes.c_size_t)
_vp, _dp, _i32p, _u8p = ctypes.c_void_p, _P(ctypes.c_double), _P(ctypes.c_int32), _P(ctypes.c_uint8)
_pp, _op, _scp, _cp = _P(LmpcParams), _P(LmpcOptions), _P(LmpcSynthCfg), _P(LmpcCommand)
_kp, _hdp, _hop, _rcp = _P(LmpcLegKin), _P(LmpcHoqpDims), _P(LmpcHoqpOptions), _P(LmpcRolloutCfg)
_rbp, _mp, _sp, _tp = _P(LmpcRobot), _P(LmpcRbdModel), _P(LmpcRbdState), _P(LmpcWbcTarget)
_cfp, _sop, _srp, _esp = _P(LmpcSimCfg), _P(LmpcSimOut), _P(LmpcStackRobot), _P(LmpcEstSensors)
_ecp, _efp, _eop, _ccp = _P(LmpcEstCfg), _P(LmpcEstFilter), _P(LmpcEstOut), _P(LmpcContactCfg)
_cop, _lcp, _lop, _lgp = _P(LmpcContactOut), _P(LmpcLowlevelCfg), _P(LmpcLowlevelOut), _P(LmpcLowsimLog)
_HEADERS = (
    _Header("lmpc.h", "lmpc_abi_version", ABI_VERSION, {}, {
        "lmpc_params_go1": (None, [_pp]),
        "lmpc_params_a1": (None, [_pp]),
        "lmpc_options_default": (None, [_op]),
        "lmpc_record_len": (_int, [_int]),
        "lmpc_abi_version": (_int, []),
        "lmpc_strerror": (ctypes.c_char_p, [_int]),
        "lmpc_create": (_int, [_pp, _int, _int, _int, _P(_vp)]),
        "lmpc_destroy": (None, [_vp]),
        "lmpc_set_options": (_int, [_vp, _op]),
        "lmpc_set_params": (_int, [_vp, _pp]),
        "lmpc_reserve": (_int, [_vp, _int]),
        "lmpc_solve_batch": (_int, [_vp, _dp, _u8p, _int, _dp, _i32p, _i32p]),
        "lmpc_solve_batch_device": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
        "lmpc_sync": (_int, [_vp]),
        "lmpc_predict_contact": (_int, [_int, _int, _f64, _f64, _f64]),
        "lmpc_current_contact": (_int, [_int, _int, _f64]),
        "lmpc_contact_schedule": (_int, [_int, _f64, _f64, _f64, _int, _u8p, _u8p]),
        "lmpc_pack_record": (_int, [_pp, _int, _P(LmpcStateIn), _dp, _dp]),
        "lmpc_synth_cfg_go1": (None, [_scp]),
        "lmpc_synth_cfg_a1_standing": (None, [_scp]),
        "lmpc_synth_fill": (_int, [_pp, _scp, _int, _u64, _i64, _int, _dp, _u8p]),
        # ABI 2: terrain extension
        "lmpc_terrain_frame": (None, [_dp, _dp]),
        "lmpc_solve_batch_ex": (_int, [_vp, _dp, _u8p, _dp, _int, _dp, _i32p, _i32p]),
        "lmpc_solve_batch_warm": (_int, [_vp, _dp, _u8p, _dp, _int, _u8p, _u8p, _dp, _i32p, _i32p]),
        "lmpc_shift_active_set": (None, [_u8p, _int, _int, _u8p]),
        "lmpc_solve_batch_device_ex": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
        "lmpc_synth_normals": (_int, [_u64, _i64, _int, _f64, _dp]),
        # on-device input generation
        "lmpc_command_to_record": (_int, [_pp, _int, _cp, _dp, _u8p]),
        "lmpc_build_records_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp]),
        "lmpc_solve_commands_device": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
        "lmpc_synth_commands": (_int, [_scp, _u64, _i64, _int, _cp]),
        "lmpc_synth_commands_device": (_int, [_vp, _scp, _u64, _i64, _int, _vp, _vp]),
        "lmpc_synth_normals_device": (_int, [_vp, _u64, _i64, _int, _f64, _vp, _vp]),
        # GRF -> joint torque
        "lmpc_leg_kin_default": (None, [_kp]),
        "lmpc_foot_jacobian": (None, [_kp, _int, _dp, _dp]),
        "lmpc_grf_to_torque": (_int, [_kp, _dp, _dp, _dp, _dp]),
        "lmpc_grf_to_torque_device": (_int, [_vp, _kp, _vp, _vp, _vp, _int, _vp, _vp]),
        # ABI 3: dense-path selection
        "lmpc_set_dense_path": (_int, [_vp, _int]),
        "lmpc_get_dense_path": (_int, [_vp]),
        "lmpc_set_riccati_path": (_int, [_vp, _int]),
        "lmpc_get_riccati_path": (_int, [_vp]),
        # ABI 7: per-leg gait phases, warm-start workspace
        "lmpc_contact_schedule_legs": (_int, [_int, _dp, _f64, _f64, _int, _u8p, _u8p]),
        "lmpc_reserve_warm": (_int, [_vp, _int]),
    }),
    _Header("lmpc_hoqp.h", "lmpc_hoqp_abi_version", HOQP_ABI_VERSION, {}, {
        "lmpc_hoqp_dims_wbc": (None, [_hdp]),
        "lmpc_hoqp_options_default": (None, [_hop]),
        "lmpc_hoqp_record_len": (_i64, [_hdp]),
        "lmpc_hoqp_slack_len": (_int, [_hdp]),
        "lmpc_hoqp_lds_bytes": (_i64, [_hdp]),
        "lmpc_hoqp_create": (_int, [_hdp, _int, _int, _P(_vp)]),
        "lmpc_hoqp_destroy": (None, [_vp]),
        "lmpc_hoqp_set_options": (_int, [_vp, _hop]),
        "lmpc_hoqp_solve_batch": (_int, [_vp, _dp, _int, _dp, _dp, _i32p, _i32p]),
        "lmpc_hoqp_solve_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
        "lmpc_hoqp_sync": (_int, [_vp]),
        "lmpc_wbc_tasks": (_int, [_P(LmpcWbcInput), _dp]),
        "lmpc_wbc_tasks_device": (_int, [_vp, _int, _vp, _vp]),
        "lmpc_hoqp_solve_batch_z": (_int, [_vp, _dp, _int, _dp, _dp, _i32p, _i32p, _dp, _i32p]),
        "lmpc_hoqp_solve_device_z": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        # ABI 2: warm start from the last solve's active sets
        "lmpc_hoqp_abi_version": (_int, []),
        "lmpc_hoqp_act_len": (_i64, [_hdp]),
        "lmpc_hoqp_solve_batch_warm": (_int, [_vp, _dp, _int, _dp, _dp, _i32p, _i32p, _P(_u64)]),
        "lmpc_hoqp_solve_device_warm": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    }),
    _Header("lmpc_rollout.h", "lmpc_rollout_abi_version", ROLLOUT_ABI_VERSION, {"lmpc_robot_size": LmpcRobot}, {
        "lmpc_rollout_abi_version": (_int, []),
        "lmpc_robot_size": (_int, []),
        "lmpc_rollout_cfg_go1": (None, [_rcp]),
        "lmpc_robot_init": (_int, [_rcp, _dp, _dp, _f64, _f64, _int, _f64, _rbp]),
        "lmpc_robot_plant_step": (_int, [_pp, _rbp, _dp]),
        "lmpc_robot_advance": (_int, [_pp, _rcp, _rbp, _dp, _dp]),
        "lmpc_shift_active_set_device": (_int, [_vp, _vp, _int, _vp, _vp]),
        "lmpc_solve_commands_warm_device": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
        "lmpc_rollout_device": (_int, [_vp, _rcp, _vp, _vp, _int, _int, _P(LmpcRolloutLog), _vp]),
    }),
    _Header("lmpc_rbd.h", "lmpc_rbd_abi_version", RBD_ABI_VERSION,
            {"lmpc_rbd_model_size": LmpcRbdModel, "lmpc_rbd_state_size": LmpcRbdState,
             "lmpc_wbc_target_size": LmpcWbcTarget, "lmpc_rbd_terms_size": LmpcRbdTerms}, {
        "lmpc_rbd_abi_version": (_int, []),
        "lmpc_rbd_model_size": (_int, []),
        "lmpc_rbd_state_size": (_int, []),
        "lmpc_wbc_target_size": (_int, []),
        "lmpc_rbd_terms_size": (_int, []),
        "lmpc_rbd_model_go1": (None, [_mp]),
        "lmpc_rbd_model_a1": (None, [_mp]),
        "lmpc_wbc_target_default": (None, [_tp]),
        "lmpc_rbd_compute": (_int, [_mp, _sp, _P(LmpcRbdTerms)]),
        "lmpc_wbc_input_from_state": (_int, [_mp, _sp, _tp, _P(LmpcWbcInput)]),
        "lmpc_wbc_inputs_device": (_int, [_mp, _vp, _vp, _int, _vp, _vp]),
        "lmpc_rbd_compute_device": (_int, [_mp, _vp, _int, _vp, _vp]),
    }),
    _Header("lmpc_sim.h", "lmpc_sim_abi_version", SIM_ABI_VERSION,
            {"lmpc_sim_cfg_size": LmpcSimCfg, "lmpc_sim_out_size": LmpcSimOut}, {
        "lmpc_sim_abi_version": (_int, []),
        "lmpc_sim_cfg_size": (_int, []),
        "lmpc_sim_out_size": (_int, []),
        "lmpc_sim_cfg_default": (None, [_cfp]),
        "lmpc_sim_work_bytes": (_size, [_int]),
        "lmpc_rbd_forward_dynamics": (_int, [_mp, _sp, _dp, _i32p, _int, _sop]),
        "lmpc_sim_step": (_int, [_mp, _cfp, _sp, _dp, _i32p, _sp, _sop]),
        "lmpc_rbd_forward_dynamics_device": (_int, [_mp, _vp, _vp, _i64, _vp, _i64, _int, _int, _vp, _vp]),
        "lmpc_sim_step_device": (_int, [_mp, _cfp, _vp, _vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _vp, _size, _vp]),
    }),
    _Header("lmpc_stack.h", "lmpc_stack_abi_version", STACK_ABI_VERSION, {"lmpc_stack_robot_size": LmpcStackRobot}, {
        "lmpc_stack_abi_version": (_int, []),
        "lmpc_stack_robot_size": (_int, []),
        "lmpc_stack_check_rates": (_int, [_pp, _cfp, _int, _int]),
        "lmpc_stack_robot_init": (_int, [_rcp, _mp, _sp, _dp, _f64, _f64, _int, _f64, _srp, _sop]),
        "lmpc_stack_advance": (_int, [_pp, _rcp, _srp, _sp, _sop, _dp]),
        "lmpc_stack_targets": (_int, [_srp, _dp, _tp, _tp]),
        "lmpc_stack_reserve": (_int, [_vp, _int]),
        "lmpc_stack_advance_device": (_int, [_vp, _rcp, _vp, _vp, _vp, _int, _vp]),
        "lmpc_stack_solve_device": (_int, [_vp, _int, _vp, _vp, _vp, _vp]),
        "lmpc_stack_copy_records_device": (_int, [_vp, _int, _vp, _vp, _vp]),
        "lmpc_stack_targets_device": (_int, [_vp, _vp, _i64, _tp, _int, _vp, _vp]),
        "lmpc_stack_candidates_device": (_int, [_vp, _int, _vp, _vp]),
    }),
    _Header("lmpc_est.h", "lmpc_est_abi_version", EST_ABI_VERSION,
            {"lmpc_est_sensors_size": LmpcEstSensors, "lmpc_est_cfg_size": LmpcEstCfg,
             "lmpc_est_filter_size": LmpcEstFilter, "lmpc_est_out_size": LmpcEstOut}, {
        "lmpc_est_abi_version": (_int, []),
        "lmpc_est_sensors_size": (_int, []),
        "lmpc_est_cfg_size": (_int, []),
        "lmpc_est_filter_size": (_int, []),
        "lmpc_est_out_size": (_int, []),
        "lmpc_est_cfg_default": (None, [_ecp]),
        "lmpc_est_sensors_from_plant": (_int, [_mp, _ecp, _sp, _sop, _int, _u32, _int, _esp]),
        "lmpc_est_init": (_int, [_mp, _ecp, _esp, _dp, _efp]),
        "lmpc_est_report": (_int, [_mp, _esp, _efp, _sp, _eop]),
        "lmpc_est_update": (_int, [_mp, _ecp, _esp, _efp, _sp, _eop]),
        "lmpc_est_feedback": (_int, [_sop, _eop, _sop]),
        "lmpc_est_sensors_from_plant_device": (_int, [_mp, _ecp, _vp, _vp, _int, _int, _u32, _vp, _i64, _vp, _vp]),
        "lmpc_est_init_device": (_int, [_mp, _ecp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
        "lmpc_est_update_device": (_int, [_mp, _ecp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    }),
    _Header("lmpc_contact.h", "lmpc_contact_abi_version", CONTACT_ABI_VERSION,
            {"lmpc_contact_cfg_size": LmpcContactCfg, "lmpc_contact_out_size": LmpcContactOut}, {
        "lmpc_contact_abi_version": (_int, []),
        "lmpc_contact_cfg_size": (_int, []),
        "lmpc_contact_out_size": (_int, []),
        "lmpc_contact_cfg_default": (None, [_ccp]),
        "lmpc_contact_work_bytes": (_size, [_int]),
        "lmpc_contact_solve": (_int, [_ccp, _dp, _dp, _i32p, _dp, _cop]),
        "lmpc_contact_step": (_int, [_mp, _ccp, _sp, _dp, _i32p, _sp, _sop, _cop]),
        "lmpc_contact_solve_device": (_int, [_ccp, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
        "lmpc_contact_step_device": (_int, [_mp, _ccp, _vp, _vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _size,
                                            _vp]),
    }),
    _Header("lmpc_lowlevel.h", "lmpc_lowlevel_abi_version", LOWLEVEL_ABI_VERSION,
            {"lmpc_lowlevel_cfg_size": LmpcLowlevelCfg, "lmpc_lowlevel_out_size": LmpcLowlevelOut}, {
        "lmpc_lowlevel_abi_version": (_int, []),
        "lmpc_lowlevel_cfg_size": (_int, []),
        "lmpc_lowlevel_out_size": (_int, []),
        "lmpc_lowlevel_block_robots": (_int, []),
        "lmpc_lowlevel_cfg_go1": (None, [_lcp]),
        "lmpc_lowlevel_cfg_a1": (None, [_lcp]),
        "lmpc_leg_kin_from_model": (_int, [_mp, _kp]),
        "lmpc_leg_fk": (_int, [_kp, _int, _dp, _dp]),
        "lmpc_leg_inv_kin": (_int, [_kp, _int, _dp, _dp, _dp]),
        "lmpc_lowlevel": (_int, [_lcp, _sp, _tp, _i32p, _lop]),
        "lmpc_lowlevel_device": (_int, [_lcp, _vp, _vp, _vp, _i64, _vp, _vp, _int, _vp, _vp]),
    }),
    _Header("lmpc_lowsim.h", "lmpc_lowsim_abi_version", LOWSIM_ABI_VERSION, {}, {
        "lmpc_lowsim_abi_version": (_int, []),
        "lmpc_lowsim_block_robots": (_int, []),
        "lmpc_lowsim_run": (_int, [_mp, _cfp, _lcp, _sp, _tp, _i32p, _sop, _i32p, _lop, _int, _int, _lgp]),
        "lmpc_lowsim_run_device": (_int, [_mp, _cfp, _lcp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _int, _int, _int, _lgp,
                                          _vp]),
    }),
    _Header("lmpc_multi.h", "lmpc_multi_abi_version", MULTI_ABI_VERSION, {}, {
        "lmpc_multi_abi_version": (_int, []),
        "lmpc_multi_shard": (None, [_int, _int, _int, _i32p, _i32p]),
        "lmpc_multi_create": (_int, [_pp, _int, _i32p, _int, _P(_vp)]),
        "lmpc_multi_destroy": (None, [_vp]),
        "lmpc_multi_num_devices": (_int, [_vp]),
        "lmpc_multi_set_options": (_int, [_vp, _op]),
        "lmpc_multi_set_dense_path": (_int, [_vp, _int]),
        "lmpc_multi_solve_commands_device": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
        "lmpc_multi_solve_synth_device": (_int, [_vp, _scp, _u64, _i64, _int, _f64, _vp, _vp, _vp]),
        "lmpc_multi_solve_commands": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _vp]),
    }),
)

_BY_NAME = {h.name: h for h in _HEADERS}
# every symbol a header declares, in the table's order (the tests hold each tuple against its header)
EXPORTED_SYMBOLS = tuple(_BY_NAME["lmpc.h"].protos)
HOQP_SYMBOLS = tuple(_BY_NAME["lmpc_hoqp.h"].protos)
ROLLOUT_SYMBOLS = tuple(_BY_NAME["lmpc_rollout.h"].protos)
RBD_SYMBOLS = tuple(_BY_NAME["lmpc_rbd.h"].protos)
SIM_SYMBOLS = tuple(_BY_NAME["lmpc_sim.h"].protos)
STACK_SYMBOLS = tuple(_BY_NAME["lmpc_stack.h"].protos)
EST_SYMBOLS = tuple(_BY_NAME["lmpc_est.h"].protos)
CONTACT_SYMBOLS = tuple(_BY_NAME["lmpc_contact.h"].protos)
LOWLEVEL_SYMBOLS = tuple(_BY_NAME["lmpc_lowlevel.h"].protos)
LOWSIM_SYMBOLS = tuple(_BY_NAME["lmpc_lowsim.h"].protos)
MULTI_SYMBOLS = tuple(_BY_NAME["lmpc_multi.h"].protos)


def _bind(L, path: str, headers) -> None:
    """Give every function of `headers` its prototype, then hold the library to the binding's ABI and structure sizes.
    Each header's ABI is read before its other functions are looked up, so a library of another ABI is reported as
    that, not as the first symbol it lacks."""
    def symbol(h, name):
        try:
            return getattr(L, name)
        except AttributeError:
            raise NativeLibraryError(f"{path}: no symbol {name} (include/lmpc/{h.name})") from None

    for h in headers:
        report = symbol(h, h.abi_fn)
        report.restype, report.argtypes = h.protos[h.abi_fn]
        abi, sizes, mirrors = report(), {}, {name: ctypes.sizeof(cls) for name, cls in h.sizes.items()}
        if abi == h.abi:
            for name, (restype, argtypes) in h.protos.items():
                fn = symbol(h, name)
                fn.restype, fn.argtypes = restype, argtypes
            sizes = {name: getattr(L, name)() for name in h.sizes}
        if abi != h.abi or sizes != mirrors:
            raise NativeLibraryError(f"{path}: {h.name}: the library is ABI {abi} with structure sizes {sizes}, this "
                                     f"binding is ABI {h.abi} with {mirrors}")


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
        _bind(L, path, [h for h in _HEADERS if h.name != "lmpc_multi.h"])
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
        _bind(M, MULTI_LIB_PATH, [_BY_NAME["lmpc_multi.h"]])
        _mlib = M
        return M


def check(rc: int, what: str = "lmpc") -> None:
    if rc != LMPC_OK:
        msg = "RCCL communication failed" if rc == LMPC_ERR_COMM else lib().lmpc_strerror(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} ({rc})")
