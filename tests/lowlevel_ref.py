"""Independent NumPy restatement of the reference's joint-PD low-level controller (test helper, not a test), read from
the reference's lines (relative to src/legged_ctrl/src):

    BaseInterface::tau_ctrl_update     interfaces/BaseInterface.cpp:451-489
    A1Kinematics::fk / inv_kin         utils/A1Kinematics.cpp:38-75, 321-446
    the torque sent                    interfaces/GazeboInterface.cpp:106-110

It shares nothing with the library: the foot position is the reference's expanded expression, J is the complex step of
that `fk` (not a closed form), and the velocity solve is `np.linalg.solve`.  For a pose `inv_kin` also returns its
margins to every branch boundary, so that a test can keep away from poses where a rounding error picks the branch.
"""
import numpy as np

H_STEP = 1e-30


def rot(euler):
    """R = Rz(yaw) Ry(pitch) Rx(roll); euler = (yaw, pitch, roll) as in lmpc_rbd_state."""
    y, p, r = euler
    Rz = np.array([[np.cos(y), -np.sin(y), 0.0], [np.sin(y), np.cos(y), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(p), 0.0, np.sin(p)], [0.0, 1.0, 0.0], [-np.sin(p), 0.0, np.cos(p)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(r), -np.sin(r)], [0.0, np.sin(r), np.cos(r)]])
    return Rz @ Ry @ Rx


def fk(rho_fix, rho_opt, q):
    """autoFunc_fk_derive (A1Kinematics.cpp:40-75), term for term; q may be complex."""
    in1, in2, in3 = q, rho_opt, rho_fix
    t2, t3, t4 = np.cos(in1[0]), np.cos(in1[1]), np.cos(in1[2])
    t5, t6, t7 = np.sin(in1[0]), np.sin(in1[1]), np.sin(in1[2])
    t8 = in1[1] + in1[2]
    t9 = np.sin(t8)
    x = (((in3[0] + in2[2] * t9) - in3[4] * t9) - t6 * in3[3]) + in2[0] * np.cos(t8)
    y = ((((((((in3[1] + in2[1] * t2) + in3[2] * t2) + t3 * t5 * in3[3]) + in2[0] * t3 * t5 * t7) +
             in2[0] * t4 * t5 * t6) - in2[2] * t3 * t4 * t5) + in2[2] * t5 * t6 * t7) + in3[4] * t3 * t4 * t5) - \
        in3[4] * t5 * t6 * t7
    a, b, c = in2[0] * t2, in2[2] * t2, in3[4] * t2
    z = (((((((in2[1] * t5 + in3[2] * t5) - t2 * t3 * in3[3]) - a * t3 * t7) - a * t4 * t6) + b * t3 * t4) -
          b * t6 * t7) - c * t3 * t4) + c * t6 * t7
    return np.array([x, y, z])


def jac(rho_fix, rho_opt, q):
    """d fk / d q by the complex step: exact to rounding, no closed form."""
    J = np.zeros((3, 3))
    for k in range(3):
        qc = np.array(q, dtype=complex)
        qc[k] += 1j * H_STEP
        J[:, k] = fk(rho_fix, rho_opt, qc).imag / H_STEP
    return J


def inv_kin(rho_fix, p, cur_q):
    """A1Kinematics::inv_kin (A1Kinematics.cpp:321-446) -> (q [3], the smallest margin to a branch boundary, the
    margins by name)."""
    ox, oy, d, lt, lc = (float(v) for v in rho_fix)
    Xf, Yf, Zf = (float(v) for v in p)
    Yf_, Xf_ = Yf - oy, Xf - ox
    with np.errstate(invalid="ignore"):
        L = float(np.sqrt(Zf * Zf + Yf_ * Yf_ - d * d))
    t1 = t1c = 0.0
    at = np.arctan2
    if oy > 0:
        if Zf > 0:
            if Yf_ > 0:
                t1 = at(Zf, Yf_) - at(L, d)
            elif Yf_ == 0:
                t1 = np.pi / 2 - at(L, d)
            elif Yf_ < 0:
                t1 = np.pi - at(Zf, -Yf_) - at(L, d)
            t1c = at(Zf, Yf_) + at(L, d)
        elif Zf < 0:
            if Yf_ > 0:
                t1 = at(Zf, Yf_) + at(L, d)
            elif Yf_ == 0:
                t1 = -np.pi / 2 + at(L, d)
            elif Yf_ < 0:
                t1 = -np.pi - at(Zf, -Yf_) + at(L, d)
            t1c = at(Zf, Yf_) - at(L, d)
        else:
            t1, t1c = at(L, d), -at(L, d)
    else:
        if Zf > 0:
            if Yf_ < 0:
                t1 = -at(Zf, -Yf_) + at(L, -d)
            elif Yf_ == 0:
                t1 = -np.pi / 2 + at(L, -d)
            elif Yf_ > 0:
                t1 = -np.pi + at(Zf, Yf_) + at(L, -d)
            t1c = -at(L, -d) - at(Zf, -Yf_)
        elif Zf < 0:
            if Yf_ < 0:
                t1 = at(-Zf, -Yf_) - at(L, -d)
            elif Yf_ == 0:
                t1 = -np.pi / 2 - at(L, -d)
            elif Yf_ > 0:
                t1 = np.pi - at(-Zf, Yf_) - at(L, -d)
            t1c = at(-Zf, -Yf_) + at(L, -d)
    m = {"Zf": abs(Zf), "Yf_": abs(Yf_), "t1_choice": abs(abs(t1 - cur_q[0]) - abs(t1c - cur_q[0]))}
    if not abs(t1 - cur_q[0]) < abs(t1c - cur_q[0]):
        t1 = t1c
    cos_beta = (lt * lt + lc * lc - Xf_ * Xf_ - L * L) / (2 * lt * lc)
    m["cos_beta"] = min(abs(abs(cos_beta + 1) - 0.001), abs(abs(cos_beta - 1) - 0.001))
    if abs(cos_beta + 1) < 0.001:
        beta = np.pi
    elif abs(cos_beta - 1) < 0.001:
        beta = 0.0
    else:
        with np.errstate(invalid="ignore"):
            beta = float(np.arccos(cos_beta))
    t3 = beta - np.pi
    j2z = d * np.sin(t1)
    m["L_flip"] = abs(Zf - j2z)
    if Zf > j2z:
        L = -L
    t2 = at(-Xf_, L) + at(lc * np.sin(-t3), lt + lc * np.cos(-t3))
    m["t2_wrap"] = min(abs(t2 + 60 * np.pi / 180), abs(t2 - 240 * np.pi / 180))
    if t2 < -60 * np.pi / 180:
        t2 = t2 + 2 * np.pi
    elif t2 > 240 * np.pi / 180:
        t2 = t2 - 2 * np.pi
    vals = [v for v in m.values()]
    margin = float("nan") if any(np.isnan(v) for v in vals) else float(min(vals))
    return np.array([t1, t2, t3]), margin, m


def lowlevel(cfg, state, forces_des, foot_pos_des, foot_vel_des, mode):
    """One robot.  cfg: dict(rho_fix [4][5], rho_opt [4][3], kp [4][3], kd [4][3], tau_limit [3]); state: the 36
    doubles of lmpc_rbd_state -> dict(tau, joint_tau_tgt, joint_ang_tgt, joint_vel_tgt [12], flags [4], margin)."""
    s = np.asarray(state, dtype=np.float64)
    euler, pos, q, lin_vel, qd = s[0:3], s[3:6], s[6:18], s[21:24], s[24:36]
    R = rot(euler)
    out = dict(tau=np.zeros(12), joint_tau_tgt=np.zeros(12), joint_ang_tgt=np.zeros(12), joint_vel_tgt=np.zeros(12),
               flags=np.zeros(4, dtype=np.int32), margin=np.inf)
    for i in range(4):
        sl = slice(3 * i, 3 * i + 3)
        rf, ro = np.asarray(cfg["rho_fix"][i], dtype=np.float64), np.asarray(cfg["rho_opt"][i], dtype=np.float64)
        J = jac(rf, ro, q[sl])
        ff = -J.T @ (R.T @ np.asarray(forces_des, dtype=np.float64)[sl])
        ang, vel, flags = q[sl].copy(), qd[sl].copy(), 0
        if mode > 0:
            p_rel = R.T @ (np.asarray(foot_pos_des, dtype=np.float64)[sl] - pos)
            v_rel = R.T @ (np.asarray(foot_vel_des, dtype=np.float64)[sl] - lin_vel)
            a, margin, _ = inv_kin(rf, p_rel, q[sl])
            out["margin"] = min(out["margin"], margin) if not np.isnan(margin) else float("nan")
            if np.any(np.isnan(a)):
                flags |= 1
            else:
                ang = a
            with np.errstate(all="ignore"):
                try:
                    w = np.linalg.solve(J, v_rel)
                except np.linalg.LinAlgError:
                    w = np.full(3, np.nan)
            if np.any(np.isnan(w)):
                flags |= 2
            else:
                vel = w
        with np.errstate(all="ignore"):
            tau = np.asarray(cfg["kp"][i]) * (ang - q[sl]) + np.asarray(cfg["kd"][i]) * (vel - qd[sl]) + ff
        if not np.all(np.isfinite(tau)):
            flags |= 4
        for k in range(3):
            lim = float(cfg["tau_limit"][k])
            if lim > 0 and abs(tau[k]) > lim:
                tau[k] = np.sign(tau[k]) * lim
                flags |= 8
        out["tau"][sl], out["joint_tau_tgt"][sl] = tau, ff
        out["joint_ang_tgt"][sl], out["joint_vel_tgt"][sl] = ang, vel
        out["flags"][i] = flags
    return out


def cfg_dict(c):
    """An lmpc_lowlevel_cfg (ctypes mirror) -> the dict `lowlevel` takes."""
    return dict(rho_fix=np.array([list(r) for r in c.kin.rho_fix]), rho_opt=np.array([list(r) for r in c.kin.rho_opt]),
                kp=np.array([list(r) for r in c.kp]), kd=np.array([list(r) for r in c.kd]),
                tau_limit=np.array(list(c.tau_limit)))
