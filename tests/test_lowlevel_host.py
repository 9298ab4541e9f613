"""CPU tests of the joint-PD low-level controller (include/lmpc/lmpc_lowlevel.h): the host functions against the
independent NumPy restatement tests/lowlevel_ref.py (complex-step Jacobian of the reference's expanded fk,
np.linalg.solve), the kinematics read off the rigid-body models, hand cases for every flag, and the loop closed on the
CPU: host advance, the oracle's exact QP solve, host targets, `lmpc_lowlevel`, the host plant.

Tolerances.  Host against the restatement: 1e-12 relative to max(1, |ref|), the bound test_grf_to_torque_device_vs_oracle
uses for the same Jacobian; flags bit for bit.  Only cases whose every inverse-kinematics branch margin (lowlevel_ref)
exceeds 1e-6 are compared -- on a boundary a rounding error picks the branch -- and at most 5 % of the drawn cases may be
dropped for it.  The round trip inv_kin(fk(q), q) is held to ten times the restatement's own worst error on the same
poses, which the test computes.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import lowlevel_ref as LR
import model_sets
from conftest import ROOT, rel_err
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import lowlevel as LL
from legged_mpc_control_amd import rbd, rollout, sim, stack, synth
from oracle import oracle as O
from test_rbd_host import model_json, preset

ROBOTS = ("go1", "a1")
N_CASES = 256
SEED = 20241
MARGIN = 1e-6
TOL = 1e-12
Q_LO, Q_HI = np.array([-0.8, -0.6, -2.6]), np.array([0.8, 2.0, -0.9])
FIELDS = ("tau", "joint_tau_tgt", "joint_ang_tgt", "joint_vel_tgt")


def cfg_for(name):
    """The robot's own Gazebo gains on the kinematics of its own rigid-body model."""
    return LL.cfg_go1(preset(name)) if name == "go1" else LL.cfg_a1(preset(name))


def target_of(forces, pos_des, vel_des):
    t = rbd.target()
    t.forces_des[:] = [float(v) for v in forces]
    t.foot_pos_des[:] = [float(v) for v in pos_des]
    t.foot_vel_des[:] = [float(v) for v in vel_des]
    return t


def draw_case(rng, ref_cfg):
    """A random trunk pose (|roll|, |pitch| <= 0.3), joints in the round trip's ranges, rates, forces up to 150 N, and
    foot targets fk(q + delta), |delta| <= 0.2, put into the world frame."""
    s = np.zeros(36)
    s[0], s[1:3] = rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.3, 2)
    s[3:5], s[5] = rng.uniform(-1.0, 1.0, 2), rng.uniform(0.25, 0.35)
    s[6:18] = rng.uniform(Q_LO, Q_HI, (4, 3)).reshape(12)
    s[18:21], s[21:24], s[24:36] = rng.normal(0, 0.3, 3), rng.uniform(-0.5, 0.5, 3), rng.uniform(-2.0, 2.0, 12)
    R = LR.rot(s[0:3])
    delta = rng.uniform(-0.2, 0.2, (4, 3))
    pos_des = np.concatenate([R @ LR.fk(ref_cfg["rho_fix"][l], ref_cfg["rho_opt"][l], s[6 + 3 * l:9 + 3 * l] + delta[l])
                              + s[3:6] for l in range(4)])
    return dict(state=s, forces=rng.uniform(-150.0, 150.0, 12), pos_des=pos_des, vel_des=rng.uniform(-1.0, 1.0, 12))


@functools.lru_cache(maxsize=None)
def kept_cases():
    """{(robot, mode): dict(cfg, cases, refs, drawn)}: N_CASES seeded cases each whose restatement keeps every branch
    margin above MARGIN, computed once (tests/test_gpu_lowlevel.py draws its batches from them)."""
    out = {}
    for ri, name in enumerate(ROBOTS):
        c = cfg_for(name)
        ref_cfg = LR.cfg_dict(c)
        for mode in (0, 1):
            rng = np.random.default_rng(SEED + 10 * ri + mode)
            cases, refs, drawn = [], [], 0
            while len(cases) < N_CASES:
                drawn += 1
                assert drawn <= 2 * N_CASES, "the restatement drops too many cases: choose another seed"
                case = draw_case(rng, ref_cfg)
                ref = LR.lowlevel(ref_cfg, case["state"], case["forces"], case["pos_des"], case["vel_des"], mode)
                if mode == 1 and not ref["margin"] > MARGIN:
                    continue
                cases.append(case)
                refs.append(ref)
            out[(name, mode)] = dict(cfg=c, cases=cases, refs=refs, drawn=drawn)
    return out


def run_host(c, case, mode):
    gait = N.GAIT_STAND if mode == 0 else N.GAIT_TROT
    return LL.lowlevel(c, rbd.state_from_vector(case["state"]), target_of(case["forces"], case["pos_des"], case["vel_des"]),
                       gait)


def hand_cases():
    """(name, cfg, case, mode) of the hand cases, shared with the GPU test: out of reach, a NaN force, the clamp, mode
    0."""
    c = cfg_for("go1")
    base = kept_cases()[("go1", 1)]["cases"][0]
    far = dict(base, pos_des=base["pos_des"].copy())
    hip = np.array(c.kin.rho_fix[0][0:2] + [0.0])  # FL's target 1 m from its hip, outwards and down (body frame)
    far["pos_des"][0:3] = LR.rot(base["state"][0:3]) @ (hip + [0.0, 0.6, -0.8]) + base["state"][3:6]
    nanf = dict(base, forces=base["forces"].copy())
    nanf["forces"][7] = np.nan
    heavy = dict(base, forces=np.tile([0.0, 0.0, 150.0], 4))
    return [("far", c, far, 1), ("nan_force", c, nanf, 1), ("clamp", LL.cfg_go1(preset("go1"), tau_limit=5.0), heavy, 1),
            ("mode0", c, base, 0)]


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_binding_sizes_and_presets():
    L = N.lib()
    assert L.lmpc_lowlevel_abi_version() == N.LOWLEVEL_ABI_VERSION == 1
    assert (L.lmpc_lowlevel_cfg_size(), L.lmpc_lowlevel_out_size()) == (LL.CFG_BYTES, LL.OUT_BYTES) == (472, 400)
    assert N.LmpcLowlevelOut.tau.offset == 0 and N.LmpcLowlevelOut.flags.offset == 384 and LL.TAU_STRIDE == 50
    assert L.lmpc_lowlevel_block_robots() >= 1
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmpc", "lmpc_lowlevel.h")).read(), flags=re.S)
    assert sorted(N.LOWLEVEL_SYMBOLS) == sorted(set(re.findall(r"\b(lmpc_[a-z0-9_]+)\s*\(", src)))
    for sym in N.LOWLEVEL_SYMBOLS:
        assert hasattr(L, sym), sym
    kin = N.LmpcLegKin()
    L.lmpc_leg_kin_default(ctypes.byref(kin))
    for c, kp, kd in ((LL.cfg_go1(), 0.5, 0.3), (LL.cfg_a1(), 15.0, 0.4)):
        assert bytes(c.kin) == bytes(kin)
        assert np.all(np.array([list(r) for r in c.kp]) == kp) and np.all(np.array([list(r) for r in c.kd]) == kd)
        assert list(c.tau_limit) == [0.0, 0.0, 0.0]
    c = LL.cfg_go1(kp=(1.0, 2.0, 3.0), kd=7.0, tau_limit=(4.0, 5.0, 6.0))
    assert [list(r) for r in c.kp] == [[1.0, 2.0, 3.0]] * 4 and list(c.tau_limit) == [4.0, 5.0, 6.0]
    # the shared header stays free of the HIP runtime
    text = open(os.path.join(ROOT, "legged_mpc_control_amd", "csrc", "lmpc_lowlevel_common.h")).read()
    assert "hip_runtime" not in text and "hipLaunch" not in text


def test_argument_errors():
    L = N.lib()
    R_ = ctypes.byref
    c, s, t, o, k = LL.cfg_go1(), N.LmpcRbdState(), rbd.target(), N.LmpcLowlevelOut(), N.LmpcLegKin()
    ERR = -1
    assert L.lmpc_lowlevel(None, R_(s), R_(t), None, R_(o)) == ERR
    assert L.lmpc_lowlevel(R_(c), None, R_(t), None, R_(o)) == ERR
    assert L.lmpc_lowlevel(R_(c), R_(s), None, None, R_(o)) == ERR
    assert L.lmpc_lowlevel(R_(c), R_(s), R_(t), None, None) == ERR
    assert L.lmpc_leg_kin_from_model(None, R_(k)) == ERR and L.lmpc_leg_kin_from_model(R_(rbd.model_go1()), None) == ERR
    z = (ctypes.c_double * 3)()
    assert L.lmpc_leg_fk(R_(c.kin), 4, z, z) == ERR and L.lmpc_leg_inv_kin(R_(c.kin), -1, z, z, z) == ERR
    # the device entry point checks its arguments before touching the device
    p = ctypes.c_void_p(ctypes.addressof(o))
    assert L.lmpc_lowlevel_device(R_(c), None, None, None, 0, None, None, 0, None, None) == 0
    assert L.lmpc_lowlevel_device(R_(c), p, p, None, 0, None, None, -1, p, None) == ERR
    assert L.lmpc_lowlevel_device(None, p, p, None, 0, None, None, 1, p, None) == ERR
    assert L.lmpc_lowlevel_device(R_(c), None, p, None, 0, None, None, 1, p, None) == ERR
    assert L.lmpc_lowlevel_device(R_(c), p, None, None, 0, None, None, 1, p, None) == ERR
    assert L.lmpc_lowlevel_device(R_(c), p, p, None, 0, None, None, 1, None, None) == ERR
    assert L.lmpc_lowlevel_device(R_(c), p, p, p, 0, None, None, 1, p, None) == ERR  # a gait stride below 1
    assert L.lmpc_lowlevel_device(R_(c), p, p, None, 0, p, None, 1, p, None) == ERR  # d_sim_out without d_candidates
    assert L.lmpc_lowlevel_device(R_(c), p, p, None, 0, None, p, 1, p, None) == ERR


# ---- kinematics from the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_leg_kin_from_model_is_the_plants(name):
    """rho_fix read off the model: R fk + pos equals lmpc_rbd_compute's foot_pos to 1e-13."""
    md, model = model_json(name), preset(name)
    kin = LL.leg_kin_from_model(model)
    jo, foot = np.array(md["joint_origin"]), np.array(md["foot"])
    for l in range(4):
        assert list(kin.rho_fix[l]) == [jo[3 * l, 0], jo[3 * l, 1], jo[3 * l + 1, 1], -jo[3 * l + 2, 2], -foot[l, 2]]
        assert list(kin.rho_opt[l]) == [0.0, 0.0, 0.0]
        assert (kin.rho_fix[l][1] > 0) == (l % 2 == 0)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(50):
        s = draw_case(rng, LR.cfg_dict(cfg_for(name)))["state"]
        terms = N.LmpcRbdTerms()
        assert N.lib().lmpc_rbd_compute(ctypes.byref(model), ctypes.byref(rbd.state_from_vector(s)), ctypes.byref(terms)) == 0
        R = LR.rot(s[0:3])
        for l in range(4):
            q = s[6 + 3 * l:9 + 3 * l]
            for p in (LR.fk(list(kin.rho_fix[l]), [0.0] * 3, q), LL.fk(kin, l, q)):
                worst = max(worst, float(np.max(np.abs(R @ p + s[3:6] - np.array(terms.foot_pos[3 * l:3 * l + 3])))))
    print(f"{name}: R fk + pos against lmpc_rbd_compute's foot_pos: {worst:.2e}")
    assert worst <= 1e-13


def test_leg_kin_from_model_rejects_other_classes():
    """The asymmetric robots of tests/model_sets.py whose geometry leaves A1Kinematics' class (offsets off the hip /
    thigh / calf axes) are refused and leave `kin` untouched; "bodies" varies only masses and inertias, its geometry is
    Go1's, and it passes with Go1's lengths."""
    for name in ("lopsided", "feet", "origins"):
        model = rbd.model_from_json(model_sets.model(name))
        kin = N.LmpcLegKin()
        before = bytes(kin)
        assert N.lib().lmpc_leg_kin_from_model(ctypes.byref(model), ctypes.byref(kin)) == -1, name
        assert bytes(kin) == before
        with pytest.raises(ValueError):
            LL.leg_kin_from_model(model)
    assert bytes(LL.leg_kin_from_model(rbd.model_from_json(model_sets.model("bodies")))) == \
        bytes(LL.leg_kin_from_model(preset("go1")))
    # one stray component is enough, and 1e-12 is the line
    md = model_json("go1")
    md["joint_origin"][4][0] = 2e-12
    assert N.lib().lmpc_leg_kin_from_model(ctypes.byref(rbd.model_from_json(md)), ctypes.byref(N.LmpcLegKin())) == -1
    md["joint_origin"][4][0] = 5e-13
    assert N.lib().lmpc_leg_kin_from_model(ctypes.byref(rbd.model_from_json(md)), ctypes.byref(N.LmpcLegKin())) == 0


@pytest.mark.parametrize("name", ROBOTS)
def test_inv_kin_round_trip(name):
    """2000 seeded poses: inv_kin(fk(q), q) = q within ten times the restatement's own worst error on them."""
    kin = LL.leg_kin_from_model(preset(name))
    rng = np.random.default_rng(77)
    q = rng.uniform(Q_LO, Q_HI, (2000, 3))
    worst_ref = worst_lib = 0.0
    for i in range(2000):
        l = i % 4
        rf = list(kin.rho_fix[l])
        back, _, _ = LR.inv_kin(rf, LR.fk(rf, [0.0] * 3, q[i]), q[i])
        worst_ref = max(worst_ref, float(np.max(np.abs(back - q[i]))))
        worst_lib = max(worst_lib, float(np.max(np.abs(LL.inv_kin(kin, l, LL.fk(kin, l, q[i]), q[i]) - q[i]))))
    print(f"{name}: round trip, restatement {worst_ref:.2e} rad, library {worst_lib:.2e} rad")
    assert worst_ref < 1e-10  # the restatement itself inverts these poses
    assert worst_lib <= 10.0 * worst_ref


# ---- host against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("mode", (0, 1))
def test_host_matches_restatement(name, mode):
    k = kept_cases()[(name, mode)]
    dropped = k["drawn"] - N_CASES
    assert dropped <= 0.05 * k["drawn"], f"{dropped} of {k['drawn']} drawn cases dropped"
    worst = {f: 0.0 for f in FIELDS}
    for case, ref in zip(k["cases"], k["refs"]):
        assert ref["margin"] > MARGIN
        o = run_host(k["cfg"], case, mode)
        assert list(o.flags) == list(ref["flags"]) == [0, 0, 0, 0]
        for f in FIELDS:
            worst[f] = max(worst[f], rel_err(np.array(getattr(o, f)), ref[f]))
    print(f"{name} mode {mode}: {dropped} of {k['drawn']} dropped; host vs restatement " +
          ", ".join(f"{f} {v:.2e}" for f, v in worst.items()))
    assert max(worst.values()) <= TOL
    if mode == 1:  # the PD terms are there
        assert any(not np.array_equal(r["tau"], r["joint_tau_tgt"]) for r in k["refs"])


def test_feed_forward_is_grf_to_torque():
    """joint_tau_tgt is lmpc_grf_to_torque's, bit for bit, on the same R."""
    from legged_mpc_control_amd import grf_to_torque

    k = kept_cases()[("go1", 1)]
    for case in k["cases"][:20]:
        o = run_host(k["cfg"], case, 1)
        s = case["state"]
        # the library's own R: root_rot_mat of a robot initialised in this state
        robot, _ = stack.robot_init(rollout.cfg_go1(), preset("go1"), rbd.state_from_vector(s))
        tau = grf_to_torque(k["cfg"].kin, np.array(robot.rb.cmd.state.root_rot_mat), s[6:18], case["forces"])
        assert np.array_equal(tau, np.array(o.joint_tau_tgt))


# ---- hand cases -----------------------------------------------------------------------------------------------------
def test_hand_cases():
    got = {name: (case, run_host(c, case, mode)) for name, c, case, mode in hand_cases()}
    case, o = got["far"]
    assert list(o.flags) == [LL.IK_NAN, 0, 0, 0]
    assert np.array(o.joint_ang_tgt[0:3]).tobytes() == case["state"][6:9].tobytes()
    ref = LR.lowlevel(LR.cfg_dict(cfg_for("go1")), case["state"], case["forces"], case["pos_des"], case["vel_des"], 1)
    assert list(ref["flags"]) == list(o.flags) and rel_err(np.array(o.tau), ref["tau"]) <= TOL
    case, o = got["nan_force"]
    assert list(o.flags) == [0, 0, LL.TAU_NONFINITE, 0] and np.all(np.isnan(o.tau[6:9]))
    assert np.all(np.isfinite(np.array(o.tau)[[0, 1, 2, 3, 4, 5, 9, 10, 11]]))
    case, o = got["clamp"]
    assert all(f & LL.CLAMPED for f in o.flags) and all(f & ~LL.CLAMPED == 0 for f in o.flags)
    assert np.all(np.abs(o.tau) <= 5.0) and np.any(np.abs(o.tau) == 5.0)
    free = run_host(cfg_for("go1"), case, 1)
    hit = np.abs(free.tau) > 5.0
    assert np.array_equal(np.array(o.tau)[~hit], np.array(free.tau)[~hit])
    assert np.array_equal(np.array(o.tau)[hit], 5.0 * np.sign(np.array(free.tau)[hit]))
    case, o = got["mode0"]
    assert np.array(o.tau).tobytes() == np.array(o.joint_tau_tgt).tobytes() and list(o.flags) == [0, 0, 0, 0]
    assert np.array(o.joint_ang_tgt).tobytes() == case["state"][6:18].tobytes()
    assert np.array(o.joint_vel_tgt).tobytes() == case["state"][24:36].tobytes()
    # NULL gait is mode 1
    a = LL.lowlevel(cfg_for("go1"), rbd.state_from_vector(case["state"]),
                    target_of(case["forces"], case["pos_des"], case["vel_des"]), None)
    assert bytes(a) == bytes(run_host(cfg_for("go1"), case, 1)) != bytes(o)


def test_left_right_branch_follows_oy():
    """The left / right split is taken by the sign of rho_fix's oy, for all four legs: with the foot level with the hip
    (Zf == 0) the left branch gives +-atan2(L, d), the right one, which has no such case, gives 0; and a leg whose oy
    and d are mirrored follows the other branch, as the restatement does."""
    kin = LL.leg_kin_from_model(preset("go1"))
    rng = np.random.default_rng(3)
    for l in range(4):
        rf = np.array(kin.rho_fix[l])
        for mirror in (False, True):
            k2 = N.LmpcLegKin.from_buffer_copy(bytes(kin))
            r = rf.copy()
            if mirror:
                r[1], r[2] = -r[1], -r[2]
                k2.rho_fix[l][:] = list(r)
            left = r[1] > 0
            assert left == ((l % 2 == 0) != mirror)
            p = np.array([r[0] + 0.05, r[1] + (0.25 if left else -0.25), 0.0])
            t = LL.inv_kin(k2, l, p, np.zeros(3))
            L = np.sqrt(0.25 ** 2 - r[2] ** 2)
            assert t[0] == (0.0 if not left else -np.arctan2(L, r[2]))  # cur = 0: a tie, which takes the candidate
            for _ in range(20):
                q = rng.uniform(Q_LO, Q_HI)
                if not left:
                    q[0] = -q[0]
                pf = LR.fk(r, [0.0] * 3, q)
                want, margin, _ = LR.inv_kin(r, pf, q)
                if margin > MARGIN:
                    assert np.max(np.abs(LL.inv_kin(k2, l, pf, q) - want)) <= 1e-12


# ---- the loop on the CPU ----------------------------------------------------------------------------------------------
def host_loop(c, state, gait, vel_d, yaw_rate, ticks, W=8, sim_dt=0.00125, H=10):
    """Host advance, the oracle's exact QP, host targets, then W x (lmpc_lowlevel, sim.step) per MPC tick -> the states
    after every low-level tick [ticks * W][36], the plant statuses, the controller's flags."""
    p, rc, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    sc = sim.cfg(dt=sim_dt, ground_z=0.0)
    stack.check_rates(p, sc, W, 1)
    op = O.params_from(p)
    st = rbd.state_from_vector(state)
    robot, out = stack.robot_init(rc, model, st, vel_d, yaw_rate, float(state[5]), gait, 4.0)
    states, statuses, flags = [], [], []
    for _ in range(ticks):
        stack.advance(p, rc, robot, st, out)
        rec, con = synth.command_to_record(p, H, robot.rb.cmd)
        grf, _, _ = O.solve(op, H, rec, con)
        tgt = stack.targets(robot, grf[0])
        for _ in range(W):
            o = LL.lowlevel(c, st, tgt, robot.rb.cmd.gait)
            cand = [int(bool(out.held[l] | out.touch[l])) for l in range(4)]
            st, out = sim.step(model, sc, st, np.array(o.tau), cand)
            states.append(np.frombuffer(bytes(st), dtype=np.float64).copy())
            statuses.append(int(out.status))
            flags.append(list(o.flags))
    return np.array(states), np.array(statuses), np.array(flags)


def standing_state():
    from test_gpu_sim import standing_cases

    md, states, _ = standing_cases()
    s = states[1].copy()
    s[5] -= 1e-6  # the feet below the touch threshold by a margin, as test_gpu_stack.lowered does
    return md, s


def test_closed_loop_trot_on_the_cpu():
    """One Go1 robot trots at 0.3 m/s for 25 MPC ticks of 8 x 1.25 ms on the Go1 gains and the model's kinematics: the
    fall condition of test_trot_does_not_fall."""
    md, s = standing_state()
    x, status, flags = host_loop(LL.cfg_go1(rbd.model_go1()), s, N.GAIT_TROT, (0.3, 0.0), 0.0, 25)
    print(f"trot on the CPU: height {x[:, 5].min():.4f}..{x[:, 5].max():.4f} m (commanded {s[5]:.4f}), roll "
          f"{x[:, 2].min():+.4f}..{x[:, 2].max():+.4f}, pitch {x[:, 1].min():+.4f}..{x[:, 1].max():+.4f} rad, end velocity "
          f"({x[-8:, 21].mean():+.3f}, {x[-8:, 22].mean():+.3f}) m/s, flags {sorted(set(flags.reshape(-1)))}")
    assert np.all(status == 0) and np.all(flags & LL.TAU_NONFINITE == 0)
    assert np.all(np.abs(x[:, 2]) < 0.5) and np.all(np.abs(x[:, 1]) < 0.5)
    assert np.all(x[:, 5] > 0.5 * s[5])


def test_closed_loop_standing_on_the_cpu():
    """10 MPC ticks in LMPC_GAIT_STAND (mode 0: the MPC's forces alone): the height moves by less than a tenth of a
    free fall."""
    md, s = standing_state()
    x, status, flags = host_loop(LL.cfg_go1(rbd.model_go1()), s, N.GAIT_STAND, (0.0, 0.0), 0.0, 10)
    drop = float(np.max(np.abs(x[:, 5] - s[5])))
    free_fall = 0.5 * md["gravity"] * 0.1 ** 2
    print(f"standing on the CPU: trunk height changes by {1e3 * drop:.3f} mm in 0.1 s (free fall {1e3 * free_fall:.1f} mm)")
    assert np.all(status == 0) and np.all(flags == 0)
    assert drop < 0.1 * free_fall


def test_shared_header_under_sanitizers():
    """tests/cpp/lowlevel_host_check.cpp includes csrc/lmpc_lowlevel_common.h and runs a few hundred robots and the hand
    cases; built by the host compiler with -fsanitize=address,undefined and run directly (nothing loaded into Python is
    instrumented)."""
    from legged_mpc_control_amd import build as B

    exe = B.build_cpp_lowlevel_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
