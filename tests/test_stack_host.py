"""CPU tests of the full loop's MPC tick on the host (include/lmpc/lmpc_stack.h: lmpc_stack_robot_init,
lmpc_stack_advance, lmpc_stack_targets, lmpc_stack_check_rates) against the NumPy restatement tests/stack_ref.py
(oracle/fsm.py's LegFSM with its early-touchdown branch, rollout_ref's Bezier and Raibert target).

Tolerances.  FSM state, pattern index, plan_contacts and not_first_call bit for bit; phases, start times, feet, targets
and the Bezier within 1e-13 relative to max(1, |ref|) (the host figure of the linear-plant rollout's tick: the two
sides order a handful of additions differently); the FSM velocity targets, a difference of two such positions over dt,
within 2e-13 / dt.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rbd_ref as RBD
import stack_ref as SR
from conftest import ROOT
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import rbd, rollout, sim, stack
from oracle import fsm as F
from test_rbd_host import model_json, preset

DT = 0.01
TOL = 1e-13
TICKS = 240
SPEED = 2.5  # a swing of the trot lasts 20 ticks, of the crawl 10: one or two of them past 90 %
GAITS = (N.GAIT_TROT, N.GAIT_CRAWL, N.GAIT_TROT_WITH_STAND, N.GAIT_STAND)


def params(name):
    p = N.LmpcParams()
    (N.lib().lmpc_params_go1 if name == "go1" else N.lib().lmpc_params_a1)(ctypes.byref(p))
    return p


def feet_of(name):
    if name == "go1":
        return SR.GO1_FEET
    a1 = N.LmpcSynthCfg()
    N.lib().lmpc_synth_cfg_a1_standing(ctypes.byref(a1))
    return np.array(a1.default_feet).reshape(4, 3)


def cfg_of(name):
    c = rollout.cfg_go1()
    c.default_feet[:] = list(feet_of(name).reshape(12))
    return c


def standing_state(yaw=0.0, x=0.0, y=0.0, z=0.30):
    s = np.zeros(36)
    s[0], s[3], s[4], s[5] = yaw, x, y, z
    s[6:18] = np.tile([0.0, 0.8, -1.6], 4)
    return s


def sim_out(foot_pos, touch):
    o = N.LmpcSimOut()
    o.foot_pos[:] = [float(v) for v in np.asarray(foot_pos).reshape(12)]
    o.touch[:] = [int(v) for v in touch]
    return o


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def compare(rb, ref, dt):
    """One host robot against the restatement after the same advance -> (worst relative position-like deviation,
    worst absolute velocity-target deviation); the discrete fields are asserted bit for bit."""
    c, st = rb.rb.cmd, rb.rb.cmd.state
    assert list(c.plan_contacts) == [int(v) for v in ref.contacts]
    assert list(rb.rb.fsm_index) == [f.idx for f in ref.fsm]
    assert [bool(v) for v in rb.not_first_call] == [f.not_first_call for f in ref.fsm]
    assert rb.rb.tick == ref.tick
    pos = max(rel(list(st.root_euler) + list(st.root_pos) + list(st.root_ang_vel) + list(st.root_lin_vel), ref.x),
              rel(st.root_rot_mat, ref.R.reshape(9)), rel(st.foot_pos_abs, ref.foot_abs.reshape(12)),
              rel(st.root_euler_d, ref.euler_d), rel(rb.rb.foot_pos_world, ref.foot_world.reshape(12)),
              rel(c.gait_phase, [f.phase for f in ref.fsm]), rel(rb.rb.fsm_start, [f.start for f in ref.fsm]),
              rel(rb.fsm_pos_target, np.concatenate([f.pos_target for f in ref.fsm])))
    for j, f in enumerate(ref.fsm):  # the reference leaves the swing start / end unset until an FSM's first update
        if f.not_first_call:
            pos = max(pos, rel(rb.rb.swing_start_world[3 * j:3 * j + 3], f.swing_start),
                      rel(rb.swing_end_world[3 * j:3 * j + 3], f.swing_end))
    vel = float(np.max(np.abs(np.array(rb.fsm_vel_target) - np.concatenate([f.vel_target for f in ref.fsm]))))
    return pos, vel


def test_binding():
    L = N.lib()
    assert L.lmpc_stack_abi_version() == N.STACK_ABI_VERSION == 1
    assert L.lmpc_stack_robot_size() == ctypes.sizeof(N.LmpcStackRobot) == stack.ROBOT_BYTES == 960
    assert stack.STACK_ROBOT_DTYPE.itemsize == 960
    for f in ("fsm_pos_target", "fsm_vel_target", "swing_end_world", "not_first_call"):
        assert getattr(N.LmpcStackRobot, f).offset == stack.STACK_ROBOT_DTYPE.fields[f][1]
    src = open(os.path.join(ROOT, "include", "lmpc", "lmpc_stack.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(lmpc_stack_[a-z0-9_]+)\s*\(", src)))
    assert decl == sorted(N.STACK_SYMBOLS)
    for name in decl:
        assert hasattr(L, name), name


@pytest.mark.parametrize("name", ["go1", "a1"])
@pytest.mark.parametrize("gait", GAITS + ("stand_after_trot",))
def test_host_tick_matches_reference(name, gait):
    """TICKS ticks on synthetic feedback (a smooth random state and foot trajectory, touch drawn with p = 0.5)."""
    p, cfg, model, feet = params(name), cfg_of(name), preset(name), feet_of(name)
    switch = gait == "stand_after_trot"  # the reset's SWING branch: trot for a while, then movement mode 0
    g = N.GAIT_TROT if switch else gait
    rng = np.random.default_rng(1000 + 17 * GAITS.index(g) + (name == "a1") + 7 * switch)
    s0 = standing_state(yaw=0.4, x=0.3, y=-0.2)
    states, fpos, touch = SR.synthetic_feedback(rng, TICKS, s0)
    st0 = rbd.state_from_vector(s0)
    rb, first = stack.robot_init(cfg, model, st0, (0.4, -0.1), 0.3, 0.29, g, SPEED)
    ref = SR.StackRef(s0, (0.4, -0.1), 0.3, 0.29, g, SPEED, feet=feet)
    worst_p = worst_v = 0.0
    for t in range(TICKS):
        if switch and t == 57:
            rb.rb.cmd.gait = N.GAIT_STAND
            ref.gait = F.STAND
        tgt = stack.advance(p, cfg, rb, rbd.state_from_vector(states[t]), sim_out(fpos[t], touch[t]))
        ref.advance(states[t], fpos[t], touch[t], DT)
        assert rel(tgt, ref.target) <= TOL
        dp, dv = compare(rb, ref, DT)
        worst_p, worst_v = max(worst_p, dp), max(worst_v, dv)
    early, timed = sum(f.early for f in ref.fsm), sum(f.timed_out for f in ref.fsm)
    print(f"{name} gait {gait}: positions {worst_p:.2e}, velocity targets {worst_v:.2e} (bound {2e-13 / DT:.1e}); "
          f"{early} early touchdowns, {timed} timed-out swings")
    assert worst_p <= TOL
    assert worst_v <= 2e-13 / DT
    if g != N.GAIT_STAND and not switch:
        assert early >= 1 and timed >= 1
        ph = np.array([f.phase for f in ref.fsm])
        assert np.ptp(ph) > 0.0  # the legs' phases have come apart


def swing_robot(percent, speed=4.0):
    """A Go1 trot robot whose FL leg is in SWING and will be at `percent` of it after the next advance."""
    cfg, model = cfg_of("go1"), preset("go1")
    s = standing_state()
    rb, out = stack.robot_init(cfg, model, rbd.state_from_vector(s), (0.0, 0.0), 0.0, 0.30, N.GAIT_TROT, speed)
    rb.rb.cmd.plan_contacts[0] = 0
    rb.rb.fsm_index[0] = 1          # trot, FL: [STANCE until 0.5, SWING until 1.0]
    rb.rb.fsm_start[0] = 0.5
    rb.rb.cmd.gait_phase[0] = 0.5 + percent * 0.5 - speed * DT
    rb.not_first_call[0] = 1
    rb.rb.swing_start_world[0:3] = [0.1, 0.1, 0.0]
    rb.fsm_pos_target[0:3] = [0.15, 0.12, 0.05]
    return cfg, s, rb, out


def test_early_touchdown_at_95_percent():
    cfg, s, rb, out = swing_robot(0.95)
    meas = np.array(out.foot_pos)
    meas[0:3] = [0.21, 0.13, 0.004]
    stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s), sim_out(meas, (1, 0, 0, 0)))
    assert rb.rb.cmd.plan_contacts[0] == 1
    assert list(rb.fsm_pos_target[0:3]) == [0.21, 0.13, 0.004] and list(rb.fsm_vel_target[0:3]) == [0.0, 0.0, 0.0]
    # the pattern index wrapped, so the phase wrapped by -1 and the state starts there
    assert rb.rb.fsm_index[0] == 0
    assert abs(rb.rb.cmd.gait_phase[0] - (0.975 - 1.0)) < 1e-15 and rb.rb.fsm_start[0] == rb.rb.cmd.gait_phase[0]
    # the other swing leg (FR starts the trot in SWING) saw no flag and swings on
    assert rb.rb.cmd.plan_contacts[1] == 0


def test_flag_before_90_percent_is_ignored():
    cfg, s, rb, out = swing_robot(0.85)
    prev = np.array(rb.fsm_pos_target[0:3])
    tgt = stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s), sim_out(out.foot_pos, (1, 1, 1, 1)))
    assert rb.rb.cmd.plan_contacts[0] == 0 and rb.rb.fsm_index[0] == 1
    want = SR.foot_curve(0.85, np.array([0.1, 0.1, 0.0]), tgt[0])
    assert rel(rb.fsm_pos_target[0:3], want) <= TOL
    assert np.max(np.abs(np.array(rb.fsm_vel_target[0:3]) - (want - prev) / DT)) <= 2e-13 / DT
    assert rel(rb.swing_end_world[0:3], tgt[0]) == 0.0


def test_swing_times_out_without_flag():
    cfg, s, rb, out = swing_robot(1.02)
    stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s), sim_out(out.foot_pos, (0, 0, 0, 0)))
    assert rb.rb.cmd.plan_contacts[0] == 1 and rb.rb.fsm_index[0] == 0
    assert list(rb.fsm_pos_target[0:3]) == list(out.foot_pos[0:3]) and list(rb.fsm_vel_target[0:3]) == [0.0] * 3


def test_first_call_sets_start_end_and_target():
    cfg, model = cfg_of("go1"), preset("go1")
    s = standing_state(yaw=0.3)
    rb, out = stack.robot_init(cfg, model, rbd.state_from_vector(s), (0.2, 0.0), 0.0, 0.30, N.GAIT_TROT, 4.0)
    assert list(rb.not_first_call) == [0, 0, 0, 0]
    meas = np.array(out.foot_pos) + 0.01
    tgt = stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s), sim_out(meas, out.touch))
    assert list(rb.not_first_call) == [1, 1, 1, 1]
    for leg in (0, 3):  # the stance legs: start = measured, end = target = the Raibert target, velocity 0
        k = slice(3 * leg, 3 * leg + 3)
        assert list(rb.rb.swing_start_world[k]) == list(meas[k])
        assert list(rb.swing_end_world[k]) == list(tgt[leg]) == list(rb.fsm_pos_target[k])
        assert list(rb.fsm_vel_target[k]) == [0.0, 0.0, 0.0]
    for leg in (1, 2):  # the legs that start in SWING: the first swing_update ran from those values
        k = slice(3 * leg, 3 * leg + 3)
        want = SR.foot_curve(4.0 * DT / 0.5, meas[k], tgt[leg])
        assert rel(rb.fsm_pos_target[k], want) <= TOL
        assert np.max(np.abs(np.array(rb.fsm_vel_target[k]) - (want - tgt[leg]) / DT)) <= 2e-13 / DT


def test_targets_is_a_pure_copy():
    cfg, s, rb, out = swing_robot(0.5)
    stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s), sim_out(out.foot_pos, out.touch))
    rng = np.random.default_rng(5)
    u0 = rng.normal(size=12) * 40.0
    tmpl = rbd.target(torque_limits=(21.0, 22.5, 30.25), mu=0.45, swing_kp=123.0, swing_kd=4.5, contact=(0, 0, 0, 0),
                      forces_des=np.full(12, 9.0), foot_pos_des=np.full(12, 8.0), foot_vel_des=np.full(12, 7.0))
    t = stack.targets(rb, u0, tmpl)
    assert list(t.forces_des) == list(u0)
    assert list(t.foot_pos_des) == list(rb.fsm_pos_target) and list(t.foot_vel_des) == list(rb.fsm_vel_target)
    assert list(t.contact) == [int(v) for v in rb.rb.cmd.plan_contacts] == [0, 0, 0, 1]
    assert list(t.torque_limits) == [21.0, 22.5, 30.25]
    assert (t.mu, t.swing_kp, t.swing_kd) == (0.45, 123.0, 4.5)
    assert bytes(stack.targets(rb, u0)) == bytes(stack.targets(rb, u0, rbd.target()))  # the default template


def test_feedback_mapping():
    cfg, model = cfg_of("go1"), preset("go1")
    s = standing_state()
    rb, out = stack.robot_init(cfg, model, rbd.state_from_vector(s), (0.0, 0.0), 0.0, 0.30, N.GAIT_STAND, 4.0)
    s2 = s.copy()
    s2[0:3] = [0.5, -0.2, 0.1]            # yaw, pitch, roll
    s2[3:6] = [1.0, 2.0, 0.31]
    s2[18:21] = [0.01, 0.02, 0.03]
    s2[21:24] = [0.4, 0.5, 0.6]
    meas = np.arange(12) * 0.1 + 0.05
    stack.advance(params("go1"), cfg, rb, rbd.state_from_vector(s2), sim_out(meas, (1, 1, 1, 1)))
    st = rb.rb.cmd.state
    assert list(st.root_euler) == [0.1, -0.2, 0.5]  # roll, pitch, yaw
    assert list(st.root_pos) == [1.0, 2.0, 0.31] and list(st.root_ang_vel) == [0.01, 0.02, 0.03]
    assert list(st.root_lin_vel) == [0.4, 0.5, 0.6]
    assert list(rb.rb.foot_pos_world) == list(meas)
    assert list(st.foot_pos_abs) == [meas[i] - s2[3 + i % 3] for i in range(12)]
    assert rel(st.root_rot_mat, SR.rot_zyx([0.1, -0.2, 0.5]).reshape(9)) <= TOL
    # movement mode 0: all planned in contact, the targets on the measured feet
    assert list(rb.rb.cmd.plan_contacts) == [1, 1, 1, 1] and list(rb.fsm_pos_target) == list(meas)
    assert list(rb.fsm_vel_target) == [0.0] * 12 and list(rb.not_first_call) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["go1", "a1"])
def test_robot_init_first_out(name):
    cfg, model, md = cfg_of(name), preset(name), model_json(name)
    s = standing_state(yaw=-0.8, x=0.4, y=0.1)
    s[1], s[2] = 0.05, -0.03
    s[5] -= np.min(RBD.terms(md, s)["foot_pos"][2::3])  # the lowest foot on the ground
    rb, out = stack.robot_init(cfg, model, rbd.state_from_vector(s), (0.3, 0.1), 0.2, 0.28, N.GAIT_TROT, 3.5)
    want = RBD.terms(md, s)["foot_pos"]
    assert rel(out.foot_pos, want) <= TOL
    on = [int(z <= 1e-9) for z in want[2::3]]
    assert 1 <= sum(on) < 4
    assert list(out.touch) == on and list(out.held) == on and out.status == 0
    assert list(out.qdd) == [0.0] * 18 and list(out.force) == [0.0] * 12
    st = rb.rb.cmd.state
    assert list(st.root_euler) == [s[2], s[1], s[0]] and list(st.root_euler_d) == [0.0, 0.0, s[0]]
    assert list(st.root_pos_d) == [0.0, 0.0, 0.28] and list(st.root_lin_vel_d_rel) == [0.3, 0.1, 0.0]
    assert st.root_ang_vel_d_rel[2] == 0.2 and rb.rb.cmd.gait_speed == 3.5 and rb.rb.tick == 0
    assert list(rb.rb.cmd.plan_contacts) == [1, 0, 0, 1] and list(rb.rb.cmd.gait_phase) == [0.0] * 4
    assert list(rb.rb.foot_pos_world) == list(out.foot_pos)


def test_argument_checks():
    L = N.lib()
    cfg, model, p = cfg_of("go1"), preset("go1"), params("go1")
    st = rbd.state_from_vector(standing_state())
    rb, out = N.LmpcStackRobot(), N.LmpcSimOut()
    vd = (ctypes.c_double * 2)(0.0, 0.0)
    r = ctypes.byref
    good = [r(cfg), r(model), r(st), vd, 0.0, 0.3, N.GAIT_TROT, 4.0, r(rb), r(out)]
    assert L.lmpc_stack_robot_init(*good) == 0
    for i in (0, 1, 2, 3, 8, 9):
        bad = list(good)
        bad[i] = None
        assert L.lmpc_stack_robot_init(*bad) == -1
    for i, v in ((6, -1), (6, 4), (7, 0.0)):
        bad = list(good)
        bad[i] = v
        assert L.lmpc_stack_robot_init(*bad) == -1
    good = [r(p), r(cfg), r(rb), r(st), r(out), None]
    assert L.lmpc_stack_advance(*good) == 0
    for i in range(5):
        bad = list(good)
        bad[i] = None
        assert L.lmpc_stack_advance(*bad) == -1
    u0 = (ctypes.c_double * 12)()
    tm, t = rbd.target(), N.LmpcWbcTarget()
    good = [r(rb), u0, r(tm), r(t)]
    assert L.lmpc_stack_targets(*good) == 0
    for i in range(4):
        bad = list(good)
        bad[i] = None
        assert L.lmpc_stack_targets(*bad) == -1
    # the device entry points reject NULL and negative counts before they touch a device
    assert L.lmpc_stack_advance_device(None, r(cfg), None, None, None, 1, None) == -1
    assert L.lmpc_stack_reserve(None, 1) == -1
    assert L.lmpc_stack_solve_device(None, 1, None, None, None, None) == -1
    assert L.lmpc_stack_copy_records_device(None, 1, None, None, None) == -1
    assert L.lmpc_stack_targets_device(None, None, 12, r(tm), 1, None, None) == -1
    assert L.lmpc_stack_targets_device(None, None, 12, r(tm), -1, None, None) == -1
    assert L.lmpc_stack_targets_device(None, None, 12, r(tm), 0, None, None) == 0
    assert L.lmpc_stack_candidates_device(None, 1, None, None) == -1
    assert L.lmpc_stack_candidates_device(None, -1, None, None) == -1
    assert L.lmpc_stack_candidates_device(None, 0, None, None) == 0


def test_rates_must_agree():
    L = N.lib()
    p = params("go1")  # dt = 0.01
    ok = sim.cfg(dt=0.00125)
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 8, 1) == 0
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 4, 2) == 0
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(sim.cfg(dt=0.005)), 2, 1) == 0
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 7, 1) == -1
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 8, 2) == -1
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(sim.cfg(dt=0.00125 + 1e-9)), 8, 1) == -1
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 0, 1) == -1
    assert L.lmpc_stack_check_rates(ctypes.byref(p), ctypes.byref(ok), 8, 0) == -1
    assert L.lmpc_stack_check_rates(None, ctypes.byref(ok), 8, 1) == -1
    stack.check_rates(p, ok, 8)
    with pytest.raises(ValueError):
        stack.check_rates(p, ok, 7)
    with pytest.raises(ValueError):
        stack.check_rates(p, sim.cfg(dt=0.002), 4)
