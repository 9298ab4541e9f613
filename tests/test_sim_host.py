"""CPU tests of the rigid-body plant (include/lmpc/lmpc_sim.h): the host functions against the independent NumPy
reference tests/sim_ref.py (dense KKT matrix from rbd_ref's terms, LU), invariants on the reference's terms, the
inelastic touchdown, substeps, struct sizes, argument checks, status 1, and the shared header under the host
compiler's sanitizers.

Cases.  Per robot (Go1, A1) 16 states in the style of test_rbd_host.make_states, the joints uniformly inside the URDF
limits; each with all 16 contact patterns, unilateral on and off: 512 forward dynamics and 512 steps per robot.

Tolerance.  MEASURED below is the host's largest deviation from sim_ref over exactly these cases, per field, relative
to max(1, |ref|); every assertion allows ten times that figure.  Both sides solve the same linear system in fp64 from
terms that agree to 1e-14 (test_rbd_host.py); cond(M) <= 4.6e3 and the accelerations reach a few thousand rad/s^2, so
figures of 1e-12 are rounding (the step's qdd = (v+ - v) / dt carries v's 8.5e-14 times 1 / dt), and anything above 1e-9
would be a defect.  held, touch, status and the zeros of
released feet are compared bit for bit.

Tie condition.  A case is compared only if no pass of the reference's unilateral rule has a normal component with
|.| < 1e-6 m g; the seeds are chosen so that every case meets this, and the test fails (not skips) if one does not.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import rbd_ref as R
import sim_ref as S
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import rbd, sim
from legged_mpc_control_amd import wbc as W
from test_rbd_host import model_json, preset

# measured on these cases (python -m pytest tests/test_sim_host.py -s prints the figures of the run)
MEASURED = {"fd_qdd": 2.0e-12, "fd_force": 7.4e-14, "fd_eom": 9.1e-15, "fd_con": 2.7e-14,
            "qdd": 8.7e-12, "force": 5.3e-13, "q": 2.2e-16, "v": 8.5e-14, "omega": 3.0e-14, "foot_pos": 4.4e-16,
            "foot_vel": 1.1e-14, "con": 2.3e-15,
            # the two five-pass cases (faster joints and larger torques than the cases above)
            "five_fd_qdd": 1.3e-14, "five_qdd": 2.2e-14, "five_next": 2.7e-15}
TOL = {k: 10.0 * v for k, v in MEASURED.items()}
ROBOTS = ("go1", "a1")
N_STATES = 16
DT = 0.002
PATTERNS = [tuple((p >> l) & 1 for l in range(4)) for p in range(16)]
# |x_restatement - sim_ref| relative to max(1, |ref|) over test_gpu_rbd.e2e_cases: the yardstick of the GPU suite's WBC
# consistency test, recomputed by test_wbc_consistency_yardstick below
YARDSTICK_CPU = 8.61e-10  # measured 8.603e-10, rounded up
# Two Go1 cases, all feet candidates, whose rule releases one foot per pass until none is left (4 -> 3 -> 2 -> 1 -> 0:
# five reference passes, the last on the empty set): one for the forward dynamics, one for the step.  Found by a seed
# search over 1e6 - 1e7 random states (joints inside the limits, joint rates within 6 rad/s, torques within 15 N m)
# and checked against sim_ref below; every normal component of every pass is at least 0.3 N from zero.
FIVE_PASS_HEX = {
    "fd_state": """-0x1.080d153556406p+1 -0x1.1f5916efb2f75p+0 0x1.4d8099857b706p-1 0x1.8d1d76a96fce0p+0
        -0x1.07f9545d8d448p-2 -0x1.5af64b6ce9030p-3 0x1.171bc57824838p-3 0x1.d1b206775ec80p-3
        -0x1.23d9accddfb6fp+1 0x1.edc86369eb7dcp-1 0x1.a16ec8b0690bcp-2 -0x1.3521b93af8cdcp+1
        0x1.30c0bb495a224p-1 0x1.320d625745d36p+1 -0x1.7f1fbf7bbd2dcp+0 0x1.5e78faba2a35cp-2
        0x1.bb04b5fbd80c0p-5 -0x1.1b95418a5dfc3p+1 0x1.cdec8af2f37dap+0 0x1.40774858c856ep+0
        -0x1.36f83a6d038e0p-1 -0x1.8b396712a1fd4p-2 -0x1.063036dc8b6e2p-1 0x1.ebc3fe583b562p-1
        -0x1.2cc49ea6ae86fp+2 0x1.13b9f5e340084p+0 0x1.655dc4203354cp+0 0x1.4205d91c05098p+2
        -0x1.72ad3c92d872ap+2 0x1.bb8aa44461bc8p+1 0x1.3c671a658f5aep+2 -0x1.4b5548dd8e3f1p+1
        -0x1.4a5fc1edb80b6p+1 0x1.b7e02b1f37108p+0 0x1.3ac85aa98a418p-1 -0x1.031fe71d75542p+2""",
    "fd_tau": """-0x1.352d572329540p-2 -0x1.3b6ebe3da2070p+3 -0x1.a31bfdfe3b055p+3 -0x1.0c4a73eed518dp+3
        -0x1.9eed7b9ff5aaep+2 0x1.7b7a95b9aa6d0p+1 0x1.9838d681af9c0p+1 -0x1.aa36e46bd062cp+3
        -0x1.0a27e7aff0767p+3 0x1.22b7a9fe08b0ap+3 0x1.13d14518b1a50p-1 0x1.ba807bcc05b34p+2""",
    "step_state": """0x1.299fe56975471p+1 0x1.473832233b36ep-1 0x1.073f16e8a1598p-1 -0x1.c6968631c9400p-5
        -0x1.f6c027feeed70p+0 -0x1.75b888b5dde04p-1 -0x1.db050d9ca64d8p-3 0x1.1a18d7938a976p+1
        -0x1.cad088d06383ep+0 0x1.7cb2b135541b6p-1 0x1.42f8e5ef79c16p+1 -0x1.cd9feb8f93806p+0
        0x1.0743f4a2eb8dep+0 0x1.3f81facd315e6p+1 -0x1.4528702d4865cp+1 0x1.8a6b100c084f2p-1
        0x1.53ac6c8b893cep+1 -0x1.28bd12f4d316bp+1 -0x1.b8c8a8777aea6p+0 -0x1.406d2016fec42p+0
        -0x1.1aa15b6dead7ep+0 -0x1.8055f2f6632f8p-2 -0x1.5e3b1cf4442aep-1 -0x1.bd33c72d253c0p-4
        -0x1.5e0f35e469758p+2 -0x1.b8d9a2a4487f6p+1 0x1.77756410469d2p+2 0x1.1fc5392a9bf5cp+2
        0x1.32b22d5b96f10p-1 -0x1.47b5a75940c40p-1 -0x1.abfc7956f4360p-1 -0x1.67f5da232d730p-1
        0x1.1d2ef02cd9f18p+0 0x1.c317800b0db90p+1 0x1.2d8511dda4e46p+2 -0x1.e5510ac59e310p+0""",
    "step_tau": """-0x1.c75178ddc4cc2p+2 -0x1.01aef24e2b004p+2 0x1.ca49ddb6b25cep+3 -0x1.22738f8622258p+3
        0x1.b12eed719a1c0p+0 -0x1.7c6e0940fc594p+1 0x1.3b581a02a58d8p+2 0x1.bc0be4eba1598p+3
        -0x1.90002c832388cp+2 -0x1.5b6226d4a1820p+0 0x1.e3e4388049a00p-4 -0x1.9caaa8247f199p+3""",
}


def five_pass_case(level):
    """(state (36), tau (12)) of the five-pass case of `level` ("fd" or "step")."""
    return tuple(np.array([float.fromhex(x) for x in FIVE_PASS_HEX[f"{level}_{k}"].split()]) for k in ("state", "tau"))


def make_sim_states(md, seed, count=N_STATES):
    """Random states as test_rbd_host.make_states makes them (|pitch| <= 1.2, yaw over (-pi, pi], velocities of the
    size the controller sees), the joints uniformly inside the URDF limits; and random torques of a few N m."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(md["joint_lower"]), np.array(md["joint_upper"])
    states, taus = [], []
    for _ in range(count):
        euler = [rng.uniform(-np.pi, np.pi), rng.uniform(-1.2, 1.2), rng.uniform(-0.8, 0.8)]
        states.append(np.concatenate([euler, rng.uniform(-3.0, 3.0, 3), rng.uniform(lo, hi), rng.normal(0.0, 1.0, 3),
                                      rng.normal(0.0, 0.5, 3), rng.normal(0.0, 3.0, 12)]))
        taus.append(rng.normal(0.0, 5.0, 12))
    return states, taus


@pytest.fixture(scope="module")
def cases():
    """Per robot: states, torques and the reference's terms (computed once, shared, never modified)."""
    out = {}
    for r, name in enumerate(ROBOTS):
        md = model_json(name)
        states, taus = make_sim_states(md, 700 + r)
        out[name] = dict(md=md, model=preset(name), states=states, taus=taus, terms=[R.terms(md, s) for s in states],
                         weight=sum(md["mass"]) * md["gravity"])
    return out


def dev(a, ref):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(ref)) / np.maximum(1.0, np.abs(np.asarray(ref)))))


def rows_of(held):
    return [3 * l + i for l in range(4) if held[l] for i in range(3)]


def eom_residual(t, qdd, F, tau):
    """|M qdd + h - J' F - S' tau| relative to the largest term."""
    parts = [t["M"] @ qdd, t["nle"], t["J"].T @ F, np.concatenate([np.zeros(6), tau])]
    return float(np.max(np.abs(parts[0] + parts[1] - parts[2] - parts[3])) / max(np.max(np.abs(p)) for p in parts))


def vec(st):
    return np.frombuffer(bytes(st), dtype=np.float64)


@pytest.mark.parametrize("name", ROBOTS)
def test_forward_dynamics_matches_reference(cases, name):
    c = cases[name]
    worst = dict.fromkeys(("fd_qdd", "fd_force", "fd_eom", "fd_con"), 0.0)
    released = 0
    for s, tau, t in zip(c["states"], c["taus"], c["terms"]):
        st = rbd.state_from_vector(s)
        for contact in PATTERNS:
            for uni in (1, 0):
                ref = S.forward_dynamics(c["md"], s, tau, contact, uni, t)
                assert not S.tie(ref["normals"], c["weight"]), "a case on a tie: choose another seed"
                o = sim.out_dict(sim.forward_dynamics(c["model"], st, tau, contact, uni))
                assert o["status"] == 0
                assert np.array_equal(o["held"], ref["held"]) and np.array_equal(o["touch"], np.zeros(4))
                if not uni:
                    assert np.array_equal(o["held"], contact)
                released += int(np.sum(np.array(contact) - o["held"]))
                for l in range(4):
                    if not o["held"][l]:  # exactly 0.0, not merely small
                        assert np.array_equal(o["force"][3 * l:3 * l + 3], np.zeros(3))
                        assert not np.any(np.signbit(o["force"][3 * l:3 * l + 3]))
                    elif uni:
                        assert o["force"][3 * l + 2] >= 0.0
                assert np.array_equal(o["foot_pos"], rbd.terms_dict(rbd.compute(c["model"], st))["foot_pos"])
                worst["fd_qdd"] = max(worst["fd_qdd"], dev(o["qdd"], ref["qdd"]))
                worst["fd_force"] = max(worst["fd_force"], dev(o["force"], ref["force"]))
                worst["fd_eom"] = max(worst["fd_eom"], eom_residual(t, o["qdd"], o["force"], tau))
                rows = rows_of(o["held"])
                if rows:
                    con = t["J"][rows] @ o["qdd"] + t["dJv"][rows]
                    worst["fd_con"] = max(worst["fd_con"], dev(con, np.zeros(len(rows))) /
                                          max(1.0, float(np.max(np.abs(t["dJv"])))))
    print(f"{name}: forward dynamics, host vs sim_ref:", {k: f"{v:.1e}" for k, v in worst.items()},
          f"; feet released by the rule: {released}")
    assert released > 0, "the unilateral rule never released a foot: the cases do not exercise it"
    for k in worst:
        assert worst[k] <= TOL[k], f"{k}: {worst[k]:.2e} > {TOL[k]:.1e}"


@pytest.mark.parametrize("name", ROBOTS)
def test_step_matches_reference(cases, name):
    c = cases[name]
    worst = dict.fromkeys(("qdd", "force", "q", "v", "omega", "foot_pos", "foot_vel", "con"), 0.0)
    touched = set()
    for i, (s, tau, t) in enumerate(zip(c["states"], c["taus"], c["terms"])):
        st = rbd.state_from_vector(s)
        ground_z = float(np.median(t["foot_pos"][2::3]))  # some feet below it, some above
        for contact in PATTERNS:
            for uni in (1, 0):
                ref = S.step(c["md"], s, tau, contact, DT, ground_z, uni, t)
                assert not S.tie(ref["normals"], c["weight"]), "a case on a tie: choose another seed"
                assert np.min(np.abs(ref["foot_pos"][2::3] - ground_z)) > 1e-9, "a foot on the touch threshold"
                nxt, o = sim.step(c["model"], sim.cfg(dt=DT, ground_z=ground_z, unilateral=uni), st, tau, contact)
                o, n = sim.out_dict(o), vec(nxt)
                assert o["status"] == 0
                assert np.array_equal(o["held"], ref["held"]) and np.array_equal(o["touch"], ref["touch"])
                touched.update(int(x) for x in o["touch"])
                for l in range(4):
                    if not o["held"][l]:
                        assert np.array_equal(o["force"][3 * l:3 * l + 3], np.zeros(3))
                rn = ref["next"]
                worst["qdd"] = max(worst["qdd"], dev(o["qdd"], ref["qdd"]))
                worst["force"] = max(worst["force"], dev(o["force"], ref["force"]))  # P / dt
                worst["q"] = max(worst["q"], dev(n[0:18], rn[0:18]))                # euler+, pos+, joints+
                worst["v"] = max(worst["v"], dev(n[21:36], rn[21:36]))              # lin_vel+, joint_vel+
                worst["omega"] = max(worst["omega"], dev(n[18:21], rn[18:21]))
                worst["foot_pos"] = max(worst["foot_pos"], dev(o["foot_pos"], ref["foot_pos"]))
                worst["foot_vel"] = max(worst["foot_vel"], dev(o["foot_vel"], ref["foot_vel"]))
                # J_C v+ = 0 on the reference's J, with v+ rebuilt from the host's next state
                vp = np.concatenate([n[21:24], np.linalg.solve(R.euler_map(n[0:3]), n[18:21]), n[24:36]])
                rows = rows_of(o["held"])
                if rows:
                    drift = max(float(np.max(np.abs(t["J"][rows] @ vp))), float(np.max(np.abs(o["foot_vel"][rows]))))
                    worst["con"] = max(worst["con"], drift / max(1.0, float(np.max(np.abs(t["foot_vel"])))))
    print(f"{name}: step, host vs sim_ref:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert touched == {0, 1}
    for k in worst:
        assert worst[k] <= TOL[k], f"{k}: {worst[k]:.2e} > {TOL[k]:.1e}"


@pytest.mark.parametrize("name", ROBOTS)
def test_touchdown_dissipates(cases, name):
    """All feet candidates, trunk descending at 1 m/s, held bilaterally: v+ is the M-orthogonal projection of the
    unconstrained step's velocity onto J v = 0, so its kinetic energy cannot exceed that one's (exact up to rounding)."""
    c = cases[name]
    seen = 0
    for s, tau, t0 in zip(c["states"][:4], c["taus"], c["terms"]):
        s = s.copy()
        s[21:24] = [0.0, 0.0, -1.0]
        st = rbd.state_from_vector(s)
        M = R.terms(c["md"], s)["M"]
        ke = []
        for contact in ((1, 1, 1, 1), (0, 0, 0, 0)):
            nxt, o = sim.step(c["model"], sim.cfg(dt=DT, unilateral=0), st, tau, contact)
            assert o.status == 0 and list(o.held) == list(contact)
            n = vec(nxt)
            vp = np.concatenate([n[21:24], np.linalg.solve(R.euler_map(n[0:3]), n[18:21]), n[24:36]])
            ke.append(0.5 * vp @ M @ vp)
        print(f"{name}: kinetic energy after touchdown {ke[0]:.6f} J, unconstrained {ke[1]:.6f} J")
        assert ke[0] <= ke[1] * (1.0 + 1e-12)
        seen += ke[0] < 0.99 * ke[1]
    assert seen > 0  # the impact does take energy out


def test_five_passes_empty_the_set(cases):
    """The rule's longest run: four passes release one foot each, so the fourth leaves the empty set.  No foot may then
    carry a force and the result is the free body's, as the reference's fifth pass (on the empty set) gives it."""
    c = cases["go1"]
    worst = {}
    s, tau = five_pass_case("fd")
    ref = S.forward_dynamics(c["md"], s, tau, (1, 1, 1, 1), True)
    assert [len(p) for p in ref["normals"]] == [4, 3, 2, 1, 0] and not S.tie(ref["normals"], c["weight"])
    free = S.forward_dynamics(c["md"], s, tau, (0, 0, 0, 0), True, ref["terms"])
    assert np.array_equal(ref["qdd"], free["qdd"])
    o = sim.out_dict(sim.forward_dynamics(c["model"], rbd.state_from_vector(s), tau, (1, 1, 1, 1)))
    assert o["status"] == 0 and np.array_equal(o["held"], np.zeros(4))
    assert np.array_equal(o["force"], np.zeros(12)) and not np.any(np.signbit(o["force"]))
    assert bytes(sim.forward_dynamics(c["model"], rbd.state_from_vector(s), tau, (0, 0, 0, 0))) == \
        bytes(sim.forward_dynamics(c["model"], rbd.state_from_vector(s), tau, (1, 1, 1, 1)))
    worst["five_fd_qdd"] = dev(o["qdd"], ref["qdd"])
    s, tau = five_pass_case("step")
    ref = S.step(c["md"], s, tau, (1, 1, 1, 1), DT, 0.0, True)
    assert [len(p) for p in ref["normals"]] == [4, 3, 2, 1, 0] and not S.tie(ref["normals"], c["weight"])
    assert np.min(np.abs(ref["foot_pos"][2::3])) > 1e-9
    nxt, o = sim.step(c["model"], sim.cfg(dt=DT, ground_z=0.0), rbd.state_from_vector(s), tau, (1, 1, 1, 1))
    free_next, free_out = sim.step(c["model"], sim.cfg(dt=DT, ground_z=0.0), rbd.state_from_vector(s), tau, (0, 0, 0, 0))
    assert bytes(nxt) == bytes(free_next) and bytes(o) == bytes(free_out)
    o = sim.out_dict(o)
    assert o["status"] == 0 and np.array_equal(o["held"], np.zeros(4)) and np.array_equal(o["touch"], ref["touch"])
    assert np.array_equal(o["force"], np.zeros(12)) and not np.any(np.signbit(o["force"]))
    worst["five_qdd"] = dev(o["qdd"], ref["qdd"])
    worst["five_next"] = dev(vec(nxt), ref["next"])
    print("five passes, host vs sim_ref:", {k: f"{v:.1e}" for k, v in worst.items()})
    for k in worst:
        assert worst[k] <= TOL[k], f"{k}: {worst[k]:.2e} > {TOL[k]:.1e}"


def test_wbc_consistency_yardstick():
    """YARDSTICK_CPU, recomputed: the CPU restatement's x (oracle/hoqp.py) on the eight robots of
    test_gpu_rbd.e2e_cases, against sim_ref's forward dynamics with that x's tau and the targets' contact set.  The GPU
    suite asserts ten times the constant; this keeps the constant at or above what it stands for, and not far above."""
    from test_gpu_rbd import cpu_restatement, e2e_cases

    md, states, targets = e2e_cases()
    model = rbd.model_go1()
    worst = 0.0
    for s, t in zip(states, targets):
        rec = W.record_native(rbd.wbc_input_from_state(model, rbd.state_from_vector(s), rbd.target(**t)))
        xr, solved = cpu_restatement(rec)
        assert solved
        ref = S.forward_dynamics(md, s, xr[30:42], t["contact"], True)
        assert list(ref["held"]) == list(t["contact"])
        worst = max(worst, dev(xr[0:18], ref["qdd"]), dev(xr[18:30], ref["force"]))
    print(f"restatement's x vs sim_ref: {worst:.2e} (YARDSTICK_CPU {YARDSTICK_CPU:.1e})")
    assert 0.5 * YARDSTICK_CPU <= worst <= YARDSTICK_CPU


def test_substeps_equal_chained_calls(cases):
    """On the host `substeps` exists only in the binding: sim.step(substeps=3) is itself three lmpc_sim_step calls, so
    this checks no more than that the binding chains state and arguments correctly.  The substep loop proper is the
    kernel's, and tests/test_gpu_sim.py compares it with three launches and with these chained host steps."""
    c = cases["go1"]
    cf = sim.cfg(dt=DT, ground_z=-10.0)
    for s, tau, contact in zip(c["states"][:6], c["taus"], PATTERNS[9:]):
        st = rbd.state_from_vector(s)
        n3, o3 = sim.step(c["model"], cf, st, tau, contact, substeps=3)
        cur = st
        for _ in range(3):
            cur, o1 = sim.step(c["model"], cf, cur, tau, contact)
        assert bytes(n3) == bytes(cur) and bytes(o3) == bytes(o1)
        assert bytes(n3) != bytes(st)


def test_step_in_place(cases):
    """next_state may be the state itself."""
    c = cases["go1"]
    lib = N.lib()
    st = rbd.state_from_vector(c["states"][0])
    tau = (ctypes.c_double * 12)(*c["taus"][0])
    contact = (ctypes.c_int32 * 4)(1, 0, 1, 1)
    cf = sim.cfg()
    apart, o1, o2 = N.LmpcRbdState(), N.LmpcSimOut(), N.LmpcSimOut()
    assert lib.lmpc_sim_step(ctypes.byref(c["model"]), ctypes.byref(cf), ctypes.byref(st), tau, contact,
                             ctypes.byref(apart), ctypes.byref(o1)) == 0
    assert lib.lmpc_sim_step(ctypes.byref(c["model"]), ctypes.byref(cf), ctypes.byref(st), tau, contact,
                             ctypes.byref(st), ctypes.byref(o2)) == 0
    assert bytes(st) == bytes(apart) and bytes(o1) == bytes(o2)


def test_sizes_symbols_and_defaults():
    lib = N.lib()
    assert lib.lmpc_sim_abi_version() == N.SIM_ABI_VERSION == 1
    assert lib.lmpc_rbd_abi_version() == 1  # lmpc_rbd.h stays at its version
    assert (lib.lmpc_sim_cfg_size(), lib.lmpc_sim_out_size()) == (sim.CFG_BYTES, sim.OUT_BYTES) == (24, 472)
    assert ctypes.sizeof(N.LmpcSimCfg) == 24 and ctypes.sizeof(N.LmpcSimOut) == 472
    assert N.LmpcSimOut.held.offset == 432 and N.LmpcSimOut.status.offset == 464
    assert sim.CONTACT_OFFSET * 4 == N.LmpcWbcTarget.contact.offset == 336
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmpc", "lmpc_sim.h")).read(), flags=re.S)
    assert sorted(N.SIM_SYMBOLS) == sorted(set(re.findall(r"\b(lmpc_[a-z0-9_]+)\s*\(", src)))
    for sym in N.SIM_SYMBOLS:
        assert hasattr(lib, sym)
    cf = sim.cfg()
    assert (cf.dt, cf.ground_z, cf.unilateral, cf.reserved) == (0.002, 0.0, 1, 0)
    assert lib.lmpc_sim_work_bytes(4096) == 0 and lib.lmpc_sim_work_bytes(-1) == 0
    # the shared header stays free of the HIP runtime
    text = open(os.path.join(ROOT, "legged_mpc_control_amd", "csrc", "lmpc_sim_common.h")).read()
    assert "hip_runtime" not in text and "hipLaunch" not in text


def test_argument_errors():
    lib = N.lib()
    m, s, cf, o, n = rbd.model_go1(), rbd.state_from_vector(np.zeros(36)), sim.cfg(), N.LmpcSimOut(), N.LmpcRbdState()
    tau, contact = (ctypes.c_double * 12)(), (ctypes.c_int32 * 4)(1, 1, 1, 1)
    ERR_ARG = lib.lmpc_wbc_tasks(None, None)
    assert ERR_ARG != 0
    R_ = ctypes.byref
    assert lib.lmpc_rbd_forward_dynamics(None, R_(s), tau, contact, 1, R_(o)) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics(R_(m), None, tau, contact, 1, R_(o)) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics(R_(m), R_(s), None, contact, 1, R_(o)) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics(R_(m), R_(s), tau, None, 1, R_(o)) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics(R_(m), R_(s), tau, contact, 1, None) == ERR_ARG
    assert lib.lmpc_sim_step(R_(m), None, R_(s), tau, contact, R_(n), R_(o)) == ERR_ARG
    assert lib.lmpc_sim_step(R_(m), R_(cf), R_(s), tau, contact, None, R_(o)) == ERR_ARG
    assert lib.lmpc_sim_step(R_(m), R_(cf), R_(s), tau, contact, R_(n), None) == ERR_ARG
    for dt in (0.0, -0.002, float("nan"), float("inf")):
        assert lib.lmpc_sim_step(R_(m), R_(sim.cfg(dt=dt)), R_(s), tau, contact, R_(n), R_(o)) == ERR_ARG
    assert lib.lmpc_sim_step(R_(m), R_(cf), R_(s), tau, contact, R_(n), R_(o)) == 0
    # the device entry points check their arguments before touching the device
    assert lib.lmpc_rbd_forward_dynamics_device(R_(m), None, None, 12, None, 4, 0, 1, None, None) == 0
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), None, None, 12, None, 4, 0, 1, None, None, None, 0, None) == 0
    assert lib.lmpc_rbd_forward_dynamics_device(R_(m), None, None, 12, None, 4, 3, 1, None, None) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics_device(R_(m), None, None, 12, None, 4, -1, 1, None, None) == ERR_ARG
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), None, None, 12, None, 4, 3, 1, None, None, None, 0, None) == ERR_ARG
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), None, None, 12, None, 4, -1, 1, None, None, None, 0, None) == ERR_ARG
    # strides, substeps and dt are checked too (dummy non-NULL pointers: refused before any launch)
    p = ctypes.c_void_p(ctypes.addressof(o))
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), p, p, 11, p, 4, 1, 1, p, p, None, 0, None) == ERR_ARG
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), p, p, 12, p, 3, 1, 1, p, p, None, 0, None) == ERR_ARG
    assert lib.lmpc_sim_step_device(R_(m), R_(cf), p, p, 12, p, 4, 1, 0, p, p, None, 0, None) == ERR_ARG
    assert lib.lmpc_sim_step_device(R_(m), R_(sim.cfg(dt=0.0)), p, p, 12, p, 4, 1, 1, p, p, None, 0, None) == ERR_ARG
    assert lib.lmpc_rbd_forward_dynamics_device(R_(m), p, p, 11, p, 4, 1, 1, p, None) == ERR_ARG
    with pytest.raises(ValueError):
        sim.step(m, cf, s, np.zeros(12), (1, 1, 1, 1), substeps=0)


def test_status_one_on_singular_configuration():
    """A degenerate model, through the host functions only: zero-length legs on coincident hips give two held feet
    identical Jacobian rows, J_C M^-1 J_C' is singular (the leg's own 3 x 3 block of it is exactly zero)."""
    md = model_json("go1")
    md["joint_origin"] = [[0.0, 0.0, 0.0]] * 12
    md["foot"] = [[0.0, 0.0, 0.0]] * 4
    m = rbd.model_from_json(md)
    s = np.zeros(36)
    s[5] = 0.3
    s[21:] = np.linspace(-0.4, 0.4, 15)
    t = R.terms(md, s)
    assert np.array_equal(t["J"][0:3], t["J"][3:6])
    st = rbd.state_from_vector(s)
    tau = np.linspace(-1.0, 1.0, 12)
    for uni in (0, 1):
        o = sim.forward_dynamics(m, st, tau, (1, 1, 0, 0), uni)
        assert o.status == 1
        blank = N.LmpcSimOut()
        blank.status = 1
        assert bytes(o) == bytes(blank)
        nxt, o = sim.step(m, sim.cfg(unilateral=uni), st, tau, (1, 1, 0, 0))
        assert o.status == 1 and bytes(o) == bytes(blank) and bytes(nxt) == bytes(st)
    # the same model with no foot held is an ordinary free-falling body
    nxt, o = sim.step(m, sim.cfg(), st, tau, (0, 0, 0, 0))
    assert o.status == 0 and bytes(nxt) != bytes(st)


def test_shared_header_under_sanitizers():
    """tests/cpp/sim_host_check.cpp includes csrc/lmpc_sim_common.h and steps a few robots; built by the host compiler
    with -fsanitize=address,undefined and run directly (nothing loaded into Python is instrumented)."""
    from legged_mpc_control_amd import build as B

    exe = B.build_cpp_sim_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sim_host_check ok" in r.stdout and "runtime error" not in r.stderr
