"""CPU tests of the joint-PD low-level controller and of the fused low-level loop's host side off the two presets: on
the controller settings of tests/model_sets.py (`ll_cfg`: 12 different kp, 12 different kd, three different torque
limits, a non-zero rho_opt, 20 different rho_fix numbers) and on its `limbs` robot, whose four legs all differ and whose
kinematics lmpc_leg_kin_from_model can still read.

Why.  Every lmpc_lowlevel_cfg of tests/test_lowlevel_host.py and tests/test_lowsim_host.py holds one kp, one kd, no
limit or one, rho_opt = 0 and four rho_fix rows that are one row up to signs.  The device kernels pick a lane's part of
the configuration with an opaque leg index (lmpc_ll::leg_cfg), the host loops over the legs: a transposed gain table,
leg 0's row on every lane, kd in kp's place, one limit for three joints, a dropped rho_opt or leg 0's lengths on every
leg pass every test there.  `test_defect_needs_the_new_cfg` shows that each of these mistakes (model_sets.LL_DEFECTS)
leaves the host's output on the Go1 cfg bit for bit as it is and moves it on the new cfg; tests/test_gpu_lowlevel_models.py
runs the kernels on the same pools.

Tolerances are tests/test_lowlevel_host.py's: host against the restatement 1e-12 relative to max(1, |ref|), flags bit for
bit, only cases whose every inverse-kinematics branch margin exceeds 1e-6, at most 5 % of the drawn cases dropped.
`lmpc_lowsim_run` against the explicit loop: bit for bit.

The singular hand case.  With q = (0, 0, 0) every sine and cosine is exact on any libm, and J = [[0, -(lt + b), -b],
[lt + b, 0, 0], [d, -a, -a]] with a = rho_opt[0], b = lc - rho_opt[2]: for a = 0 two rows are multiples of each other,
the elimination leaves an exactly zero 2 x 2 block and lmpc_ll::lu_solve3 divides by zero.  For a != 0 (the "skew" cfgs)
det J = -(lt + b) lt a: the same pose is regular there, and no pose is singular independently of libm (that needs
tan q2 = a / b).  So the straight-leg pose runs on all four legs in front of the "skew_limited" pool, where it is a
regular case whose torque depends on rho_opt, and in front of the "limbs" pool, where it is the division by zero.
"""
import functools

import numpy as np
import pytest

import lowlevel_ref as LR
import model_sets as MS
from conftest import rel_err
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import lowlevel as LL
from legged_mpc_control_amd import lowsim as LS
from legged_mpc_control_amd import rbd, sim
from test_lowlevel_host import FIELDS, MARGIN, TOL, cfg_for, draw_case, kept_cases, run_host
from test_lowsim_host import KINDS, SIM_DT, explicit_loop, make_robots, same_ll

N_MOVING, N_STANDING = 259, 64  # kept cases of mode 1 and of mode 0 per cfg (the GPU module's largest batch is 259)
SEED = 51907
LOWSIM_SEED = 7411
LOWSIM_COUNT, BILATERAL_COUNT = 67, 17
LEGS = ("FL", "FR", "RL", "RR")


# ---- the controller's pools ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pools():
    """{kind: dict(cfg, ref_cfg, cases {mode: [...]}, refs {mode: [...]}, drawn {mode: n})}: seeded cases by
    test_lowlevel_host.draw_case whose restatement keeps every branch margin above MARGIN, computed once
    (tests/test_gpu_lowlevel_models.py draws its batches from them)."""
    out = {}
    for ki, kind in enumerate(MS.LL_KINDS):
        c = MS.ll_cfg(kind)
        ref_cfg = LR.cfg_dict(c)
        p = dict(cfg=c, ref_cfg=ref_cfg, cases={}, refs={}, drawn={})
        for mode, want in ((1, N_MOVING), (0, N_STANDING)):
            rng = np.random.default_rng(SEED + 10 * ki + mode)
            cases, refs, drawn = [], [], 0
            while len(cases) < want:
                drawn += 1
                assert drawn <= 2 * want, "the restatement drops too many cases"
                case = draw_case(rng, ref_cfg)
                ref = LR.lowlevel(ref_cfg, case["state"], case["forces"], case["pos_des"], case["vel_des"], mode)
                if mode == 1 and not ref["margin"] > MARGIN:
                    continue
                cases.append(case)
                refs.append(ref)
            p["cases"][mode], p["refs"][mode], p["drawn"][mode] = cases, refs, drawn
        out[kind] = p
    return out


def reference(p, case, mode):
    return LR.lowlevel(p["ref_cfg"], case["state"], case["forces"], case["pos_des"], case["vel_des"], mode)


@functools.lru_cache(maxsize=None)
def hand_cases(kind):
    """[(tag, case)] of mode 1, once for each of the four legs, on the kind's cfg: "far" (a target 1 m from the hip,
    outwards and down: IK_NAN), "nan_force" (TAU_NONFINITE) and "straight" (the leg's joints at exactly 0 with a
    non-zero v_rel: the division by zero where rho_opt[0] == 0, see the module's docstring).  The other legs keep a kept
    case's well-separated inputs."""
    p = pools()[kind]
    out = []
    for l in range(4):
        base = p["cases"][1][l]
        rf = p["ref_cfg"]["rho_fix"][l]
        far = dict(base, pos_des=base["pos_des"].copy())
        hip = np.array([rf[0], rf[1], 0.0])
        far["pos_des"][3 * l:3 * l + 3] = LR.rot(base["state"][0:3]) @ (hip + [0.0, 0.6 * np.sign(rf[1]), -0.8]) + \
            base["state"][3:6]
        nanf = dict(base, forces=base["forces"].copy())
        nanf["forces"][3 * l + 1] = np.nan
        straight = dict(base, state=base["state"].copy(), pos_des=base["pos_des"].copy())
        straight["state"][6 + 3 * l:9 + 3 * l] = 0.0
        # a target well inside the leg's reach (a straight leg is on its edge) and away from the branch boundaries
        q_t = np.array([0.2 * np.sign(rf[1]), 0.6, -1.2])
        straight["pos_des"][3 * l:3 * l + 3] = LR.rot(base["state"][0:3]) @ LR.fk(rf, p["ref_cfg"]["rho_opt"][l], q_t) + \
            base["state"][3:6]
        out += [(f"far_{LEGS[l]}", far), (f"nan_force_{LEGS[l]}", nanf), (f"straight_{LEGS[l]}", straight)]
    return out


def deviation(o, ref):
    """A host struct against the restatement's dict: flags bit for bit, NaNs by position -> the worst deviation of the
    doubles per field."""
    assert list(o.flags) == [int(f) for f in ref["flags"]]
    worst = {}
    for f in FIELDS:
        got, want = np.array(getattr(o, f)), np.asarray(ref[f])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f
        worst[f] = rel_err(got[~nan], want[~nan]) if (~nan).any() else 0.0
    return worst


# ---- the inputs are what they say -------------------------------------------------------------------------------------
def test_settings_are_what_they_say():
    md = MS.check_limbs(MS.model("limbs"))
    assert md["gravity"] == 9.7 and md["name"] == "limbs"
    kp, kd, ro = MS.LL_GAINS["kp"], MS.LL_GAINS["kd"], MS.LL_RHO_OPT
    assert sorted(kp.reshape(-1)) == list(np.linspace(0.5, 15.0, 12)) and sorted(kd.reshape(-1)) == list(np.linspace(0.2, 0.6, 12))
    assert len(set(MS.LL_LIMITS)) == 3 and MS.LL_LIMITS == (9.0, 14.0, 21.0)
    assert np.all((np.abs(ro) >= 0.005) & (np.abs(ro) <= 0.02))
    for kind in MS.LL_KINDS:
        c = LR.cfg_dict(MS.ll_cfg(kind))
        assert np.array_equal(c["kp"], kp) and np.array_equal(c["kd"], kd)
        assert list(c["tau_limit"]) == ([0.0] * 3 if kind == "skew" else list(MS.LL_LIMITS))
        rf = c["rho_fix"]
        for k in range(5):
            assert len(set(np.abs(rf[:, k]))) == 4
        assert np.all(rf[:, 3] != rf[:, 4])
        assert np.array_equal(rf[:, 1] > 0, [True, False, True, False])
        if kind == "limbs":
            assert np.all(c["rho_opt"] == 0.0)
            kin = LL.leg_kin_from_model(rbd.model_from_json(md))
            assert np.array_equal(rf, np.array([list(r) for r in kin.rho_fix]))
        else:
            assert len(set(np.abs(rf).reshape(-1))) == 20
            assert np.array_equal(c["rho_opt"], ro)
            assert np.array_equal(np.sign(ro[:, 1]), np.sign(rf[:, 2]))  # the sign rule
    # every defect changes the cfg it targets
    for name, (_, kind, _) in MS.LL_DEFECTS.items():
        c = MS.ll_cfg(kind)
        assert bytes(MS.ll_defective(c, name)) != bytes(c), name


# ---- host against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MS.LL_KINDS)
def test_host_matches_restatement(kind):
    p = pools()[kind]
    worst = {f: 0.0 for f in FIELDS}
    for mode, want in ((1, N_MOVING), (0, N_STANDING)):
        dropped = p["drawn"][mode] - want
        print(f"{kind} mode {mode}: {dropped} of {p['drawn'][mode]} drawn cases dropped")
        assert dropped <= 0.05 * p["drawn"][mode], f"{dropped} of {p['drawn'][mode]} drawn cases dropped"
        for case, ref in zip(p["cases"][mode], p["refs"][mode]):
            if mode == 1:
                assert ref["margin"] > MARGIN
            o = run_host(p["cfg"], case, mode)
            for f, v in deviation(o, ref).items():
                worst[f] = max(worst[f], v)
            assert all(fl & ~LL.CLAMPED == 0 for fl in o.flags)
    print(f"{kind}: host vs restatement " + ", ".join(f"{f} {v:.2e}" for f, v in worst.items()))
    assert max(worst.values()) <= TOL
    assert any(not np.array_equal(r["tau"], r["joint_tau_tgt"]) for r in p["refs"][1])


@pytest.mark.parametrize("kind", ("skew_limited", "limbs"))
def test_limits_bite_and_differ(kind):
    """On the restatement: between 20 % and 80 % of the torque components are clamped, each joint is clamped somewhere and
    left alone somewhere, and some clamped component would pass under another joint's limit."""
    p = pools()[kind]
    lim = np.tile(p["ref_cfg"]["tau_limit"], 4)
    clamped = np.zeros(3, dtype=int)
    free = np.zeros(3, dtype=int)
    tells = total = 0
    for mode in (1, 0):
        for case, ref in zip(p["cases"][mode], p["refs"][mode]):
            s = case["state"]
            kp, kd = p["ref_cfg"]["kp"].reshape(12), p["ref_cfg"]["kd"].reshape(12)
            pre = kp * (ref["joint_ang_tgt"] - s[6:18]) + kd * (ref["joint_vel_tgt"] - s[24:36]) + ref["joint_tau_tgt"]
            hit = np.abs(pre) > lim
            assert np.array_equal(np.abs(ref["tau"][hit]), lim[hit]) and np.array_equal(ref["tau"][~hit], pre[~hit])
            assert np.array_equal(ref["flags"] & LL.CLAMPED != 0, hit.reshape(4, 3).any(axis=1))
            clamped += hit.reshape(4, 3).sum(axis=0)
            free += (~hit).reshape(4, 3).sum(axis=0)
            total += 12
            for k in range(3):
                other = [MS.LL_LIMITS[j] for j in range(3) if j != k]
                tells += int(np.sum(hit.reshape(4, 3)[:, k] & (np.abs(pre.reshape(4, 3)[:, k]) <= max(other))))
    share = clamped.sum() / total
    print(f"{kind}: {100 * share:.1f} % of the torque components clamped; per joint clamped {list(clamped)}, left alone "
          f"{list(free)}; {tells} clamped components lie under another joint's limit")
    assert 0.2 <= share <= 0.8
    assert np.all(clamped >= 1) and np.all(free >= 1)
    assert tells >= 1


@pytest.mark.parametrize("kind", ("skew_limited", "limbs"))
def test_hand_cases(kind):
    p = pools()[kind]
    regular = kind == "skew_limited"
    for tag, case in hand_cases(kind):
        l = LEGS.index(tag.rsplit("_", 1)[1])
        ref = reference(p, case, 1)
        o = run_host(p["cfg"], case, 1)
        worst = deviation(o, ref)
        print(f"{kind} {tag}: flags {list(o.flags)}, host vs restatement " + ", ".join(f"{f} {v:.2e}" for f, v in worst.items()))
        assert max(worst.values()) <= TOL
        others = [i for i in range(4) if i != l]
        assert all(o.flags[i] & ~LL.CLAMPED == 0 for i in others)  # nothing leaks into another leg
        if tag.startswith("far"):
            assert o.flags[l] & LL.IK_NAN and np.isnan(ref["margin"])
            assert np.array(o.joint_ang_tgt[3 * l:3 * l + 3]).tobytes() == case["state"][6 + 3 * l:9 + 3 * l].tobytes()
        elif tag.startswith("nan_force"):
            assert o.flags[l] & LL.TAU_NONFINITE and not o.flags[l] & (LL.IK_NAN | LL.VEL_NAN)
            assert np.all(np.isnan(o.tau[3 * l:3 * l + 3]))
            assert np.all(np.isfinite(np.delete(np.array(o.tau), [3 * l, 3 * l + 1, 3 * l + 2])))
        else:
            assert ref["margin"] > MARGIN  # no inverse-kinematics branch is on a boundary
            J = LR.jac(p["ref_cfg"]["rho_fix"][l], p["ref_cfg"]["rho_opt"][l], np.zeros(3))
            if regular:  # rho_opt[0] != 0 keeps the straight leg regular, and the result depends on it
                assert abs(np.linalg.det(J)) > 1e-6 and not o.flags[l] & LL.VEL_NAN
            else:        # an exactly zero 2 x 2 block: the solve divides by zero, the rate target falls back
                assert J[1, 1] == J[1, 2] == J[2, 1] == J[2, 2] == 0.0
                assert o.flags[l] & LL.VEL_NAN
                assert np.array(o.joint_vel_tgt[3 * l:3 * l + 3]).tobytes() == case["state"][24 + 3 * l:27 + 3 * l].tobytes()


# ---- the defects ------------------------------------------------------------------------------------------------------
def host_answers(c, items):
    return [run_host(c, case, mode) for case, mode in items]


def moved(a, b):
    """The largest deviation between two lists of host outputs over every field (NaN positions must differ or agree; a
    flag that differs counts as moved)."""
    worst = 0.0
    for x, y in zip(a, b):
        if list(x.flags) != list(y.flags):
            return np.inf
        for f in FIELDS:
            u, v = np.array(getattr(x, f)), np.array(getattr(y, f))
            ok = ~(np.isnan(u) | np.isnan(v))
            worst = max(worst, rel_err(u[ok], v[ok]) if ok.any() else 0.0)
    return worst


@pytest.mark.parametrize("defect", tuple(MS.LL_DEFECTS))
def test_defect_needs_the_new_cfg(defect):
    """Each mistake leaves the Go1 cfg's answers bit for bit as they are and moves the targeted cfg's by more than
    1e3 TOL.  Leg 0's rho_fix magnitudes with each leg's own signs ARE Go1's rows, so that defect too is held to the bits
    there.  The exchange of the whole kp and kd tables is the one mistake the presets do show (their kp differs from
    their kd): that is asserted as it is, and it hides on a cfg whose kp equals its kd."""
    _, kind, hidden = MS.LL_DEFECTS[defect]
    go1 = cfg_for("go1")
    items = [(case, 1) for case in kept_cases()[("go1", 1)]["cases"]]
    good, bad = host_answers(go1, items), host_answers(MS.ll_defective(go1, defect), items)
    assert all(bytes(x) == bytes(y) for x, y in zip(good, bad)) == hidden, "the defect shows on the Go1 cfg"
    if not hidden:
        flat = LL.cfg_go1(rbd.model_go1(), kp=0.4, kd=0.4)
        good, bad = host_answers(flat, items), host_answers(MS.ll_defective(flat, defect), items)
        assert all(bytes(x) == bytes(y) for x, y in zip(good, bad))
    p = pools()[kind]
    items = [(case, 1) for case in p["cases"][1]] + [(case, 0) for case in p["cases"][0]]
    shift = moved(host_answers(p["cfg"], items), host_answers(MS.ll_defective(p["cfg"], defect), items))
    print(f"{defect}: moves the {kind} pool by {shift:.2e}")
    assert shift > 1e3 * TOL


# ---- the fused loop, host ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lowsim_setup(bilateral=False):
    """(model, joint-PD cfg, plant cfg) of the `limbs` sets: the plant's ground off zero; the second set bilateral."""
    return (rbd.model_from_json(MS.model("limbs")), MS.ll_cfg("limbs"),
            sim.cfg(dt=SIM_DT, ground_z=MS.SIM_GROUND_Z, unilateral=0 if bilateral else 1))


LEVEL = 0.25  # the hips' height over the feet in the crouch of the `limbs` sets [m]


def level_crouch():
    """The recipe's crouch (0, 0.8, -1.6) puts the feet of equal legs level; on `limbs` only the longest leg would reach
    the ground.  Here every leg folds as far as its own lengths ask: q2 = -2 q1 with (lt + lc) cos q1 = LEVEL, which is
    the recipe's pose on a leg of lt + lc = 0.359 m (Go1's is 0.426 m, A1's 0.4 m)."""
    rf = LR.cfg_dict(MS.ll_cfg("limbs"))["rho_fix"]
    q1 = np.arccos(LEVEL / (rf[:, 3] + rf[:, 4]))
    return tuple(np.stack([np.zeros(4), q1, -2.0 * q1], axis=1).reshape(12))


@functools.lru_cache(maxsize=None)
def lowsim_robots():
    """67 robots of test_lowsim_host's four kinds on the `limbs` model, crouching with level feet on ground_z =
    SIM_GROUND_Z; the bilateral set is the first 17.  The stance feet are sent 1.5 times the weight they carry: with the
    recipe's own forces no torque reaches LL_LIMITS (the largest is 17.0 N m, on a 21 N m joint) and no leg is clamped."""
    return make_robots(lowsim_setup()[0], LOWSIM_COUNT, LOWSIM_SEED, MS.SIM_GROUND_Z, push=1.5, crouch=level_crouch())


@functools.lru_cache(maxsize=None)
def lowsim_logs(ticks, substeps, count, bilateral=False):
    return [explicit_loop(lowsim_setup(bilateral), rb, ticks, substeps) for rb in lowsim_robots()[:count]]


def test_lowsim_input_conditions():
    """On the explicit loop's logs of the 8-tick sets (substeps 1): test_lowsim_host.test_input_conditions' three counts
    on the unilateral set, a clamped and an unclamped leg, and on the bilateral set a held foot that pulls."""
    robots = lowsim_robots()
    logs = lowsim_logs(8, 1, LOWSIM_COUNT)
    changed = released = touchdowns = clamped = unclamped = 0
    for rb, lg in zip(robots, logs):
        outs = [N.LmpcSimOut.from_buffer_copy(b) for b in lg["outs"]]
        cand = np.array(lg["candidates"])
        changed += int(np.any(cand[1:] != cand[:-1]))
        for k, o in enumerate(outs):
            assert o.status == 0
            released += sum(1 for l in range(4) if cand[k, l] == 1 and o.held[l] == 0)
            before = rb["out"] if k == 0 else outs[k - 1]
            touchdowns += sum(1 for l in range(4) if before.touch[l] == 0 and o.touch[l] == 1)
            flags = N.LmpcLowlevelOut.from_buffer_copy(lg["ll_outs"][k]).flags
            clamped += sum(1 for f in flags if f & LL.CLAMPED)
            unclamped += sum(1 for f in flags if not f & LL.CLAMPED)
    pulling = 0
    for lg in lowsim_logs(8, 1, BILATERAL_COUNT, True):
        for k, b in enumerate(lg["outs"]):
            o = N.LmpcSimOut.from_buffer_copy(b)
            assert o.status == 0 and list(o.held) == lg["candidates"][k]  # bilateral: every candidate is held
            pulling += sum(1 for l in range(4) if o.held[l] == 1 and o.force[3 * l + 2] < 0.0)
    print(f"limbs: {LOWSIM_COUNT} robots x 8 ticks: {changed} robots with a changing candidate word, {released} releases, "
          f"{touchdowns} touch-downs, {clamped} clamped legs, {unclamped} unclamped; bilateral, {BILATERAL_COUNT} robots: "
          f"{pulling} pulling feet")
    assert changed >= 1 and released >= 1 and touchdowns >= 1
    assert clamped >= 1 and unclamped >= 1
    assert pulling >= 1, "no held foot pulls: the set does not tell the bilateral path from the unilateral one"


@pytest.mark.parametrize("bilateral", [False, True])
@pytest.mark.parametrize("ticks", [1, 8])
@pytest.mark.parametrize("substeps", [1, 3])
def test_lowsim_run_matches_explicit_loop(bilateral, ticks, substeps):
    """All 67 robots (17 bilateral) for the 8-tick, one-substep set, the first 8 (every kind twice) otherwise."""
    full = BILATERAL_COUNT if bilateral else LOWSIM_COUNT
    count = full if (ticks, substeps) == (8, 1) else 8
    refs = lowsim_logs(ticks, substeps, count, bilateral)
    model, c, sc = lowsim_setup(bilateral)
    kinds = set()
    for b, (rb, ref) in enumerate(zip(lowsim_robots(), refs)):
        kinds.add(rb["kind"])
        state0, out0 = bytes(rb["state"]), bytes(rb["out"])
        r = LS.run(model, sc, c, rb["state"], rb["target"], rb["out"], ticks, substeps, rb["gait"], log=True)
        assert bytes(rb["state"]) == state0 and bytes(rb["out"]) == out0
        assert bytes(r["state"]) == ref["states"][-1] and bytes(r["sim_out"]) == ref["outs"][-1], b
        assert same_ll(bytes(r["ll_out"]), ref["ll_outs"][-1]) and list(r["candidates"]) == ref["candidates"][-1], b
        for k in range(ticks):
            assert bytes(r["states"][k]) == ref["states"][k], (b, k)
            assert bytes(r["outs"][k]) == ref["outs"][k], (b, k)
            assert same_ll(bytes(r["ll_outs"][k]), ref["ll_outs"][k]), (b, k)
        assert r["candidates_log"].tolist() == ref["candidates"], b
    assert kinds == set(KINDS)


def test_lowsim_settings_are_read():
    """The plant settings the fused kernel gets as loose scalars matter on these sets: with ground_z = 0 or with the
    other `unilateral` the explicit loop ends elsewhere."""
    model, c, sc = lowsim_setup()
    rbs = lowsim_robots()[:BILATERAL_COUNT]
    here = [lg["states"][-1] for lg in lowsim_logs(8, 1, BILATERAL_COUNT)]
    flat = [explicit_loop((model, c, sim.cfg(dt=SIM_DT, ground_z=0.0)), rb, 8, 1)["states"][-1] for rb in rbs]
    bil = [lg["states"][-1] for lg in lowsim_logs(8, 1, BILATERAL_COUNT, True)]
    assert any(a != b for a, b in zip(here, flat)) and any(a != b for a, b in zip(here, bil))
