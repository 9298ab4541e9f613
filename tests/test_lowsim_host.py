"""CPU tests of the fused low-level loop's host side (include/lmpc/lmpc_lowsim.h): `lmpc_lowsim_run` against the explicit
loop of the existing, separately tested host calls -- the candidate rule, `lmpc_lowlevel`, then `lmpc_sim_step`
`substeps` times -- bit for bit; its argument checks; the binding; and the stand-alone sanitizer program.

The robots (`robots()`, shared with tests/test_gpu_lowsim.py).  Go1 and A1 on their own models and gains, standing in a
crouch (joints near (0, 0.8, -1.6)) with the lowest foot 1 um below the ground, in four kinds by index:

  0  trot: FR and RL are sent 3 cm up (the PD pulls on feet the plant still holds), FL and RR carry the weight;
  1  drop: the robot starts 0.2 mm above the ground, sinking at 5 cm/s, no foot held: its feet touch down inside the run;
  2  stand: LMPC_GAIT_STAND (movement mode 0), the weight on four feet;
  3  trot with the other diagonal, perturbed joints and a sideways velocity.

`make_robots` is that recipe over a model, a seed and a ground height (tests/test_lowlevel_models_host.py builds the
`limbs` robot's sets with it); `explicit_loop` takes a preset's name or a (model, joint-PD cfg, plant cfg) triple.

`test_input_conditions` asserts on the explicit loop's own logs (not on the new code) that these inputs reach what the
fused kernel must get right: a candidate word that changes between two ticks, a foot released by the unilateral rule,
and a touch-down (touch 0 -> 1) inside the run.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import lowlevel as LL
from legged_mpc_control_amd import lowsim as LS
from legged_mpc_control_amd import rbd, sim
from test_lowlevel_host import cfg_for
from test_rbd_host import preset

SIM_DT = 0.00125  # the reference's low-level rate
SEED = 7311
COUNTS = {"go1": 67, "a1": 17}  # the largest batches of tests/test_gpu_lowsim.py
KINDS = ("trot", "drop", "stand", "trot2")


def sim_cfg():
    return sim.cfg(dt=SIM_DT, ground_z=0.0)


CROUCH = (0.0, 0.8, -1.6) * 4


def make_robots(model, count, seed, ground_z=0.0, lift=0.03, push=1.0, crouch=CROUCH):
    """`count` robots of `model` by the recipe above, the ground at `ground_z`: dicts of kind, state (LmpcRbdState),
    target (LmpcWbcTarget), gait (the gait word) and out (the lmpc_sim_out the first tick reads its candidates from:
    held = touch = the foot is on or below the ground).  lift: how far up the swing feet are sent [m]; push: the stance
    feet's forces_des as a multiple of the weight they carry; crouch: the 12 joint angles the robots stand near.  The
    joint-PD cfg is not read: the targets are the plant's
    own feet."""
    rng = np.random.default_rng(seed)
    weight = sum(model.mass) * model.gravity
    out = []
    for i in range(count):
        kind = KINDS[i % 4]
        s = np.zeros(36)
        s[0] = rng.uniform(-np.pi, np.pi)
        s[1:3] = rng.uniform(-0.02, 0.02, 2)
        s[3:5] = rng.uniform(-1.0, 1.0, 2)
        s[6:18] = np.array(crouch) + rng.uniform(-0.05, 0.05, 12) * (1.0 if kind == "trot2" else 0.2)
        feet = np.array(sim.forward_dynamics(model, rbd.state_from_vector(s), np.zeros(12), (0, 0, 0, 0), True).foot_pos)
        s[5] = ground_z - feet[2::3].min() + (2e-4 if kind == "drop" else -1e-6)
        if kind == "drop":
            s[23] = -0.05
        if kind == "trot2":
            s[22] = 0.1
        feet[2::3] += s[5]
        swing = {"trot": (1, 2), "trot2": (0, 3)}.get(kind, ())
        forces, pos_des = np.zeros(12), feet.copy()
        for l in range(4):
            if l in swing:
                pos_des[3 * l + 2] += lift
            else:
                forces[3 * l + 2] = push * weight / (4 - len(swing))
        t = rbd.target()
        t.forces_des[:] = [float(v) for v in forces]
        t.foot_pos_des[:] = [float(v) for v in pos_des]
        t.foot_vel_des[:] = [0.0] * 12
        o = N.LmpcSimOut()
        o.foot_pos[:] = [float(v) for v in feet]
        for l in range(4):
            o.held[l] = o.touch[l] = int(feet[3 * l + 2] <= ground_z)
        out.append(dict(kind=kind, state=rbd.state_from_vector(s), target=t, out=o,
                        gait=N.GAIT_STAND if kind == "stand" else N.GAIT_TROT))
    return out


@functools.lru_cache(maxsize=None)
def robots(name):
    """COUNTS[name] robots of the preset `name` on the ground z = 0."""
    return make_robots(preset(name), COUNTS[name], SEED + (0 if name == "go1" else 1))


def setup_for(name):
    """(model, joint-PD cfg, plant cfg) of a preset: what the loops below run a robot on."""
    return preset(name), cfg_for(name), sim_cfg()


def explicit_loop(name, rb, ticks, substeps):
    """The yardstick: per tick the candidates from the last lmpc_sim_out, lmpc_lowlevel, lmpc_sim_step `substeps` times.
    name: a preset's, or a (model, joint-PD cfg, plant cfg) triple.
    -> dict of per-tick lists (states, outs, ll_outs as bytes; candidates as lists)."""
    model, c, sc = setup_for(name) if isinstance(name, str) else name
    st, o = rb["state"], rb["out"]
    log = dict(states=[], outs=[], ll_outs=[], candidates=[])
    for _ in range(ticks):
        cand = [int(bool(o.held[l] | o.touch[l])) for l in range(4)]
        ll = LL.lowlevel(c, st, rb["target"], rb["gait"])
        st, o = sim.step(model, sc, st, list(ll.tau), cand, substeps)
        log["states"].append(bytes(st)), log["outs"].append(bytes(o)), log["ll_outs"].append(bytes(ll))
        log["candidates"].append(cand)
    return log


def same_ll(a: bytes, b: bytes) -> bool:
    """lmpc_lowlevel_out blocks: NaNs at the same places, every other bit equal."""
    x, y = np.frombuffer(a, dtype=np.float64, count=48), np.frombuffer(b, dtype=np.float64, count=48)
    nan = np.isnan(x)
    return np.array_equal(nan, np.isnan(y)) and x[~nan].tobytes() == y[~nan].tobytes() and a[384:] == b[384:]


@functools.lru_cache(maxsize=None)
def reference_logs(name, ticks, substeps, count):
    return [explicit_loop(name, rb, ticks, substeps) for rb in robots(name)[:count]]


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_binding():
    L = N.lib()
    assert L.lmpc_lowsim_abi_version() == N.LOWSIM_ABI_VERSION == 1
    assert L.lmpc_lowsim_block_robots() == 16
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmpc", "lmpc_lowsim.h")).read(), flags=re.S)
    assert sorted(N.LOWSIM_SYMBOLS) == sorted(set(re.findall(r"\b(lmpc_[a-z0-9_]+)\s*\(", src)))
    for sym in N.LOWSIM_SYMBOLS:
        assert hasattr(L, sym), sym
    assert ctypes.sizeof(N.LmpcLowsimLog) == 32
    # the shared host header stays free of the HIP runtime
    text = open(os.path.join(ROOT, "legged_mpc_control_amd", "csrc", "lmpc_lowsim_common.h")).read()
    assert "hip_runtime" not in text and "hipLaunch" not in text


# ---- the inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["go1", "a1"])
def test_input_conditions(name):
    """On the explicit loop's logs of the 8-tick set (substeps 1): some candidate word differs between two ticks, some
    candidate foot of a solved step is not held (released by the unilateral rule), some foot touches down."""
    count = COUNTS[name]
    logs = reference_logs(name, 8, 1, count)
    changed = released = touchdowns = 0
    for rb, lg in zip(robots(name), logs):
        outs = [N.LmpcSimOut.from_buffer_copy(b) for b in lg["outs"]]
        cand = np.array(lg["candidates"])
        changed += int(np.any(cand[1:] != cand[:-1]))
        for k, o in enumerate(outs):
            assert o.status == 0
            released += sum(1 for l in range(4) if cand[k, l] == 1 and o.held[l] == 0)
            before = rb["out"] if k == 0 else outs[k - 1]
            touchdowns += sum(1 for l in range(4) if before.touch[l] == 0 and o.touch[l] == 1)
    print(f"{name}: {count} robots x 8 ticks: {changed} robots with a changing candidate word, {released} releases, "
          f"{touchdowns} touch-downs")
    assert changed >= 1 and released >= 1 and touchdowns >= 1


# ---- lmpc_lowsim_run against the explicit loop -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["go1", "a1"])
@pytest.mark.parametrize("ticks", [1, 8])
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("log", [False, True])
def test_run_matches_explicit_loop(name, ticks, substeps, log):
    """Trot, drop and LMPC_GAIT_STAND robots (the first 8 of `robots`; all of them for the 8-tick, one-substep set)."""
    count = COUNTS[name] if (ticks, substeps) == (8, 1) else 8
    refs = reference_logs(name, ticks, substeps, count)
    model, c, sc = preset(name), cfg_for(name), sim_cfg()
    kinds = set()
    for b, (rb, ref) in enumerate(zip(robots(name), refs)):
        kinds.add(rb["kind"])
        state0, out0 = bytes(rb["state"]), bytes(rb["out"])
        r = LS.run(model, sc, c, rb["state"], rb["target"], rb["out"], ticks, substeps, rb["gait"], log=log)
        assert bytes(rb["state"]) == state0 and bytes(rb["out"]) == out0  # the inputs are not modified
        assert bytes(r["state"]) == ref["states"][-1], b
        assert bytes(r["sim_out"]) == ref["outs"][-1], b
        assert same_ll(bytes(r["ll_out"]), ref["ll_outs"][-1]), b
        assert list(r["candidates"]) == ref["candidates"][-1], b
        if log:
            for k in range(ticks):
                assert bytes(r["states"][k]) == ref["states"][k], (b, k)
                assert bytes(r["outs"][k]) == ref["outs"][k], (b, k)
                assert same_ll(bytes(r["ll_outs"][k]), ref["ll_outs"][k]), (b, k)
            assert r["candidates_log"].tolist() == ref["candidates"], b
    assert kinds == set(KINDS)


def test_failed_plant_step():
    """A NaN forces_des: the controller flags a non-finite torque, the plant fails on every tick, the state passes
    through and lmpc_sim_out is zero but for its status -- as the explicit loop leaves them."""
    name = "go1"
    rb = dict(robots(name)[0])
    t = N.LmpcWbcTarget.from_buffer_copy(bytes(rb["target"]))
    t.forces_des[4] = float("nan")
    rb["target"] = t
    ref = explicit_loop(name, rb, 3, 1)
    r = LS.run(preset(name), sim_cfg(), cfg_for(name), rb["state"], t, rb["out"], 3, 1, rb["gait"], log=True)
    for k in range(3):
        assert bytes(r["states"][k]) == ref["states"][k] == bytes(rb["state"])
        assert bytes(r["outs"][k]) == ref["outs"][k] and r["outs"][k].status == 1
        assert same_ll(bytes(r["ll_outs"][k]), ref["ll_outs"][k])
        assert r["ll_outs"][k].flags[1] & LL.TAU_NONFINITE
    assert r["candidates_log"].tolist() == ref["candidates"] and r["candidates_log"][2].tolist() == [0, 0, 0, 0]


def test_partial_log_and_chaining():
    name = "a1"
    rb = robots(name)[1]
    model, c, sc = preset(name), cfg_for(name), sim_cfg()
    full = LS.run(model, sc, c, rb["state"], rb["target"], rb["out"], 8, 1, rb["gait"], log=True)
    a = LS.run(model, sc, c, rb["state"], rb["target"], rb["out"], 3, 1, rb["gait"])
    b = LS.run(model, sc, c, a["state"], rb["target"], a["sim_out"], 5, 1, rb["gait"])
    for k in ("state", "sim_out", "ll_out"):
        assert bytes(b[k]) == bytes(full[k]), k
    assert list(b["candidates"]) == list(full["candidates"])
    # only the states logged: the C call with three NULL log pointers
    st = N.LmpcRbdState.from_buffer_copy(bytes(rb["state"]))
    so = N.LmpcSimOut.from_buffer_copy(bytes(rb["out"]))
    rows = (N.LmpcRbdState * 8)()
    lg = N.LmpcLowsimLog(ctypes.addressof(rows), None, None, None)
    cand, ll, g = (ctypes.c_int32 * 4)(), N.LmpcLowlevelOut(), ctypes.c_int32(rb["gait"])
    assert N.lib().lmpc_lowsim_run(ctypes.byref(model), ctypes.byref(sc), ctypes.byref(c), ctypes.byref(st),
                                   ctypes.byref(rb["target"]), ctypes.byref(g), ctypes.byref(so), cand, ctypes.byref(ll),
                                   8, 1, ctypes.byref(lg)) == 0
    assert bytes(rows) == bytes(full["states"]) and bytes(st) == bytes(full["state"])


def test_argument_checks():
    name = "go1"
    rb = robots(name)[0]
    model, c, sc = preset(name), cfg_for(name), sim_cfg()
    L, R_ = N.lib(), ctypes.byref
    st = N.LmpcRbdState.from_buffer_copy(bytes(rb["state"]))
    so = N.LmpcSimOut.from_buffer_copy(bytes(rb["out"]))
    cand, ll = (ctypes.c_int32 * 4)(7, 7, 7, 7), N.LmpcLowlevelOut()
    tg = rb["target"]

    def call(model_=R_(model), sc_=R_(sc), c_=R_(c), st_=R_(st), tg_=R_(tg), so_=R_(so), cand_=cand, ll_=R_(ll), ticks=2,
             substeps=1):
        return L.lmpc_lowsim_run(model_, sc_, c_, st_, tg_, None, so_, cand_, ll_, ticks, substeps, None)

    for kw in (dict(model_=None), dict(sc_=None), dict(c_=None), dict(st_=None), dict(tg_=None), dict(so_=None),
               dict(cand_=None), dict(ll_=None), dict(ticks=-1), dict(substeps=0), dict(substeps=-2)):
        assert call(**kw) == -1, kw
    for dt in (0.0, -1e-3, float("nan"), float("inf")):
        assert call(sc_=R_(sim.cfg(dt=dt))) == -1, dt
    assert bytes(st) == bytes(rb["state"]) and bytes(so) == bytes(rb["out"]) and list(cand) == [7, 7, 7, 7]
    # ticks == 0: LMPC_OK, nothing touched, nothing read
    assert L.lmpc_lowsim_run(None, None, None, None, None, None, None, None, None, 0, 0, None) == 0
    assert call(ticks=0) == 0 and bytes(st) == bytes(rb["state"]) and list(cand) == [7, 7, 7, 7]
    assert call() == 0 and bytes(st) != bytes(rb["state"])
    with pytest.raises(RuntimeError):
        LS.run(model, sc, c, rb["state"], tg, rb["out"], 2, 0)


def test_kernels_have_no_scratch():
    """lmpc_lowsim_kernel, both lmpc_sim_kernel instances and the contact kernels of the three-launch step (the bare solve
    and the step kernel's TERMS and APPLY instances, template arguments 1 and 2; the fused instance, argument 0, spills by
    design), cross-compiled with the product's flags: no scratch and no spilled VGPR.  They share one front and one back
    half of the plant step (lmpc_sim_device.h); the fused controller + plant kernel also owes it to a compiler option and
    two opaque indices (build.py).  A compiler upgrade that brings the spills back changes no result, so
    only this test would notice."""
    from legged_mpc_control_amd import build as B

    for source, pattern, count in (("lmpc_lowsim.hip", "lmpc_lowsim_kernel", 1), ("lmpc_sim.hip", "lmpc_sim_kernel", 2),
                                   ("lmpc_contact.hip", "lmpc_contact_solve_kernel", 1),
                                   ("lmpc_contact.hip", "lmpc_contact_step_kernelILi1E", 1),
                                   ("lmpc_contact.hip", "lmpc_contact_step_kernelILi2E", 1)):
        meta = {k: v for k, v in B.device_metadata(source).items() if pattern in k}
        assert len(meta) == count, (source, list(meta))
        for name, m in meta.items():
            print(f"{name[:60]}...: {m}")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_sanitizer_program():
    """tests/cpp/lowsim_host_check.cpp, built with -fsanitize=address,undefined, as a stand-alone program."""
    from legged_mpc_control_amd import build as B

    exe = B.build_cpp_lowsim_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lowsim_host_check ok" in r.stdout
