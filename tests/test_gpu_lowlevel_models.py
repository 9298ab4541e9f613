"""GPU tests of the joint-PD low-level kernel (lmpc_lowlevel.hip), of the fused low-level loop (lmpc_lowsim.hip) and of
`stack.StackLoop(..., low_level=cfg[, fused_low_level=True])` on the controller settings and the `limbs` robot of
tests/model_sets.py: the inputs of tests/test_lowlevel_models_host.py, which checks the host functions on them against
the NumPy restatement and shows, mistake by mistake, that the presets' configurations hide what these tell apart.

Why.  Both kernels pick a lane's part of lmpc_lowlevel_cfg with an opaque leg index (`lo` in lmpc_lowlevel_kernel, `lo`
re-derived every tick next to `L` in lmpc_lowsim_kernel), the fused kernel gets dt, ground_z and unilateral as loose
scalars and indexes the plant's model by lane.  On the presets every gain table holds one number, the limit is one number
or none, rho_opt is zero, the legs are mirror images, the ground is 0 and the plant unilateral: leg 0's gains or lengths
on every lane, a transposed table, tau_limit[0] for three joints, a dropped rho_opt, ground_z or `unilateral` change no
bit there.  Here they do: the device must agree with the host (1e-12) on cfgs where the host's answer moves by 1e-9 and
more under each of those mistakes, and the fused kernel must leave the unfused launches' bytes.

Inputs (once per module, from the host module's caches).
  * controller: "skew" and "skew_limited" at the batches 1, 5, 63, 64, 65 and 259 (64 robots per block), "limbs" at 65:
    kept cases of mode 1 and mode 0 alternating (mode 1 alone once the 64 of mode 0 are used up) behind the hand cases --
    out of reach, a NaN force and the straight leg, once per leg (the straight leg divides by zero on "limbs", where
    rho_opt is 0; on "skew_limited" it is a regular pose, see the host module).
  * fused loop: 67 `limbs` robots on ground_z = -0.23 at the batches 1, 5, 16, 17, 67; the first 17 again with
    unilateral = 0.
  * the loop: Go1 with LL_GAINS and LL_LIMITS, 4 trot robots, 6 MPC ticks of 2 x 5 ms, unfused and fused.

Tolerance.  Device and host differ only through sin / cos / sqrt / atan2 / acos (controller) and sin / cos (plant), so the
project's fixed bars hold from the first run: 1e-12 for the controller (test_gpu_lowlevel.TOL), 1e-10 for the plant
(test_gpu_models.BARS["plant"]); flags, candidates, held and touch bit for bit.  MEASURED is the largest deviation on an
MI355X over exactly these inputs, relative to max(1, |host|); the assertions allow ten times that as well (libm may
differ between ROCm versions).  Every run prints its figures.  Fused against unfused: bytewise.
"""
import numpy as np
import pytest

import model_sets as MS
import sim_ref as S
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import lowlevel as LL
from legged_mpc_control_amd import rbd, sim, stack
from test_gpu_lowlevel import TOL, deviation, run_device, sim_outs
from test_gpu_lowsim import assert_same, assert_same_logs, run_fused, run_loop, run_unfused
from test_gpu_models import BARS, SIM_FIELDS, compare_flags, dev, filled, sim_out, up, vec
from test_gpu_sim import standing_cases
from test_gpu_stack import lowered
from test_lowlevel_host import run_host
from test_lowlevel_models_host import (BILATERAL_COUNT, LOWSIM_COUNT, hand_cases, lowsim_logs, lowsim_robots, lowsim_setup,
                                        pools)

pytestmark = pytest.mark.gpu

# largest device-vs-host deviation on this file's inputs on an MI355X, relative to max(1, |host|) (every run prints its own)
MEASURED = {
    "controller": {"tau": 2.0e-14, "joint_tau_tgt": 7.1e-15, "joint_ang_tgt": 1.3e-15, "joint_vel_tgt": 7.8e-15},
    "loop": {"tau": 4.3e-15, "joint_tau_tgt": 2.0e-15, "joint_ang_tgt": 2.2e-16, "joint_vel_tgt": 4.1e-16},
    "plant": {"qdd": 4.7e-13, "force": 2.5e-14, "foot_pos": 5.6e-17, "foot_vel": 3.9e-16, "next": 1.8e-15}}
BAR = {"controller": TOL, "loop": TOL, "plant": BARS["plant"]}
BR = 64  # robots per block of lmpc_lowlevel_kernel (test_gpu_lowlevel.test_argument_checks holds it against the library)
LL_BATCHES = (1, 5, BR - 1, BR, BR + 1, 4 * BR + 3)
LS_BATCHES = (1, 5, 16, 17, LOWSIM_COUNT)  # 16 robots per block of lmpc_lowsim_kernel
PLANT_BATCH = 17
GUARD = 4
FORCE_AT = N.LmpcSimOut.force.offset  # lmpc_sim_out.force inside a packed row


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.init()
    return torch


def judge(family, what, worst):
    """Print the run's figures; assert the family's fixed bar and ten times the MI355X's figure."""
    print(f"{what}: device vs host", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= BAR[family], f"{what}: {k}: {v:.2e} > {BAR[family]:.0e}"
        assert v <= 10.0 * MEASURED[family][k], f"{what}: {k}: {v:.2e} > ten times the measured {MEASURED[family][k]:.1e}"


# ---- lmpc_lowlevel_device against the host ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ll_pool():
    """Per kind: the cfg, (case, mode) pairs -- the hand cases, then kept cases of mode 1 and mode 0 alternating -- the
    number of hand cases, and the host's output for each, computed once and left unchanged."""
    out = {}
    for kind, count in (("skew", max(LL_BATCHES)), ("skew_limited", max(LL_BATCHES)), ("limbs", BR + 1)):
        p = pools()[kind]
        hands = [] if kind == "skew" else hand_cases(kind)
        items = [(case, 1) for _, case in hands]
        moving, standing = iter(p["cases"][1]), iter(p["cases"][0])
        while len(items) < count:
            items.append((next(moving), 1))
            nxt = next(standing, None)
            if nxt is not None and len(items) < count:
                items.append((nxt, 0))
        out[kind] = dict(cfg=p["cfg"], items=items, tags=[t for t, _ in hands],
                         host=[run_host(p["cfg"], case, mode) for case, mode in items])
    return out


@pytest.mark.parametrize("kind,batch", [(k, b) for k in ("skew", "skew_limited") for b in LL_BATCHES] + [("limbs", BR + 1)])
def test_lowlevel_device_matches_host(gpu, ll_pool, kind, batch):
    p = ll_pool[kind]
    items, host = p["items"][:batch], p["host"][:batch]
    outs = sim_outs(np.random.default_rng(batch), batch)
    rows, cand = run_device(gpu, p["cfg"], items, outs=outs)
    worst = deviation(rows[:batch], host)  # flags bit for bit, NaNs by position
    judge("controller", f"{kind} batch {batch}", worst)
    flags = LL.out_view(rows[:batch])["flags"]
    for b, tag in enumerate(p["tags"][:batch]):  # the hand cases in front
        l = ("FL", "FR", "RL", "RR").index(tag.rsplit("_", 1)[1])
        want = LL.IK_NAN if tag.startswith("far") else LL.TAU_NONFINITE if tag.startswith("nan_force") else \
            LL.VEL_NAN if kind == "limbs" else 0
        assert flags[b, l] & ~LL.CLAMPED == want, tag
    if batch >= BR - 1:
        modes = {m for _, m in items}
        assert modes == {0, 1}
        if kind != "skew":
            clamped = flags & LL.CLAMPED != 0
            assert clamped.any() and not clamped.all()
    want = np.array([[int(bool(o.held[l] | o.touch[l])) for l in range(4)] for o in outs], dtype=np.int32)
    assert np.array_equal(cand[:batch], want)
    assert np.all(rows[batch:] == 0xA5) and np.all(cand[batch:] == 0x5A5A5A5A)


def test_lowlevel_batch_independence(gpu, ll_pool):
    """On "skew_limited": a robot alone = first = last = in the middle of 259, bit for bit, for a hand case (the straight
    leg of FL), a moving and a standing robot."""
    p = ll_pool["skew_limited"]
    B = max(LL_BATCHES)
    hands = len(p["tags"])
    assert p["tags"][2] == "straight_FL" and p["items"][hands][1] == 1 and p["items"][hands + 1][1] == 0
    for r in (2, hands, hands + 1):
        alone, _ = run_device(gpu, p["cfg"], [p["items"][r]])
        others = [i for i in range(B) if i != r]
        for idx in ([r] + others, others + [r], others[:B // 2] + [r] + others[B // 2:]):
            rows, _ = run_device(gpu, p["cfg"], [p["items"][i] for i in idx])
            assert np.array_equal(rows[idx.index(r)], alone[0]), r


# ---- lmpc_lowsim_run_device against the unfused launches --------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("ticks", [1, 3, 8])
@pytest.mark.parametrize("batch", LS_BATCHES)
def test_fused_equals_unfused_on_limbs(gpu, batch, ticks, substeps):
    setup, rbs = lowsim_setup(), lowsim_robots()[:batch]
    want = run_unfused(gpu, setup, rbs, ticks, substeps)
    got = run_fused(gpu, setup, rbs, ticks, substeps)  # guard rows behind every buffer and log
    assert set(got) == set(want)
    assert_same(got, want)
    if batch == LOWSIM_COUNT and ticks == 8 and substeps == 1:  # the inputs do what the host module says
        cand = want["candidates_log"]
        words = np.ascontiguousarray(want["out_log"]).view(np.int32)[..., sim.OUT_BYTES // 4 - 10:]
        held, touch = words[..., 0:4], words[..., 4:8]
        assert np.any(cand[1:] != cand[:-1])
        assert np.any((cand == 1) & (held == 0))           # released by the unilateral rule
        assert np.any((touch[:-1] == 0) & (touch[1:] == 1))  # a touch-down on the ground off zero
        clamped = LL.out_view(want["ll_out_log"])["flags"] & LL.CLAMPED != 0
        assert clamped.any() and not clamped.all()


def test_fused_equals_unfused_bilateral(gpu):
    """unilateral = 0 reaches the fused kernel: the unfused launches' bytes, every candidate held, and a held foot that
    pulls (so the unilateral path would have released it)."""
    setup, rbs = lowsim_setup(True), lowsim_robots()[:BILATERAL_COUNT]
    want = run_unfused(gpu, setup, rbs, 8, 1)
    got = run_fused(gpu, setup, rbs, 8, 1)
    assert_same(got, want)
    held = np.ascontiguousarray(got["out_log"]).view(np.int32)[..., sim.OUT_BYTES // 4 - 10:][..., 0:4]
    assert np.array_equal(held, got["candidates_log"])
    fz = np.ascontiguousarray(got["out_log"][..., FORCE_AT:FORCE_AT + 96]).view(np.float64)[..., 2::3]
    assert np.any((held == 1) & (fz < 0.0))
    uni = run_fused(gpu, lowsim_setup(), rbs, 8, 1)
    assert not np.array_equal(uni["states"], got["states"])


# ---- the plant step the bytewise comparison rests on ------------------------------------------------------------------
def test_plant_step_on_limbs_matches_host(gpu):
    """`sim.step_device` on the `limbs` model against `sim.step`, the plant's bar: the seventh tick of the fused set's
    first 17 robots, taken from the host's explicit loop (the state and lmpc_sim_out six ticks leave, the host
    controller's torque on that state).  By then 46 of the 68 feet are candidates."""
    model, c, sc = lowsim_setup()
    md = MS.model("limbs")
    weight = sum(md["mass"]) * md["gravity"]
    rbs, logs = lowsim_robots()[:PLANT_BATCH], lowsim_logs(8, 1, LOWSIM_COUNT)[:PLANT_BATCH]
    sts = [N.LmpcRbdState.from_buffer_copy(lg["states"][5]) for lg in logs]
    cands = np.array([lg["candidates"][6] for lg in logs], dtype=np.int32)
    taus = np.array([list(LL.lowlevel(c, st, rb["target"], rb["gait"]).tau) for st, rb in zip(sts, rbs)])
    touched = set()
    for st, tau, cand in zip(sts, taus, cands):  # the inputs keep off the unilateral rule's ties and the touch threshold
        ref = S.step(md, vec(st), tau, cand, sc.dt, sc.ground_z, True)
        assert not S.tie(ref["normals"], weight), "a case on a tie: choose another tick"
        assert np.min(np.abs(ref["foot_pos"][2::3] - sc.ground_z)) > 1e-9, "a foot on the touch threshold"
        touched.update(int(x) for x in ref["touch"])
    assert touched == {0, 1} and int(cands.sum()) >= 2 * PLANT_BATCH
    B = PLANT_BATCH
    d_next, d_out = filled(gpu, B + GUARD, rbd.STATE_BYTES), filled(gpu, B + GUARD, sim.OUT_BYTES)
    sim.step_device(model, sc, up(gpu, rbd.pack(sts)), up(gpu, taus), up(gpu, cands), d_next[:B], d_out[:B], 1)
    gpu.cuda.synchronize()
    nxt, raw = d_next.cpu().numpy(), d_out.cpu().numpy()
    worst = {}
    for b in range(B):
        hn, ho = sim.step(model, sc, sts[b], taus[b], cands[b])
        d, h = sim_out(raw[b]), sim.out_dict(ho)
        compare_flags(d, h)
        for k in SIM_FIELDS:
            worst[k] = max(worst.get(k, 0.0), dev(d[k], h[k]))
        worst["next"] = max(worst.get("next", 0.0), dev(nxt[b].view(np.float64), vec(hn)))
    assert np.all(nxt[B:] == 0xA5) and np.all(raw[B:] == 0xA5)
    judge("plant", f"limbs batch {B}: step", worst)


# ---- the loop ---------------------------------------------------------------------------------------------------------
def test_loop_with_distinct_gains_and_limits(gpu):
    """StackLoop on Go1 with LL_GAINS and LL_LIMITS, 4 trot robots, wbc_per_mpc = 2 at 5 ms, 6 MPC ticks, logged: every
    logged ll_out row is lmpc_lowlevel's of the logged state, target and gait (1e-12, flags bit for bit), and the fused
    loop's log is the unfused one's bytes.  These gains are not tuned to walk: no falling condition."""
    T, W, B = 6, 2, 4
    c = LL.cfg_go1(rbd.model_go1(), kp=MS.LL_GAINS["kp"], kd=MS.LL_GAINS["kd"], tau_limit=MS.LL_LIMITS)
    (ulog, ufin), = run_loop(gpu, False, W, 0.005, [T], low_level=c)
    (flog, ffin), = run_loop(gpu, True, W, 0.005, [T], low_level=c)
    assert_same_logs(flog, ulog)
    for x, y in zip(ffin, ufin):
        assert np.array_equal(x, y)
    _, states, _ = standing_cases()
    first = [rbd.state_from_vector(s) for s in lowered(states)]
    assert ulog["ll_out"].shape == (T * W, B, LL.OUT_BYTES)
    worst = {}
    for t in range(T):
        rbs = stack.robots_from(ulog["robots"][t])
        for b in range(B):
            tgt = N.LmpcWbcTarget.from_buffer_copy(ulog["target"][t, b].tobytes())
            for i in range(W):
                k = t * W + i
                prev = first[b] if k == 0 else N.LmpcRbdState.from_buffer_copy(ulog["states"][k - 1, b].tobytes())
                h = LL.lowlevel(c, prev, tgt, rbs[b].rb.cmd.gait)
                for f, v in deviation(ulog["ll_out"][k, b:b + 1], [h]).items():
                    worst[f] = max(worst.get(f, 0.0), v)
    flags = ulog["ll_flags"]
    print(f"loop: flag words seen {sorted(set(int(v) for v in np.unique(flags)))}")
    assert np.array_equal(flags, LL.out_view(ulog["ll_out"])["flags"])
    judge("loop", "Go1 with LL_GAINS and LL_LIMITS, 6 MPC ticks", worst)
