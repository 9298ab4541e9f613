"""GPU tests of the joint-PD low-level controller (lmpc_lowlevel.hip through include/lmpc/lmpc_lowlevel.h) and of
`stack.StackLoop(..., low_level=...)`: the kernel against the host function (the same arithmetic compiled for the CPU),
the candidates it writes against `lmpc_stack_candidates_device`, guard rows, batch independence, both gait strides, and
the loop -- teacher-forced against the host stages, chaining, standing, a trot that must not fall on both of the
reference's gain sets, and the loop's other options on top of it.

Device vs host.  The two sides differ only through sin / cos / sqrt / atan2 / acos (no contraction on either side): the
doubles within 1e-12 relative to max(1, |host|), flags bit for bit.  The inputs are tests/test_lowlevel_host.py's kept
cases (every inverse-kinematics branch margin above 1e-6, so no rounding error picks a branch) with its hand cases in
front.  With R robots per block (lmpc_lowlevel_block_robots) the batches 1, 5, R - 1, R, R + 1 and 4 R + 3 cover one
robot, a partial block, one short of a block, exactly one, one robot into the second block, and several blocks with a
partial last one.

Trot.  "Not fallen" is test_gpu_stack's condition on every logged tick, with wbc_status replaced by the controller's
non-finite-torque flag.  Tracking quality is printed, not asserted.  Measured on an MI355X: see DESIGN.md 4i.
"""
import ctypes

import numpy as np
import pytest

import sim_ref as S
from conftest import rel_err
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import contact, est, rbd, rollout, sim, stack, synth
from legged_mpc_control_amd import lowlevel as LL
from test_gpu_sim import TOL as SIM_TOL
from test_gpu_sim import standing_cases
from test_gpu_stack import lowered, to_host
from test_lowlevel_host import FIELDS, hand_cases, kept_cases, run_host, target_of

pytestmark = pytest.mark.gpu

H = 10
GUARD = 4
TOL = 1e-12
BR = 64  # robots per block; test_argument_checks holds it against lmpc_lowlevel_block_robots().  Not asked of the
         # library here: loading it while the tests are collected would bring HIP up before torch does (conftest.py)
BATCHES = (1, 5, BR - 1, BR, BR + 1, 4 * BR + 3)
TROT_SPECS = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.0, 0.15), 0.0), ((0.2, 0.0), 0.3)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.init()
    return torch


@pytest.fixture(scope="module")
def pool():
    """Per robot name: the cfg, (case, mode) pairs -- for Go1 the hand cases that run on its cfg first, then kept cases
    of mode 1 and mode 0 alternating -- and the host's output for each, computed once and left unchanged."""
    out = {}
    for name, count in (("go1", max(BATCHES)), ("a1", BR + 1)):
        k1, k0 = kept_cases()[(name, 1)], kept_cases()[(name, 0)]
        items = []
        if name == "go1":
            items = [(case, mode) for tag, _, case, mode in hand_cases() if tag != "clamp"]
        i = 0
        while len(items) < count:
            items.append((k1["cases"][i // 2], 1) if i % 2 == 0 else (k0["cases"][i // 2], 0))
            i += 1
        host = [run_host(k1["cfg"], case, mode) for case, mode in items]
        out[name] = dict(cfg=k1["cfg"], items=items, host=host)
    return out


def sim_outs(rng, B):
    """B lmpc_sim_out blocks with random held / touch words (0, 1, and values a careless `|` would mishandle)."""
    outs = []
    for _ in range(B):
        o = N.LmpcSimOut()
        o.held[:] = [int(v) for v in rng.choice([0, 1, 0, 1, 2, -1], 4)]
        o.touch[:] = [int(v) for v in rng.choice([0, 1, 0, 1, 4], 4)]
        outs.append(o)
    return outs


def run_device(torch, c, items, gait="packed", outs=None):
    """The kernel on `items` ((case, mode) pairs) with GUARD prefilled rows behind every output.  gait: "packed" (int32
    [B], stride 1), "robots" (the gait word inside lmpc_stack_robot blocks, stride 240) or None (mode 1 for all).
    outs: lmpc_sim_out blocks, then the candidates are written too -> (out rows uint8 [B + GUARD][400], candidates)."""
    B = len(items)
    d_state = torch.from_numpy(np.array([case["state"] for case, _ in items])).cuda().view(torch.uint8).contiguous()
    tg = [target_of(case["forces"], case["pos_des"], case["vel_des"]) for case, _ in items]
    d_target = torch.from_numpy(stack.to_bytes(tg)).cuda()
    words = np.array([N.GAIT_STAND if mode == 0 else N.GAIT_TROT for _, mode in items], dtype=np.int32)
    d_gait = None
    if gait == "packed":
        d_gait = torch.from_numpy(words).cuda()
    elif gait == "robots":
        d_robots = torch.zeros((B, stack.ROBOT_BYTES), dtype=torch.uint8, device="cuda")
        d_gait = est.gait_view(d_robots)
        d_gait.copy_(torch.from_numpy(words).cuda())
        assert B == 1 or d_gait.stride(0) == stack.ROBOT_BYTES // 4
    d_out = torch.full((B + GUARD, LL.OUT_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
    d_cand = torch.full((B + GUARD, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_so = None if outs is None else torch.from_numpy(stack.to_bytes(outs)).cuda()
    LL.lowlevel_device(c, d_state, d_target, d_out[:B], d_gait, d_so, None if outs is None else d_cand[:B])
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_cand.cpu().numpy()


def deviation(rows, host):
    """Device rows against host structs: flags bit for bit -> the worst deviation of the doubles per field."""
    v = LL.out_view(rows)
    worst = {}
    for b, h in enumerate(host):
        assert list(v["flags"][b]) == list(h.flags), b
        for f in FIELDS:
            hv = np.array(getattr(h, f))
            nan = np.isnan(hv)
            assert np.array_equal(np.isnan(v[f][b]), nan), (b, f)
            worst[f] = max(worst.get(f, 0.0), rel_err(v[f][b][~nan], hv[~nan]) if (~nan).any() else 0.0)
    return worst


@pytest.mark.parametrize("name,batch", [("go1", b) for b in BATCHES] + [("a1", BR + 1)])
def test_device_matches_host(gpu, pool, name, batch):
    p = pool[name]
    items, host = p["items"][:batch], p["host"][:batch]
    outs = sim_outs(np.random.default_rng(batch), batch)
    rows, cand = run_device(gpu, p["cfg"], items, outs=outs)
    worst = deviation(rows[:batch], host)
    print(f"{name} batch {batch}: device vs host " + ", ".join(f"{f} {v:.2e}" for f, v in worst.items()))
    assert max(worst.values()) <= TOL
    if name == "go1" and batch >= 3:  # the hand cases in front: out of reach, a NaN force, mode 0
        flags = LL.out_view(rows)["flags"]
        assert list(flags[0]) == [LL.IK_NAN, 0, 0, 0] and list(flags[1]) == [0, 0, LL.TAU_NONFINITE, 0]
        assert rows[0, 192:216].tobytes() == items[0][0]["state"][6:9].tobytes()  # joint_ang_tgt of FL = its joint_pos
        assert rows[2, 0:96].tobytes() == rows[2, 96:192].tobytes()               # mode 0: tau is joint_tau_tgt
    want = np.array([[int(bool(o.held[l] | o.touch[l])) for l in range(4)] for o in outs], dtype=np.int32)
    assert np.array_equal(cand[:batch], want)
    assert np.all(rows[batch:] == 0xA5) and np.all(cand[batch:] == 0x5A5A5A5A)


def test_clamp_on_the_device(gpu):
    (c, case, mode), = [(c, case, mode) for tag, c, case, mode in hand_cases() if tag == "clamp"]
    rows, _ = run_device(gpu, c, [(case, mode)])
    v, h = LL.out_view(rows[:1]), run_host(c, case, mode)
    assert list(v["flags"][0]) == list(h.flags) and all(f & LL.CLAMPED for f in h.flags)
    assert np.all(np.abs(v["tau"][0]) <= 5.0) and max(deviation(rows[:1], [h]).values()) <= TOL


def test_candidates(gpu, pool):
    """Given d_sim_out / d_candidates the launch writes lmpc_stack_candidates_device's words, bit for bit; without them
    the candidate buffer is left alone, and the controller's output is the same bits either way."""
    B = 4 * BR + 3
    p = pool["go1"]
    outs = sim_outs(np.random.default_rng(99), B)
    rows, cand = run_device(gpu, p["cfg"], p["items"][:B], outs=outs)
    d_so = gpu.from_numpy(stack.to_bytes(outs)).cuda()
    d_ref = gpu.full((B, 4), 0x5A5A5A5A, dtype=gpu.int32, device="cuda")
    stack.candidates_device(d_so, d_ref)
    gpu.cuda.synchronize()
    assert np.array_equal(cand[:B], d_ref.cpu().numpy())
    assert set(np.unique(cand[:B])) == {0, 1}
    rows2, cand2 = run_device(gpu, p["cfg"], p["items"][:B], outs=None)
    assert np.all(cand2 == 0x5A5A5A5A)
    assert np.array_equal(rows, rows2)


def test_batch_independence_and_gait_strides(gpu, pool):
    """A robot alone = first = last = in the middle of the largest batch, bit for bit, for a moving and a standing
    robot; the gait word read with stride 1 and with lmpc_stack_robot's stride gives the same bits."""
    p = pool["go1"]
    B = 4 * BR + 3
    for r in (7, 8):  # a kept case of mode 1 and one of mode 0
        assert p["items"][r][1] == (1 if r == 7 else 0)
        alone, _ = run_device(gpu, p["cfg"], [p["items"][r]])
        others = [i for i in range(B) if i != r]
        for idx in ([r] + others, others + [r], others[:B // 2] + [r] + others[B // 2:]):
            rows, _ = run_device(gpu, p["cfg"], [p["items"][i] for i in idx])
            assert np.array_equal(rows[idx.index(r)], alone[0])
    a, _ = run_device(gpu, p["cfg"], p["items"][:B], gait="packed")
    b, _ = run_device(gpu, p["cfg"], p["items"][:B], gait="robots")
    assert np.array_equal(a, b)
    # NULL gait: mode 1 for every robot, so only the standing ones change
    c, _ = run_device(gpu, p["cfg"], p["items"][:B], gait=None)
    modes = np.array([m for _, m in p["items"][:B]])
    assert np.array_equal(a[:B][modes == 1], c[:B][modes == 1])
    assert not np.array_equal(a[:B][modes == 0], c[:B][modes == 0])


# ---- the loop ------------------------------------------------------------------------------------------------------
def make_loop(states, specs, wbc_per_mpc, sim_dt, gait, low_level, **options):
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    sts = [rbd.state_from_vector(s) for s in states]
    robots, outs = [], []
    for st, (vd, yr) in zip(sts, specs):
        rb, o = stack.robot_init(cfg, model, st, vd, yr, float(st.pos[2]), gait, 4.0)
        robots.append(rb), outs.append(o)
    loop = stack.StackLoop(model, p, H, len(states), cfg, sim.cfg(dt=sim_dt, ground_z=0.0), wbc_per_mpc,
                           low_level=low_level, **options)
    return loop, robots, sts, outs


def upload(torch, *lists):
    return [torch.from_numpy(stack.to_bytes(x)).cuda() for x in lists]


def gains(name):
    """The reference's Go1 or A1 Gazebo gains on the Go1 model's own kinematics."""
    return LL.cfg_go1(rbd.model_go1()) if name == "go1" else LL.cfg_a1(rbd.model_go1())


@pytest.fixture(scope="module")
def forced(gpu):
    """4 trot robots, wbc_per_mpc = 2 at a 5 ms plant step, 12 MPC ticks, logged; run once for the two tests on it."""
    md, states, _ = standing_cases()
    specs = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.2, -0.1), 0.2), ((-0.2, 0.0), -0.3)]
    c = gains("go1")
    loop, robots, sts, outs = make_loop(lowered(states), specs, 2, 0.005, N.GAIT_TROT, c)
    assert loop.pipeline is None
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 12, log=True))
    gpu.cuda.synchronize()
    final = [x.cpu().numpy() for x in (d_rb, d_st, d_out)]
    yield dict(md=md, cfg=c, loop=loop, robots=robots, sts=sts, outs=outs, log=log, final=final)
    loop.close()


def test_teacher_forced_loop(gpu, forced):
    """Every low-level tick's controller output recomputed on the host from the logged state, target and gait; every
    plant step recomputed from the logged tau; the candidates from the previous step's held | touch."""
    f, log = forced, forced["log"]
    loop, md, W = f["loop"], f["md"], 2
    T, B = 12, 4
    assert "wbc_status" not in log and "wbc_iters" not in log
    assert np.all(log["qp_status"] == 0) and np.all(log["sim_status"] == 0)
    assert log["ll_out"].shape == (T * W, B, LL.OUT_BYTES) and log["ll_flags"].shape == (T * W, B, 4)
    assert np.array_equal(log["ll_flags"], LL.out_view(log["ll_out"])["flags"])
    assert np.array_equal(log["tau"], LL.out_view(log["ll_out"])["tau"])
    weight = sum(md["mass"]) * md["gravity"]
    worst_ll = worst_step = 0.0
    ties = 0
    for t in range(T):
        rbs = stack.robots_from(log["robots"][t])
        for b in range(B):
            tgt = N.LmpcWbcTarget.from_buffer_copy(log["target"][t, b].tobytes())
            for i in range(W):
                k = t * W + i
                prev_st = f["sts"][b] if k == 0 else N.LmpcRbdState.from_buffer_copy(log["states"][k - 1, b].tobytes())
                prev_out = f["outs"][b] if k == 0 else N.LmpcSimOut.from_buffer_copy(log["out"][k - 1, b].tobytes())
                h = LL.lowlevel(f["cfg"], prev_st, tgt, rbs[b].rb.cmd.gait)
                worst_ll = max(worst_ll, max(deviation(log["ll_out"][k, b:b + 1], [h]).values()))
                cand = [int(bool(prev_out.held[l] | prev_out.touch[l])) for l in range(4)]
                assert list(log["candidates"][k, b]) == cand
                nxt, ho = sim.step(loop.model, loop.sim_cfg, prev_st, log["tau"][k, b], cand)
                worst_step = max(worst_step, rel_err(log["states"][k, b].view(np.float64),
                                                     np.frombuffer(bytes(nxt), dtype=np.float64)))
                ref = S.step(md, np.frombuffer(bytes(prev_st), dtype=np.float64), log["tau"][k, b], cand, 0.005, 0.0, True)
                if S.tie(ref["normals"], weight):
                    ties += 1
                else:
                    assert list(log["held"][k, b]) == list(ho.held)
    print(f"teacher-forced: controller {worst_ll:.2e} (bound {TOL:.0e}), plant step {worst_step:.2e} (bound "
          f"{10 * SIM_TOL['next']:.1e}); {ties} steps on a tie of the unilateral rule, held not compared there")
    assert worst_ll <= TOL
    assert worst_step <= 10 * SIM_TOL["next"]
    assert ties <= T * W * B // 10
    assert np.array_equal(f["final"][0], log["robots"][-1]) and np.array_equal(f["final"][1], log["states"][-1])
    assert np.array_equal(f["final"][2], log["out"][-1])


def test_chaining(gpu, forced):
    """5 + 7 MPC ticks leave the bits of 12: robots, state, out and every log."""
    f = forced
    loop = f["loop"]
    d_rb, d_st, d_out = upload(gpu, f["robots"], f["sts"], f["outs"])
    a = to_host(loop.run_device(d_rb, d_st, d_out, 5, log=True))
    b = to_host(loop.run_device(d_rb, d_st, d_out, 7, log=True))
    assert loop.run_device(d_rb, d_st, d_out, 0) is None
    gpu.cuda.synchronize()
    for x, y in zip((d_rb, d_st, d_out), f["final"]):
        assert np.array_equal(x.cpu().numpy(), y)
    for k, v in f["log"].items():
        assert np.array_equal(np.concatenate([a[k], b[k]]), v, equal_nan=v.dtype.kind == "f"), k


@pytest.mark.parametrize("name", ["go1", "a1"])
def test_standing(gpu, name):
    """LMPC_GAIT_STAND at the reference's rates (10 ms / 1.25 ms), 10 MPC ticks: mode 0, the forces are the MPC's."""
    md, states, _ = standing_cases()
    loop, robots, sts, outs = make_loop(lowered(states), [((0.0, 0.0), 0.0)] * 4, 8, 0.00125, N.GAIT_STAND, gains(name))
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 10, log=True))
    gpu.cuda.synchronize()
    loop.close()
    assert np.all(log["qp_status"] == 0) and np.all(log["ll_flags"] & LL.TAU_NONFINITE == 0) and np.all(log["sim_status"] == 0)
    assert np.all(log["held"] == 1)
    v = LL.out_view(log["ll_out"])
    assert np.array_equal(v["tau"], v["joint_tau_tgt"])  # mode 0
    height = log["states"].view(np.float64)[:, :, 5]
    drop = float(np.max(np.abs(height - np.array([s[5] for s in lowered(states)]))))
    free_fall = 0.5 * md["gravity"] * 0.1 ** 2
    print(f"standing ({name} gains): trunk height changes by {1e3 * drop:.3f} mm in 0.1 s (free fall {1e3 * free_fall:.1f} mm)")
    assert drop < 0.1 * free_fall


def not_fallen(log, states):
    x = log["states"].view(np.float64)
    ok = np.all(np.abs(x[:, :, 2]) < 0.5) and np.all(np.abs(x[:, :, 1]) < 0.5)
    return ok and all(np.all(x[:, b, 5] > 0.5 * states[b][5]) for b in range(x.shape[1]))


@pytest.mark.parametrize("name", ["go1", "a1"])
def test_trot_does_not_fall(gpu, name):
    """4 robots trot at gait speed 4.0 for 50 MPC ticks (two gait cycles) at 10 ms / 1.25 ms: in place, at 0.3 m/s, and
    two more (sideways, turning): test_gpu_stack.test_trot_does_not_fall on the joint-PD controller."""
    md, states, _ = standing_cases()
    states = lowered(states)
    T, W = 50, 8
    loop, robots, sts, outs = make_loop(states, TROT_SPECS, W, 0.00125, N.GAIT_TROT, gains(name))
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, T, log=True))
    gpu.cuda.synchronize()
    loop.close()
    x = log["states"].view(np.float64)  # [K][B][36]: yaw pitch roll, pos, joints, omega, v, joint rates
    pc = stack.robots_view(log["robots"])["plan_contacts"].astype(np.int32)  # [T][B][4]
    ended = held_after = by_touch = 0
    for t in range(1, T):
        for b in range(4):
            for l in range(4):
                if pc[t - 1, b, l] == 0 and pc[t, b, l] == 1:
                    ended += 1
                    by_touch += int(log["touch"][t * W - 1, b, l] == 1)
                    t2 = next((u for u in range(t + 1, T) if pc[u, b, l] == 0), T)
                    held_after += int(np.any(log["held"][t * W:t2 * W, b, l] == 1))
    for b, (vd, yr) in enumerate(TROT_SPECS):
        v_end = x[-W:, b, 21:23].mean(axis=0)
        c, s = np.cos(x[-1, b, 0]), np.sin(x[-1, b, 0])
        print(f"trot ({name} gains) robot {b}: command v = {vd}, yaw rate {yr}; end body velocity "
              f"({c * v_end[0] + s * v_end[1]:+.3f}, {-s * v_end[0] + c * v_end[1]:+.3f}) m/s, height "
              f"{x[:, b, 5].min():.4f}..{x[:, b, 5].max():.4f} m (commanded {states[b][5]:.4f}), roll "
              f"{x[:, b, 2].min():+.4f}..{x[:, b, 2].max():+.4f}, pitch {x[:, b, 1].min():+.4f}..{x[:, b, 1].max():+.4f} rad, "
              f"yaw change {x[-1, b, 0] - states[b][0]:+.4f} rad")
    flags = log["ll_flags"]
    bad = [int((log["qp_status"] != 0).sum()), int((flags & LL.TAU_NONFINITE != 0).sum()), int((log["sim_status"] != 0).sum())]
    print(f"trot ({name} gains): non-zero statuses qp / non-finite tau / sim = {bad}; flag words seen "
          f"{sorted(set(int(v) for v in np.unique(flags)))}; {ended} swings ended ({by_touch} with the touch flag set), "
          f"{held_after} of them then held by the plant")
    assert bad == [0, 0, 0]
    assert not_fallen(log, states)
    assert ended >= 1 and held_after >= 1


@pytest.mark.parametrize("option", ["estimator", "contact"])
def test_composition(gpu, option):
    """The loop's other options on top of the joint-PD controller, one 12-tick trot each: the Kalman filter's estimate as
    the feedback, and the frictional contact plant (under which the candidate words stay all ones)."""
    md, states, _ = standing_cases()
    states = lowered(states)
    opts = dict(estimator=est.cfg(dt=0.00125)) if option == "estimator" else \
        dict(plant=contact.cfg(dt=0.00125, ground_z=0.0))
    loop, robots, sts, outs = make_loop(states, TROT_SPECS, 8, 0.00125, N.GAIT_TROT, gains("go1"), **opts)
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 12, log=True))
    gpu.cuda.synchronize()
    loop.close()
    x = log["states"].view(np.float64)
    print(f"composition ({option}): height {x[:, :, 5].min():.4f}..{x[:, :, 5].max():.4f} m, |roll| <= "
          f"{np.abs(x[:, :, 2]).max():.4f}, |pitch| <= {np.abs(x[:, :, 1]).max():.4f} rad")
    assert np.all(log["qp_status"] == 0) and np.all(log["sim_status"] == 0)
    assert np.all(log["ll_flags"] & LL.TAU_NONFINITE == 0)
    if option == "estimator":
        assert np.all(log["est_status"] == 0)
    else:
        assert np.all(log["candidates"] == 1)
        assert np.all(np.ascontiguousarray(log["contact_out"]).view(np.int32)[..., 42] == 0)
    assert not_fallen(log, states)


def test_argument_checks(gpu):
    p, rcfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    c = gains("go1")
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 2, rcfg, sim.cfg(dt=0.005), 2, low_level=c, wbc_warm=True)
    L = N.lib()
    assert L.lmpc_lowlevel_block_robots() == BR
    R_ = ctypes.byref
    d = lambda n, w: gpu.zeros((n, w), dtype=gpu.uint8, device="cuda")
    st, tg, out, so = d(2, rbd.STATE_BYTES), d(2, rbd.TARGET_BYTES), d(2, LL.OUT_BYTES), d(2, sim.OUT_BYTES)
    gait, cand = gpu.zeros(2, dtype=gpu.int32, device="cuda"), gpu.zeros((2, 4), dtype=gpu.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.lmpc_lowlevel_device(R_(c), None, P(tg), None, 0, None, None, 2, P(out), None) == -1  # NULL required pointers
    assert L.lmpc_lowlevel_device(R_(c), P(st), None, None, 0, None, None, 2, P(out), None) == -1
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), None, 0, None, None, 2, None, None) == -1
    assert L.lmpc_lowlevel_device(None, P(st), P(tg), None, 0, None, None, 2, P(out), None) == -1
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), None, 0, None, None, -1, P(out), None) == -1  # a negative batch
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), P(gait), 0, None, None, 2, P(out), None) == -1  # a bad stride
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), None, 0, P(so), None, 2, P(out), None) == -1
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), None, 0, None, P(cand), 2, P(out), None) == -1
    assert L.lmpc_lowlevel_device(R_(c), None, None, None, 0, None, None, 0, None, None) == 0  # batch 0: nothing done
    assert L.lmpc_lowlevel_device(R_(c), P(st), P(tg), P(gait), 1, P(so), P(cand), 2, P(out), None) == 0
    gpu.cuda.synchronize()
    with pytest.raises(ValueError):
        LL.lowlevel_device(c, st, tg, d(1, LL.OUT_BYTES))
    with pytest.raises(ValueError):
        LL.lowlevel_device(c, st, tg, out, d_sim_out=so)
    with pytest.raises(ValueError):
        LL.lowlevel_device(c, st, tg, out, d_gait=gpu.zeros(3, dtype=gpu.int32, device="cuda"))
