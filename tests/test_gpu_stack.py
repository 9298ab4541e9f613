"""GPU tests of the full loop (include/lmpc/lmpc_stack.h; Go1, H = 10): the device advance / targets / candidates
against the host functions (the same arithmetic compiled for the CPU), the records the advance launch leaves in the MPC
context, guard rows, batch independence, and `StackLoop` -- teacher-forced against the host stages and the CPU oracle,
chaining, standing, and a trot that must not fall.

Device vs host.  The two sides differ only through sin / cos / sqrt (no contraction on either side): the FSM fields,
flags and plan_contacts match bit for bit, the doubles within 1e-12 relative to max(1, |host|); `targets` is a copy and
matches bit for bit.  The batches 1, 5, 16, 17 and 67 cover one robot, a partial block, exactly one block of 16 robots,
one robot into the second block, and several blocks with a partial last one.

Teacher-forced loop.  Every stage of every logged tick is recomputed on the host from the logged inputs of that stage:
the advance (1e-12, FSM bit for bit), the QP (the CPU oracle's optimum, 1e-7: tests/test_gpu_rollout.py's bar), the
targets (bit for bit) and the plant step (ten times tests/test_gpu_sim.py's device-vs-host step figure TOL["next"]).
held is compared bit for bit while tests/sim_ref.py reports no tie of the unilateral rule; touch where the host's foot
is more than 1e-9 m from the threshold (test_gpu_sim's own condition on its pool).

Trot.  "Not fallen" is a condition on every logged tick (all statuses 0, |roll|, |pitch| < 0.5 rad, trunk above half
the commanded height).  Tracking quality is printed, not asserted: there is no reference run to measure it against.
Measured on an MI355X: see DESIGN.md 1c.
"""
import ctypes

import numpy as np
import pytest

import sim_ref as S
import stack_ref as SR
from conftest import rel_err
from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import rbd, rollout, sim, stack, synth
from oracle import oracle as O
from test_gpu_sim import TOL as SIM_TOL
from test_gpu_sim import standing_cases
from test_stack_host import sim_out, standing_state, swing_robot

pytestmark = pytest.mark.gpu

H = 10
BATCHES = (1, 5, 16, 17, 67)
GUARD = 4
DT = 0.01
INT_FIELDS = ("gait", "plan_contacts", "fsm_index", "tick", "not_first_call")


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.init()
    return torch


@pytest.fixture(scope="module")
def solver(gpu):
    from legged_mpc_control_amd import BatchedConvexQPSolver

    return BatchedConvexQPSolver(synth.params(), H, max_batch=0)


@pytest.fixture(scope="module")
def pool():
    """67 robots in varied FSM states (every gait; 0 to 40 host ticks of synthetic feedback behind them), the state and
    plant output of their next tick, a force block, and the host's advance and targets for them, computed once.
    Robot 0 is the hand case: FL at 95 % of its swing with the flag set."""
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    rng = np.random.default_rng(2024)
    before, states, outs = [], [], []
    for i in range(67):
        gait = (N.GAIT_TROT, N.GAIT_CRAWL, N.GAIT_TROT_WITH_STAND, N.GAIT_STAND, N.GAIT_TROT)[i % 5]
        s0 = standing_state(yaw=rng.uniform(-3, 3), x=rng.uniform(-1, 1), y=rng.uniform(-1, 1))
        n = int(rng.integers(0, 41))
        st, fp, tc = SR.synthetic_feedback(rng, n + 1, s0)
        if i == 0:
            _, s0, rb, out = swing_robot(0.95)
            st, fp, tc = s0[None, :], np.array(out.foot_pos)[None, :], np.array([[1, 0, 1, 0]])
            n = 0
        else:
            rb, _ = stack.robot_init(cfg, model, rbd.state_from_vector(s0), (rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)),
                                     rng.uniform(-0.4, 0.4), 0.30, gait, rng.uniform(2.5, 4.5))
        for t in range(n):
            stack.advance(p, cfg, rb, rbd.state_from_vector(st[t]), sim_out(fp[t], tc[t]))
        before.append(rb)
        states.append(rbd.state_from_vector(st[n]))
        o = sim_out(fp[n], tc[n])
        o.held[:] = [int(v) for v in rng.integers(0, 2, 4)]
        outs.append(o)
    grf = rng.normal(size=(67, H, 12)) * 30.0
    tmpl = rbd.target(torque_limits=(20.0, 25.0, 30.0), mu=0.4, swing_kp=300.0, swing_kd=30.0)
    after, tgts = [], []
    for i in range(67):
        rb = N.LmpcStackRobot.from_buffer_copy(bytes(before[i]))
        stack.advance(p, cfg, rb, states[i], outs[i])
        after.append(rb)
        tgts.append(stack.targets(rb, grf[i, 0], tmpl))
    assert after[0].rb.cmd.plan_contacts[0] == 1 and before[0].rb.cmd.plan_contacts[0] == 0  # the early touchdown
    return dict(p=p, cfg=cfg, model=model, before=before, states=states, outs=outs, grf=grf, tmpl=tmpl, after=after,
                tgts=tgts)


def run_advance(torch, solver, pool, idx):
    """advance, records, targets and candidates on the device for the pool's robots `idx`, every output with GUARD
    prefilled rows behind it -> dict of NumPy arrays."""
    B = len(idx)

    def guarded(rows, fill=0xA5):
        g = torch.full((B + GUARD, rows.shape[1]), fill, dtype=torch.uint8, device="cuda")
        g[:B] = torch.from_numpy(rows).cuda()
        return g

    d_robots = guarded(stack.to_bytes([pool["before"][i] for i in idx]))
    d_state = torch.from_numpy(stack.to_bytes([pool["states"][i] for i in idx])).cuda()
    d_out = torch.from_numpy(stack.to_bytes([pool["outs"][i] for i in idx])).cuda()
    d_grf = torch.from_numpy(np.ascontiguousarray(pool["grf"][idx])).cuda()
    d_target = torch.full((B + GUARD, rbd.TARGET_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
    d_cand = torch.full((B + GUARD, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stack.advance_device(solver, pool["cfg"], d_robots[:B], d_state, d_out)
    d_rec, d_con = stack.context_records(solver, B)
    stack.targets_device(d_robots[:B], d_grf, pool["tmpl"], d_target[:B])
    stack.candidates_device(d_out, d_cand[:B])
    d_rec2, d_con2 = solver.build_records_device(d_robots[:B, :N.COMMAND_BYTES].contiguous())
    torch.cuda.synchronize()
    return dict(robots=d_robots.cpu().numpy(), target=d_target.cpu().numpy(), cand=d_cand.cpu().numpy(),
                rec=d_rec.cpu().numpy(), con=d_con.cpu().numpy(), rec2=d_rec2.cpu().numpy(), con2=d_con2.cpu().numpy())


def robot_deviation(dev_rows, host_structs):
    """Device robots (uint8 [B][960]) against host structs: the integer fields bit for bit -> the worst deviation of
    the doubles relative to max(1, |host|)."""
    d = stack.robots_view(dev_rows)
    h = stack.robots_view(stack.to_bytes(host_structs))
    worst = 0.0
    for name in stack.STACK_ROBOT_DTYPE.names:
        if name in INT_FIELDS:
            assert np.array_equal(d[name], h[name]), name
        else:
            worst = max(worst, rel_err(d[name], h[name]))
    return worst


@pytest.mark.parametrize("batch", BATCHES)
def test_device_matches_host(gpu, solver, pool, batch):
    idx = list(range(batch))
    got = run_advance(gpu, solver, pool, idx)
    worst = robot_deviation(got["robots"][:batch], [pool["after"][i] for i in idx])
    print(f"batch {batch}: device advance vs host, doubles within {worst:.2e}")
    assert worst <= 1e-12
    # targets: a copy of the device's own robots, the forces and the template, bit for bit
    dev_robots = stack.robots_from(got["robots"][:batch])
    for b in range(batch):
        assert bytes(got["target"][b]) == bytes(stack.targets(dev_robots[b], pool["grf"][b, 0], pool["tmpl"]))
    assert rel_err(np.array([got["target"][b, :288].view(np.float64) for b in range(batch)]),
                   np.array([np.frombuffer(bytes(pool["tgts"][b]), dtype=np.float64)[:36] for b in range(batch)])) <= 1e-12
    want = np.array([[int(bool(o.held[l] | o.touch[l])) for l in range(4)] for o in pool["outs"][:batch]], dtype=np.int32)
    assert np.array_equal(got["cand"][:batch], want)
    # the records the advance launch left in the context are lmpc_build_records_device's, bit for bit
    assert np.array_equal(got["rec"].view(np.uint64), got["rec2"].view(np.uint64)) and np.array_equal(got["con"], got["con2"])
    # guard rows
    assert np.all(got["robots"][batch:] == 0xA5) and np.all(got["target"][batch:] == 0xA5)
    assert np.all(got["cand"][batch:] == 0x5A5A5A5A)


def test_batch_independence(gpu, solver, pool):
    """A robot alone = first = last = in the middle of 67, bit for bit (robot 7, mid-swing)."""
    r = 7
    alone = run_advance(gpu, solver, pool, [r])
    others = [i for i in range(67) if i != r]
    for idx in ([r] + others, others + [r], others[:33] + [r] + others[33:]):
        got = run_advance(gpu, solver, pool, idx)
        k = idx.index(r)
        for key in ("robots", "target", "cand", "rec", "con"):
            assert np.array_equal(got[key][k], alone[key][0]), key


# ---- the loop ------------------------------------------------------------------------------------------------------
def loop_setup(torch, states, specs, wbc_per_mpc, sim_dt, gait, speed=4.0):
    """specs: (vel_d, yaw_rate) per robot.  -> (loop, host robots, host states, host first outs, device buffers)."""
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    sts = [rbd.state_from_vector(s) for s in states]
    robots, outs = [], []
    for st, (vd, yr) in zip(sts, specs):
        rb, o = stack.robot_init(cfg, model, st, vd, yr, float(st.pos[2]), gait, speed)
        robots.append(rb)
        outs.append(o)
    loop = stack.StackLoop(model, p, H, len(states), cfg, sim.cfg(dt=sim_dt, ground_z=0.0), wbc_per_mpc)
    bufs = [torch.from_numpy(stack.to_bytes(x)).cuda() for x in (robots, sts, outs)]
    return loop, robots, sts, outs, bufs


def lowered(states, by=1e-6):
    """test_gpu_sim's standing pose, the trunk 1 um lower: the feet are then below the touch threshold by a margin
    instead of within a rounding error of it."""
    out = [s.copy() for s in states]
    for s in out:
        s[5] -= by
    return out


def to_host(log):
    return {k: v.cpu().numpy() for k, v in log.items()}


@pytest.fixture(scope="module")
def forced(gpu):
    """4 trot robots, wbc_per_mpc = 2 at a 5 ms plant step, 12 MPC ticks, logged; run once for the two tests on it."""
    md, states, _ = standing_cases()
    states = lowered(states)
    specs = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.2, -0.1), 0.2), ((-0.2, 0.0), -0.3)]
    loop, robots, sts, outs, (d_rb, d_st, d_out) = loop_setup(gpu, states, specs, 2, 0.005, N.GAIT_TROT)
    log = loop.run_device(d_rb, d_st, d_out, 12, log=True)
    gpu.cuda.synchronize()
    final = [x.cpu().numpy() for x in (d_rb, d_st, d_out)]
    yield dict(md=md, loop=loop, robots=robots, sts=sts, outs=outs, log=to_host(log), final=final)
    loop.close()


def test_teacher_forced_loop(gpu, forced):
    f, log = forced, forced["log"]
    loop, md = f["loop"], f["md"]
    p, cfg, model, W = loop.params, loop.rollout_cfg, loop.model, loop.wbc_per_mpc
    T, B = 12, 4
    assert np.all(log["qp_status"] == 0) and np.all(log["wbc_status"] == 0) and np.all(log["sim_status"] == 0)
    weight = sum(md["mass"]) * md["gravity"]
    op = O.params_from(p)
    worst_adv = worst_step = 0.0
    recs, cons = [], []
    skipped_touch = 0
    for t in range(T):
        prev_rb = f["robots"] if t == 0 else stack.robots_from(log["robots"][t - 1])
        k0 = t * W - 1
        for b in range(B):
            st = f["sts"][b] if t == 0 else N.LmpcRbdState.from_buffer_copy(log["states"][k0, b].tobytes())
            out = f["outs"][b] if t == 0 else N.LmpcSimOut.from_buffer_copy(log["out"][k0, b].tobytes())
            rb = N.LmpcStackRobot.from_buffer_copy(bytes(prev_rb[b]))
            stack.advance(p, cfg, rb, st, out)
            worst_adv = max(worst_adv, robot_deviation(log["robots"][t, b:b + 1], [rb]))
            dev_rb = stack.robots_from(log["robots"][t, b:b + 1])[0]
            assert bytes(log["cmd"][t, b]) == bytes(dev_rb.rb.cmd)
            r, c = synth.command_to_record(p, H, dev_rb.rb.cmd)
            recs.append(r)
            cons.append(c)
            assert bytes(log["target"][t, b]) == bytes(stack.targets(dev_rb, log["u0"][t, b], loop.template))
            for i in range(W):
                k = t * W + i
                prev_out = out if i == 0 else N.LmpcSimOut.from_buffer_copy(log["out"][k - 1, b].tobytes())
                prev_st = st if i == 0 else N.LmpcRbdState.from_buffer_copy(log["states"][k - 1, b].tobytes())
                cand = [int(bool(prev_out.held[l] | prev_out.touch[l])) for l in range(4)]
                assert list(log["candidates"][k, b]) == cand
                nxt, ho = sim.step(model, loop.sim_cfg, prev_st, log["tau"][k, b], cand)
                worst_step = max(worst_step, rel_err(log["states"][k, b].view(np.float64),
                                                     np.frombuffer(bytes(nxt), dtype=np.float64)))
                ref = S.step(md, np.frombuffer(bytes(prev_st), dtype=np.float64), log["tau"][k, b], cand, 0.005, 0.0, True)
                assert not S.tie(ref["normals"], weight), f"tick {k} robot {b} on a tie: choose another pose"
                assert list(log["held"][k, b]) == list(ho.held)
                for l in range(4):
                    if abs(ho.foot_pos[3 * l + 2]) > 1e-9:
                        assert log["touch"][k, b, l] == ho.touch[l]
                    else:
                        skipped_touch += 1
    ref, _, fails = O.solve_batch(op, H, np.array(recs), np.array(cons), n_threads=8)
    assert fails == 0
    err = rel_err(log["u0"].reshape(-1, 12), ref[:, 0])
    print(f"teacher-forced: advance {worst_adv:.2e} (bound 1e-12), u_0 vs oracle {err:.2e} (bound 1e-7), plant step "
          f"{worst_step:.2e} (bound {10 * SIM_TOL['next']:.1e}); {skipped_touch} touch flags within 1e-9 m of the "
          f"threshold not compared")
    assert worst_adv <= 1e-12
    assert err <= 1e-7
    assert worst_step <= 10 * SIM_TOL["next"]
    # the loop's buffers hold the last logged tick
    assert np.array_equal(f["final"][0], log["robots"][-1]) and np.array_equal(f["final"][1], log["states"][-1])
    assert np.array_equal(f["final"][2], log["out"][-1])


def test_chaining(gpu, forced):
    """5 + 7 MPC ticks leave the bits of 12: robots, state, out and every log."""
    f = forced
    loop = f["loop"]
    d_rb, d_st, d_out = (gpu.from_numpy(stack.to_bytes(x)).cuda() for x in (f["robots"], f["sts"], f["outs"]))
    a = to_host(loop.run_device(d_rb, d_st, d_out, 5, log=True))
    b = to_host(loop.run_device(d_rb, d_st, d_out, 7, log=True))
    assert loop.run_device(d_rb, d_st, d_out, 0) is None
    gpu.cuda.synchronize()
    for x, y in zip((d_rb, d_st, d_out), f["final"]):
        assert np.array_equal(x.cpu().numpy(), y)
    for k, v in f["log"].items():
        assert np.array_equal(np.concatenate([a[k], b[k]]), v), k


def test_standing(gpu):
    """LMPC_GAIT_STAND at the reference's rates (10 ms / 1.25 ms), 10 MPC ticks: the forces are the MPC's."""
    md, states, _ = standing_cases()
    loop, robots, sts, outs, (d_rb, d_st, d_out) = loop_setup(gpu, lowered(states), [((0.0, 0.0), 0.0)] * 4, 8, 0.00125,
                                                              N.GAIT_STAND)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 10, log=True))
    gpu.cuda.synchronize()
    loop.close()
    assert np.all(log["qp_status"] == 0) and np.all(log["wbc_status"] == 0) and np.all(log["sim_status"] == 0)
    assert np.all(log["held"] == 1)
    height = log["states"].view(np.float64)[:, :, 5]
    drop = float(np.max(np.abs(height - np.array([s[5] for s in lowered(states)]))))
    free_fall = 0.5 * md["gravity"] * 0.1 ** 2
    print(f"standing: trunk height changes by {1e3 * drop:.3f} mm in 0.1 s (free fall {1e3 * free_fall:.1f} mm)")
    assert drop < 0.1 * free_fall


def test_trot_does_not_fall(gpu):
    """4 robots trot at gait speed 4.0 for 50 MPC ticks (two gait cycles) at 10 ms / 1.25 ms: in place, at 0.3 m/s, and
    two more (sideways, turning)."""
    md, states, _ = standing_cases()
    states = lowered(states)
    specs = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.0, 0.15), 0.0), ((0.2, 0.0), 0.3)]
    T, W = 50, 8
    loop, robots, sts, outs, (d_rb, d_st, d_out) = loop_setup(gpu, states, specs, W, 0.00125, N.GAIT_TROT)
    log = to_host(loop.run_device(d_rb, d_st, d_out, T, log=True))
    gpu.cuda.synchronize()
    loop.close()
    x = log["states"].view(np.float64)  # [K][B][36]: yaw pitch roll, pos, joints, omega, v, joint rates
    rbv = stack.robots_view(log["robots"])
    # touchdown was exercised: a swing ended (plan_contacts 0 -> 1 between MPC ticks) and the plant then held that foot
    # during the stance that followed (before the leg's next swing began, or the run's end)
    pc = rbv["plan_contacts"].astype(np.int32)  # [T][B][4]
    ended = held_after = by_touch = 0
    delays = []
    for t in range(1, T):
        for b in range(4):
            for l in range(4):
                if pc[t - 1, b, l] == 0 and pc[t, b, l] == 1:
                    ended += 1
                    # the flag the FSM saw at that tick: set means the swing ended by touch (or touched as it timed out)
                    by_touch += int(log["touch"][t * W - 1, b, l] == 1)
                    t2 = next((u for u in range(t + 1, T) if pc[u, b, l] == 0), T)
                    held = np.flatnonzero(log["held"][t * W:t2 * W, b, l] == 1)
                    if held.size:
                        held_after += 1
                        delays.append(int(held[0]))
    for b, (vd, yr) in enumerate(specs):
        v_end = x[-W:, b, 21:23].mean(axis=0)
        yaw = x[-1, b, 0]
        c, s = np.cos(yaw), np.sin(yaw)
        v_body = np.array([c * v_end[0] + s * v_end[1], -s * v_end[0] + c * v_end[1]])
        print(f"trot robot {b}: command v = {vd}, yaw rate {yr}; end body velocity ({v_body[0]:+.3f}, {v_body[1]:+.3f}) m/s "
              f"(mean of the last MPC tick), height {x[:, b, 5].min():.4f}..{x[:, b, 5].max():.4f} m (commanded "
              f"{states[b][5]:.4f}), roll {x[:, b, 2].min():+.4f}..{x[:, b, 2].max():+.4f}, pitch "
              f"{x[:, b, 1].min():+.4f}..{x[:, b, 1].max():+.4f} rad, yaw change {x[-1, b, 0] - states[b][0]:+.4f} rad")
    bad = [int((log[k] != 0).sum()) for k in ("qp_status", "wbc_status", "sim_status")]
    print(f"trot: non-zero statuses qp / wbc / sim = {bad}; {ended} swings ended ({by_touch} with the touch flag set), "
          f"{held_after} of them then held by the plant, after {min(delays, default=-1)}..{max(delays, default=-1)} "
          f"low-level ticks")
    assert bad == [0, 0, 0]
    assert np.all(np.abs(x[:, :, 2]) < 0.5) and np.all(np.abs(x[:, :, 1]) < 0.5)
    for b in range(4):
        assert np.all(x[:, b, 5] > 0.5 * states[b][5])
    assert ended >= 1 and held_after >= 1


def test_loop_argument_checks(gpu):
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 4, cfg, sim.cfg(dt=0.00125), 7)
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 4, cfg, sim.cfg(dt=0.005, unilateral=False), 2)
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 0, cfg, sim.cfg(dt=0.005), 2)
    loop = stack.StackLoop(model, p, H, 2, cfg, sim.cfg(dt=0.005), 2)
    d = lambda n, w: gpu.zeros((n, w), dtype=gpu.uint8, device="cuda")
    with pytest.raises(ValueError):
        loop.run_device(d(3, stack.ROBOT_BYTES), d(3, rbd.STATE_BYTES), d(3, sim.OUT_BYTES), 1)  # above max_batch
    with pytest.raises(ValueError):
        loop.run_device(d(2, stack.ROBOT_BYTES), d(2, rbd.STATE_BYTES), d(1, sim.OUT_BYTES), 1)
    with pytest.raises(ValueError):
        loop.run_device(d(2, stack.ROBOT_BYTES), d(2, rbd.STATE_BYTES), d(2, sim.OUT_BYTES), -1)
    L = N.lib()
    one = d(1, stack.ROBOT_BYTES)
    assert L.lmpc_stack_advance_device(loop.solver._ctx, ctypes.byref(cfg), one.data_ptr(), None, None, 1, None) == -1
    assert L.lmpc_stack_advance_device(loop.solver._ctx, ctypes.byref(cfg), None, None, None, 0, None) == 0
    assert L.lmpc_stack_advance_device(loop.solver._ctx, ctypes.byref(cfg), one.data_ptr(), None, None, -1, None) == -1
    assert L.lmpc_stack_targets_device(one.data_ptr(), one.data_ptr(), 11, ctypes.byref(loop.template), 1,
                                       one.data_ptr(), None) == -1  # stride below 12
    loop.close()
