"""GPU tests of the device loop on the frictional contact model: `stack.StackLoop(..., plant=contact.cfg(...))` and
`sim.WbcSim(..., contact=...)` (include/lmpc/lmpc_contact.h).

Teacher-forced.  4 Go1 trot robots, wbc_per_mpc = 2 at a 5 ms plant step, 12 MPC ticks, as
test_gpu_stack.test_teacher_forced_loop: every logged plant step is recomputed on the host from its logged inputs (the
state before it, the logged tau, the all-ones mask); modes and held bit for bit, the state within test_gpu_contact's
device-vs-host bar of 1e-10; every status 0; 5 + 7 ticks leave the bits of 12.

Standing and trot.  test_gpu_stack's runs on the new plant.  What the trot shows (sliding foot-steps, swing feet that
feel the ground early, touchdown delays, the estimator's velocity error with the force-threshold touch flag) is
printed by every run; the figures of an MI355X run are in DESIGN.md 4h.

Default loop.  With `plant` unset the loop is the sequence of launches it was before the option existed, bit for bit.
"""
import numpy as np
import pytest

from legged_mpc_control_amd import _native as N
from legged_mpc_control_amd import contact, est, rbd, rollout, sim, stack, synth
from test_gpu_sim import standing_cases
from test_gpu_stack import H, lowered, to_host

pytestmark = pytest.mark.gpu

BAR = 1e-10
TROT_SPECS = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.2, -0.1), 0.2), ((-0.2, 0.0), -0.3)]
FALL_SPECS = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.0, 0.15), 0.0), ((0.2, 0.0), 0.3)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.init()
    return torch


def make_loop(states, specs, wbc_per_mpc, sim_dt, gait, plant=None, estimator=None):
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    sts = [rbd.state_from_vector(s) for s in states]
    robots, outs = [], []
    for st, (vd, yr) in zip(sts, specs):
        rb, o = stack.robot_init(cfg, model, st, vd, yr, float(st.pos[2]), gait, 4.0)
        robots.append(rb), outs.append(o)
    loop = stack.StackLoop(model, p, H, len(states), cfg, sim.cfg(dt=sim_dt, ground_z=0.0), wbc_per_mpc,
                           estimator=estimator, plant=plant)
    return loop, robots, sts, outs


def upload(torch, *lists):
    return [torch.from_numpy(stack.to_bytes(x)).cuda() for x in lists]


def f64(a):
    return np.ascontiguousarray(a).view(np.float64)


def couts(log):
    """The logged lmpc_contact_out blocks -> dict of arrays [K][B][...]."""
    raw = log["contact_out"]
    d, i = f64(raw), np.ascontiguousarray(raw).view(np.int32)
    return dict(w=d[..., 0:12], gap=d[..., 12:16], res_primal=d[..., 16], res_dual=d[..., 17], mode=i[..., 36:40],
                sweeps=i[..., 40], polish=i[..., 41], status=i[..., 42])


@pytest.fixture(scope="module")
def forced(gpu):
    md, states, _ = standing_cases()
    plant = contact.cfg(dt=0.005, ground_z=0.0)
    loop, robots, sts, outs = make_loop(lowered(states), TROT_SPECS, 2, 0.005, N.GAIT_TROT, plant)
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 12, log=True))
    gpu.cuda.synchronize()
    final = [x.cpu().numpy() for x in (d_rb, d_st, d_out)]
    yield dict(loop=loop, plant=plant, robots=robots, sts=sts, outs=outs, log=log, final=final)
    loop.close()


def test_teacher_forced_loop(gpu, forced):
    f, log = forced, forced["log"]
    model, plant = f["loop"].model, f["plant"]
    K, B = 24, 4
    co = couts(log)
    assert np.all(log["qp_status"] == 0) and np.all(log["wbc_status"] == 0) and np.all(log["sim_status"] == 0)
    assert np.all(co["status"] == 0) and np.all(log["candidates"] == 1)
    assert np.array_equal(log["mode"], co["mode"])
    assert np.max(co["res_primal"]) <= plant.tol_p and np.max(co["res_dual"]) <= plant.tol_d
    worst = 0.0
    for k in range(K):
        for b in range(B):
            prev = f["sts"][b] if k == 0 else N.LmpcRbdState.from_buffer_copy(log["states"][k - 1, b].tobytes())
            nxt, ho, hc = contact.step(model, plant, prev, log["tau"][k, b], (1, 1, 1, 1))
            assert ho.status == 0 and list(hc.mode) == list(co["mode"][k, b]), f"tick {k} robot {b}"
            assert list(ho.held) == list(log["held"][k, b])
            assert (hc.sweeps, hc.polish) == (co["sweeps"][k, b], co["polish"][k, b])
            hn = np.frombuffer(bytes(nxt), dtype=np.float64)
            worst = max(worst, float(np.max(np.abs(f64(log["states"][k, b]) - hn) / np.maximum(1.0, np.abs(hn)))))
    print(f"teacher-forced on the contact model: plant step, device vs host {worst:.2e} (bar {BAR:.0e}); sweeps "
          f"{np.bincount(co['sweeps'].ravel())}, polish rounds {np.bincount(co['polish'].ravel())}, modes "
          f"{np.bincount(co['mode'].ravel(), minlength=11)}")
    assert worst <= BAR
    assert np.array_equal(f["final"][1], log["states"][-1]) and np.array_equal(f["final"][2], log["out"][-1])


def test_chaining(gpu, forced):
    """5 + 7 MPC ticks leave the bits of 12: robots, state, out and every log."""
    f, loop = forced, forced["loop"]
    d_rb, d_st, d_out = upload(gpu, f["robots"], f["sts"], f["outs"])
    a = to_host(loop.run_device(d_rb, d_st, d_out, 5, log=True))
    b = to_host(loop.run_device(d_rb, d_st, d_out, 7, log=True))
    gpu.cuda.synchronize()
    for x, y in zip((d_rb, d_st, d_out), f["final"]):
        assert np.array_equal(x.cpu().numpy(), y)
    assert a.keys() == f["log"].keys()
    for k, v in f["log"].items():
        assert np.array_equal(np.concatenate([a[k], b[k]]), v), k


def test_standing(gpu):
    """LMPC_GAIT_STAND for 0.1 s at 10 ms / 1.25 ms with the force-threshold touch flag (10 N; a standing Go1 carries
    about 31 N per foot): every foot held, touching and sticking on every tick; test_gpu_stack.test_standing's height
    condition."""
    md, states, _ = standing_cases()
    plant = contact.cfg(dt=0.00125, ground_z=0.0, touch_rule=1, force_threshold=10.0)
    loop, robots, sts, outs = make_loop(lowered(states), [((0.0, 0.0), 0.0)] * 4, 8, 0.00125, N.GAIT_STAND, plant)
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, 10, log=True))
    gpu.cuda.synchronize()
    loop.close()
    co = couts(log)
    assert np.all(log["qp_status"] == 0) and np.all(log["wbc_status"] == 0) and np.all(log["sim_status"] == 0)
    assert np.all(log["held"] == 1) and np.all(log["touch"] == 1)
    assert np.all(co["mode"] == contact.MODE_FREE)
    height = f64(log["states"])[:, :, 5]
    drop = float(np.max(np.abs(height - np.array([s[5] for s in lowered(states)]))))
    free_fall = 0.5 * md["gravity"] * 0.1 ** 2
    print(f"standing on the contact model: trunk height changes by {1e3 * drop:.3f} mm in 0.1 s (free fall "
          f"{1e3 * free_fall:.1f} mm); slip |w| <= {np.max(np.abs(co['w'])):.1e}")
    assert drop < 0.1 * free_fall


@pytest.mark.parametrize("with_estimator", (False, True))
def test_trot(gpu, with_estimator):
    """test_gpu_stack.test_trot_does_not_fall's 50-tick trot (10 ms / 1.25 ms) on the contact model, touch by the force
    threshold (10 N), on the plant's own state and on the estimator's: every status 0, every step certified, and
    test_gpu_stack's fall condition on every logged tick (|roll|, |pitch| < 0.5 rad, trunk above half the commanded
    height).  The contact statistics are printed, not asserted."""
    md, states, _ = standing_cases()
    states = lowered(states)
    T, W = 50, 8
    plant = contact.cfg(dt=0.00125, ground_z=0.0, touch_rule=1, force_threshold=10.0)
    loop, robots, sts, outs = make_loop(states, FALL_SPECS, W, 0.00125, N.GAIT_TROT, plant,
                                        est.cfg(dt=0.00125) if with_estimator else None)
    d_rb, d_st, d_out = upload(gpu, robots, sts, outs)
    log = to_host(loop.run_device(d_rb, d_st, d_out, T, log=True))
    gpu.cuda.synchronize()
    loop.close()
    co = couts(log)
    x = f64(log["states"])
    keys = ("qp_status", "wbc_status", "sim_status") + (("est_status",) if with_estimator else ())
    bad = [int((log[k] != 0).sum()) for k in keys]
    mode, gap = co["mode"], co["gap"]
    sliding = int(np.sum((mode >= 1) & (mode <= 8)))
    sticking = int(np.sum(mode == 0))
    early = int(np.sum((mode < 9) & (gap > 1e-6)))
    rbv = stack.robots_view(log["robots"])
    pc = rbv["plan_contacts"].astype(np.int32)
    delays = []
    for t in range(1, T):
        for b in range(4):
            for l in range(4):
                if pc[t - 1, b, l] == 0 and pc[t, b, l] == 1:
                    t2 = next((u for u in range(t + 1, T) if pc[u, b, l] == 0), T)
                    held = np.flatnonzero(log["held"][t * W:t2 * W, b, l] == 1)
                    if held.size:
                        delays.append(int(held[0]))
    fallen = not (np.all(np.abs(x[:, :, 2]) < 0.5) and np.all(np.abs(x[:, :, 1]) < 0.5) and
                  all(np.all(x[:, b, 5] > 0.5 * states[b][5]) for b in range(4)))
    print(f"trot on the contact model ({'estimate' if with_estimator else 'true state'}): non-zero statuses {bad}; "
          f"foot-steps sticking {sticking}, sliding {sliding}, with a force at a positive gap {early} of {mode.size}; "
          f"touchdown delays {min(delays, default=-1)}..{max(delays, default=-1)} low-level ticks over {len(delays)} "
          f"touchdowns; sweeps {np.bincount(co['sweeps'].ravel())}, polish {np.bincount(co['polish'].ravel())}; "
          f"height {x[:, :, 5].min():.4f}..{x[:, :, 5].max():.4f} m, |roll| <= {np.abs(x[:, :, 2]).max():.3f}, |pitch| <= "
          f"{np.abs(x[:, :, 1]).max():.3f}; fallen: {fallen}")
    if with_estimator:
        ev = np.linalg.norm(f64(log["state_est"])[:, :, 21:24] - x[:, :, 21:24], axis=2)
        print(f"estimator velocity error: median {np.median(ev):.4f}, 90 % {np.percentile(ev, 90):.4f}, 99 % "
              f"{np.percentile(ev, 99):.4f}, max {ev.max():.4f} m/s")
    assert bad == [0] * len(keys)
    assert np.all(co["status"] == 0)
    assert np.max(co["res_primal"]) <= plant.tol_p and np.max(co["res_dual"]) <= plant.tol_d
    assert not fallen  # measured: the robots stay inside test_gpu_stack's fall condition on the contact model
    assert len(delays) >= 1


def test_wbc_sim_on_the_contact_model(gpu):
    """sim.WbcSim(contact=...): standing for 50 ticks, all feet held, the trunk's height kept; with mu = 1e6 and
    use_gap = 0 the run equals the present plant's bit for bit (every foot sticks on every tick)."""
    torch = gpu
    md, states, targets = standing_cases()
    model = rbd.model_go1()
    tg = torch.from_numpy(rbd.pack([rbd.target(**t) for t in targets])).cuda()
    finals = []
    for c in (None, contact.cfg(dt=0.002, ground_z=0.0, mu=1e6, use_gap=0), contact.cfg(dt=0.002, ground_z=0.0)):
        ws = sim.WbcSim(model, 4, sim.cfg(dt=0.002, ground_z=0.0), contact=c)
        d_state = torch.from_numpy(rbd.pack([rbd.state_from_vector(s) for s in states])).cuda()
        log = ws.run_device(d_state, tg, 50, log=True)
        torch.cuda.synchronize()
        assert np.all(log["sim_status"].cpu().numpy() == 0) and np.all(log["held"].cpu().numpy() == 1)
        finals.append(d_state.cpu().numpy())
        ws.close()
    assert np.array_equal(finals[0], finals[1])
    drop = float(np.max(np.abs(f64(finals[2])[:, 5] - np.array([s[5] for s in states]))))
    assert drop < 0.1 * 0.5 * md["gravity"] * 0.1 ** 2


def test_default_loop_unchanged(gpu):
    """Without `plant` the loop is the sequence of launches it was before the option existed -- written out here from
    the public device functions -- bit for bit, before and after a contact-model loop has run in the process."""
    torch = gpu
    md, states, _ = standing_cases()
    states = lowered(states)
    T, W = 3, 2

    def default_run():
        loop, robots, sts, outs = make_loop(states, TROT_SPECS, W, 0.005, N.GAIT_TROT)
        d_rb, d_st, d_out = upload(torch, robots, sts, outs)
        log = to_host(loop.run_device(d_rb, d_st, d_out, T, log=True))
        torch.cuda.synchronize()
        loop.close()
        return log, [x.cpu().numpy() for x in (d_rb, d_st, d_out)]

    def by_hand():
        loop, robots, sts, outs = make_loop(states, TROT_SPECS, W, 0.005, N.GAIT_TROT)
        d_rb, d_st, d_out = upload(torch, robots, sts, outs)
        s = torch.cuda.current_stream()
        d_grf = torch.zeros((4, H, 12), dtype=torch.float64, device="cuda")
        d_tg = torch.zeros((4, rbd.TARGET_BYTES), dtype=torch.uint8, device="cuda")
        d_cand = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
        taus, cands = [], []
        for t in range(T):
            stack.advance_device(loop.solver, loop.rollout_cfg, d_rb, d_st, d_out, s)
            stack.solve_device(loop.solver, d_grf, None, None, s)
            stack.targets_device(d_rb, d_grf, loop.template, d_tg, s)
            for i in range(W):
                stack.candidates_device(d_out, d_cand, s)
                d_x, _ = loop.pipeline.solve_device(d_st, d_tg, s)
                d_tau = d_x[:, sim.TAU_OFFSET:sim.TAU_OFFSET + 12]
                sim.step_device(loop.model, loop.sim_cfg, d_st, d_tau, d_cand, d_st, d_out, 1, s)
                taus.append(d_tau.cpu().numpy().copy()), cands.append(d_cand.cpu().numpy().copy())
        torch.cuda.synchronize()
        loop.close()
        return np.stack(taus), np.stack(cands), [x.cpu().numpy() for x in (d_rb, d_st, d_out)]

    first, first_final = default_run()
    assert "contact_out" not in first and "mode" not in first
    taus, cands, hand_final = by_hand()
    assert np.array_equal(first["tau"], taus) and np.array_equal(first["candidates"], cands)
    for x, y in zip(first_final, hand_final):
        assert np.array_equal(x, y)
    cloop, robots, sts, outs = make_loop(states, TROT_SPECS, W, 0.005, N.GAIT_TROT, contact.cfg(dt=0.005))
    cloop.run_device(*upload(torch, robots, sts, outs), T)
    torch.cuda.synchronize()
    cloop.close()
    again, again_final = default_run()
    assert first.keys() == again.keys()
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    for x, y in zip(first_final, again_final):
        assert np.array_equal(x, y)


def test_loop_argument_checks(gpu):
    p, rcfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 2, rcfg, sim.cfg(dt=0.005), 2, plant=contact.cfg(dt=0.00125))  # not sim_cfg's dt
    with pytest.raises(ValueError):
        stack.StackLoop(model, p, H, 2, rcfg, sim.cfg(dt=0.005, ground_z=0.0), 2, plant=contact.cfg(dt=0.005, ground_z=0.1))
