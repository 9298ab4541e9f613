"""GPU tests of the hierarchical QP's warm start (lmpc_hoqp.hip, warm instantiation, through
lmpc_hoqp_solve_batch_warm / lmpc_hoqp_solve_device_warm; DESIGN.md 4c "Warm start").

The bar is tests/test_gpu_hoqp.py's: `check_against` at TOL = 1e-6 against the CPU restatement's answers
(tests/golden/hoqp_golden.npz; tests/golden/hoqp_warm_golden.npz for the tick pairs, made by tools/hoqp_warm_proto.py).
A carried active set may cost time, never the answer: every warm result is held to the same check as the cold one.
Iteration word: bits 0-15 interior-point iterations, 16-17 crossover (1 tried, 3 taken), 18 carried set tried, 19 taken,
20-23 its repair rounds.  Measured differences are printed; DESIGN.md 4c quotes them."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_hoqp import TOL, check_against, dims_from, load

pytestmark = pytest.mark.gpu

GROUPS = ["wbc", "rand3", "n20", "n64", "exhaust", "ref"]
TRIED, TAKEN = 1 << 18, 1 << 19


@pytest.fixture(scope="module")
def hq():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.init()
    from legged_mpc_control_amd import hoqp

    return hoqp


@pytest.fixture(scope="module")
def cold(hq):
    """Every golden group solved once by the cold entry point: (group dict, dims, x, w, status, iters), shared."""
    out = {}
    for group in GROUPS:
        g = load(group)
        dims = dims_from(g["dims"])
        solver = hq.HoqpBatch(dims, g["rec"].shape[0])
        out[group] = (g, dims) + tuple(solver.solve(g["rec"]))
        solver.close()
    return out


def pairs():
    return np.load(os.path.join(GOLDEN, "hoqp_warm_golden.npz"), allow_pickle=False)


def check_group(g, dims, x, w):
    for b in range(g["rec"].shape[0]):
        check_against(g["rec"][b], dims, x[b], w[b], g["x"][b], g["w"][b], bool(g["pinned"]), TOL)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(b))))


@pytest.mark.parametrize("group", GROUPS)
def test_zero_block_is_the_cold_solve(hq, cold, group):
    """A zero-filled block = no set: the warm instantiation returns the cold one's bits, and tries nothing."""
    g, dims, x0, w0, st0, it0 = cold[group]
    B = g["rec"].shape[0]
    solver = hq.HoqpBatch(dims, B)
    x, w, st, it, act = solver.solve(g["rec"], act=np.zeros((B, solver.act_len), dtype=np.int64))
    assert np.array_equal(x, x0) and np.array_equal(w, w0) and np.array_equal(st, st0)
    assert np.array_equal(it, it0) and not np.any(it & (TRIED | TAKEN))
    # written back: valid exactly where the level's crossover verified
    valid = act.reshape(B, dims.num_levels, 5)[:, :, 0]
    assert np.array_equal(valid == 1, ((it >> 16) & 3) == 3) and np.all((valid == 0) | (valid == 1))
    solver.close()


@pytest.mark.parametrize("group", GROUPS)
def test_second_solve_of_the_same_records(hq, cold, group):
    g, dims, x0, w0, st0, it0 = cold[group]
    B = g["rec"].shape[0]
    solver = hq.HoqpBatch(dims, B)
    _, _, _, _, act = solver.solve(g["rec"], act=np.zeros((B, solver.act_len), dtype=np.int64))
    x, w, st, it, act2 = solver.solve(g["rec"], act=act)
    check_group(g, dims, x, w)
    assert np.array_equal(st, st0)
    verified = ((it0 >> 16) & 3) == 3
    taken = (it & TAKEN) != 0
    assert np.array_equal((it & TRIED) != 0, verified)  # a set is carried exactly where the cold crossover verified
    assert np.all((it[taken] & 0xFFFF) == 0) and np.all(((it[taken] >> 16) & 3) == 3)
    rounds = (it[taken] >> 20) & 15
    print(f"{group}: {int(taken.sum())} of {int(verified.sum())} carried sets taken ({verified.size} levels), repair rounds "
          f"mean {rounds.mean() if rounds.size else 0:.2f} max {rounds.max() if rounds.size else 0}; warm vs cold final x "
          f"{rel(x[:, -1], x0[:, -1]):.1e}, slacks {float(np.max(np.abs(w - w0))) if w.size else 0:.1e}")
    if group == "wbc":
        # 16 chains, 48 levels: tools/hoqp_warm_proto.py --golden-wbc takes all 48 on the CPU
        assert verified.all() and taken.all(), np.argwhere(~taken).tolist()
    solver.close()


def test_next_tick(hq):
    """Tick A cold seeds the blocks, tick B (1 % later; pairs 8-11 with another contact pattern) is solved from them."""
    g = pairs()
    dims = dims_from(g["dims"])
    solver = hq.HoqpBatch(dims, 12)
    xa, wa, sta, ita, act = solver.solve(g["rec_a"], act=np.zeros((12, solver.act_len), dtype=np.int64))
    assert np.all(sta == 0) and np.all(((ita >> 16) & 3) == 3)
    xb, wb, stb, itb, _ = solver.solve(g["rec_b"], act=act)
    xc, wc, stc, _ = solver.solve(g["rec_b"])
    for k in range(12):
        check_against(g["rec_a"][k], dims, xa[k], wa[k], g["x_a"][k], g["w_a"][k], True, TOL)
        check_against(g["rec_b"][k], dims, xb[k], wb[k], g["x_b"][k], g["w_b"][k], True, TOL)
    assert np.all(stb == 0) and np.all(stc == 0)
    taken, tried = (itb & TAKEN) != 0, (itb & TRIED) != 0
    print(f"next tick: warm vs oracle final x {rel(xb[:, -1], g['x_b'][:, -1]):.1e}, warm vs cold {rel(xb[:, -1], xc[:, -1]):.1e}, "
          f"slacks warm vs cold {float(np.max(np.abs(wb - wc))):.1e}; same contacts {int(taken[:8].sum())} of 24 levels "
          f"taken (rounds max {int(((itb[:8] >> 20) & 15).max())}), changed contacts {int(taken[8:].sum())} of 12")
    assert taken[:8].all(), np.argwhere(~taken[:8]).tolist()
    assert np.all((itb[:8] & 0xFFFF) == 0)
    # contact change: taken, or tried and then solved cold
    assert tried[8:].all()
    assert np.all(taken[8:] | ((itb[8:] & 0xFFFF) > 0))
    solver.close()


@pytest.mark.parametrize("group", GROUPS)
def test_garbage_in(hq, cold, group):
    """Seeded random flags, every level marked valid: the answers are the cold ones."""
    g, dims, x0, w0, st0, it0 = cold[group]
    B = g["rec"].shape[0]
    solver = hq.HoqpBatch(dims, B)
    rng = np.random.default_rng(20261020)
    act = rng.integers(0, 2 ** 63, size=(B, dims.num_levels, 5), dtype=np.int64)
    act[:B // 2] |= rng.integers(0, 2 ** 63, size=(B // 2, dims.num_levels, 5), dtype=np.int64)  # denser sets too
    act[:, :, 0] = 1
    x, w, st, it, _ = solver.solve(g["rec"], act=act.reshape(B, -1))
    check_group(g, dims, x, w)
    if group in ("wbc", "n64"):
        assert np.array_equal(st, st0)
    assert np.all(st <= 1)
    crossed = (dims_rows(dims) > 0)[None, :]  # a level without inequality rows above or of its own has no crossover
    assert np.array_equal((it & TRIED) != 0, np.broadcast_to(crossed, it.shape))
    print(f"{group}: {int(((it & TAKEN) != 0).sum())} of {it.size} garbage sets repaired and taken; vs cold final x "
          f"{rel(x[:, -1], x0[:, -1]):.1e}")
    solver.close()


def dims_rows(dims):
    return np.cumsum([dims.ineq_rows[l] for l in range(dims.num_levels)])


def test_device_path_batch_position_and_guards(hq):
    """Device path == host path bit for bit; a chain alone == first == last == middle of 17 with its own block, bit for
    bit in x, w and act; the guard words after each tensor stay."""
    import torch

    g = pairs()
    dims = dims_from(g["dims"])
    solver = hq.HoqpBatch(dims, 17)
    L, n, AL = dims.num_levels, dims.num_vars, solver.act_len
    # blocks of all 12 pairs from tick A; the probe chain is pair 4 (a repair round on level 1)
    _, _, _, _, act_a = solver.solve(g["rec_a"], act=np.zeros((12, AL), dtype=np.int64))
    probe, pa = g["rec_b"][4], act_a[4]
    x1, w1, st1, it1, a1 = solver.solve(probe[None], act=pa[None])
    assert it1[0, 0] & TAKEN
    others = np.concatenate([g["rec_b"], g["rec_a"][:5]])
    others_act = np.concatenate([act_a, np.zeros((5, AL), dtype=np.int64)])
    for pos in (0, 8, 16):
        rec, act = others.copy(), others_act.copy()
        rec[pos], act[pos] = probe, pa
        x, w, st, it, a = solver.solve(rec, act=act)
        assert np.array_equal(x[pos], x1[0]) and np.array_equal(w[pos], w1[0]) and np.array_equal(a[pos], a1[0])
        assert st[pos] == st1[0] and np.array_equal(it[pos], it1[0])
    # device path with guard words
    G = 8
    def guarded(shape, dtype, fill):
        flat = torch.full((int(np.prod(shape)) + G,), fill, dtype=dtype, device="cuda")
        return flat, flat[:int(np.prod(shape))].view(*shape)
    fx, d_x = guarded((17, L, n), torch.float64, 7.5)
    fw, d_w = guarded((17, 44), torch.float64, 7.5)
    fs, d_st = guarded((17,), torch.int32, -7)
    fi, d_it = guarded((17, L), torch.int32, -7)
    fa, d_act = guarded((17, AL), torch.int64, 0x5A5A5A5A)
    d_act.copy_(torch.from_numpy(act))
    d_rec = torch.from_numpy(rec).cuda()
    solver.solve_device(d_rec, d_x, d_w, d_st, d_it, d_act=d_act)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy(), x) and np.array_equal(d_w.cpu().numpy(), w)
    assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_it.cpu().numpy(), it)
    assert np.array_equal(d_act.cpu().numpy(), a)
    for flat, fill in ((fx, 7.5), (fw, 7.5), (fs, -7), (fi, -7), (fa, 0x5A5A5A5A)):
        assert torch.all(flat[-G:] == fill)
    with pytest.raises(ValueError):
        solver.solve_device(d_rec, d_x, d_w, d_st, d_it, d_act=d_act.to(torch.int32))
    with pytest.raises(ValueError):
        solver.solve_device(d_rec, d_x, d_w, d_st, d_it, d_act=d_act[:, :AL - 1].contiguous())
    solver.close()


def test_nan_chain_leaves_no_set_and_spares_its_neighbours(hq, cold):
    g, dims, x0, w0, st0, it0 = cold["wbc"]
    B = g["rec"].shape[0]
    solver = hq.HoqpBatch(dims, B)
    _, _, _, _, act = solver.solve(g["rec"], act=np.zeros((B, solver.act_len), dtype=np.int64))
    x1, w1, st1, it1, act1 = solver.solve(g["rec"], act=act)
    bad = g["rec"].copy()
    poisoned = {3: (100, np.nan), 7: (4465, np.nan), 9: (2000, np.inf)}  # level 0 a, level 2 b, level 0 d
    for b, (i, v) in poisoned.items():
        bad[b, i] = v
    x, w, st, it, act2 = solver.solve(bad, act=act)
    keep = np.array([b not in poisoned for b in range(B)])
    for b in poisoned:
        assert st[b] == 2 and np.all(x[b] == 0.0) and np.all(w[b] == 0.0) and np.all(act2[b] == 0), b
    assert np.all(st[keep] == 0)
    assert np.array_equal(x[keep], x1[keep]) and np.array_equal(w[keep], w1[keep])
    assert np.array_equal(act2[keep], act1[keep]) and np.array_equal(it[keep], it1[keep])
    solver.close()


def test_two_streams_of_one_context_are_ordered(hq):
    """Two warm calls on two streams share the context's scratch and here also the blocks: the second starts after the
    first, so it finds the sets the first wrote."""
    import torch

    g = pairs()
    dims = dims_from(g["dims"])
    solver = hq.HoqpBatch(dims, 12)
    xr, wr, _, itr, actr = solver.solve(g["rec_a"], act=np.zeros((12, solver.act_len), dtype=np.int64))
    xs, ws, _, its, acts = solver.solve(g["rec_b"], act=actr)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_a, d_b = torch.from_numpy(g["rec_a"]).cuda(), torch.from_numpy(g["rec_b"]).cuda()
    d_act = torch.zeros((12, solver.act_len), dtype=torch.int64, device="cuda")
    mk = lambda: (torch.zeros((12, 3, 42), dtype=torch.float64, device="cuda"),
                  torch.zeros((12, 44), dtype=torch.float64, device="cuda"),
                  torch.zeros(12, dtype=torch.int32, device="cuda"), torch.zeros((12, 3), dtype=torch.int32, device="cuda"))
    o1, o2 = mk(), mk()
    torch.cuda.synchronize()
    solver.solve_device(d_a, *o1, stream=s1, d_act=d_act)
    solver.solve_device(d_b, *o2, stream=s2, d_act=d_act)
    torch.cuda.synchronize()
    assert np.array_equal(o1[0].cpu().numpy(), xr) and np.array_equal(o1[3].cpu().numpy(), itr)
    assert np.array_equal(o2[0].cpu().numpy(), xs) and np.array_equal(o2[1].cpu().numpy(), ws)
    assert np.array_equal(o2[3].cpu().numpy(), its) and np.array_equal(d_act.cpu().numpy(), acts)
    solver.close()


@pytest.fixture(scope="module")
def alone(hq):
    """The tick pairs' records solved alone, each by a context of its own that does nothing else: tick A, tick B, and
    tick B twice over (24 chains).  (dims, x, w, status, iters) per key; the ordering tests hold every result to these
    bits."""
    g = pairs()
    dims = dims_from(g["dims"])
    out = {}
    for key, rec in (("a", g["rec_a"]), ("b", g["rec_b"]), ("bb", np.concatenate([g["rec_b"], g["rec_b"]]))):
        solver = hq.HoqpBatch(dims, rec.shape[0])
        out[key] = tuple(solver.solve(rec))
        solver.close()
    return dims, out


def device_outputs(torch, B):
    return (torch.zeros((B, 3, 42), dtype=torch.float64, device="cuda"), torch.zeros((B, 44), dtype=torch.float64, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros((B, 3), dtype=torch.int32, device="cuda"))


def same_bits(outs, ref):
    return all(np.array_equal(o.cpu().numpy() if hasattr(o, "cpu") else o, r) for o, r in zip(outs, ref))


def test_stream_gone_before_the_next_call(hq, alone):
    """test_gpu_parity.py's test of the same name, for the hierarchical QP's context: a device-path solve on a caller's
    stream A leaves nothing recorded on A.  With A destroyed right after the call (its solve may still run), the next
    host-pointer solve, lmpc_hoqp_sync and lmpc_hoqp_destroy wait for the device instead of touching A: no crash, and
    every result equals the same solve run alone."""
    import ctypes

    import torch

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    g = pairs()
    dims, ref = alone
    d_a = torch.from_numpy(g["rec_a"]).cuda()
    for after in ("host", "sync", "close"):
        t = hq.HoqpBatch(dims, 12)
        a = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(a), 1) == 0  # hipStreamNonBlocking
        outs = device_outputs(torch, 12)
        torch.cuda.synchronize()
        t.solve_device(d_a, *outs, stream=torch.cuda.ExternalStream(a.value))  # returns at once
        assert hip.hipStreamDestroy(a) == 0                                     # the caller's stream is gone
        if after == "host":
            assert same_bits(t.solve(g["rec_b"]), ref["b"])  # waits for the device, never for A
        elif after == "sync":
            assert t._L.lmpc_hoqp_sync(t._ctx) == 0
        t.close()
        torch.cuda.synchronize()
        assert same_bits(outs, ref["a"]), after


def test_scratch_growth_with_a_launch_pending(hq, alone):
    """A context made for 12 chains: 12 on stream A, then 24 on stream B.  The second call grows the scratch, and the
    old block is the one the first launch may still be working in: both results equal the solves run alone."""
    import torch

    g = pairs()
    dims, ref = alone
    solver = hq.HoqpBatch(dims, 12)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_a = torch.from_numpy(g["rec_a"]).cuda()
    d_bb = torch.from_numpy(np.concatenate([g["rec_b"], g["rec_b"]])).cuda()
    o1, o2 = device_outputs(torch, 12), device_outputs(torch, 24)
    torch.cuda.synchronize()
    solver.solve_device(d_a, *o1, stream=sa)
    solver.solve_device(d_bb, *o2, stream=sb)
    torch.cuda.synchronize()
    assert same_bits(o1, ref["a"]) and same_bits(o2, ref["bb"])
    solver.close()


def test_host_path_behind_a_device_call_on_another_stream(hq, alone):
    """A device-path solve on a caller's stream, then at once a host-pointer solve (the context's own stream): they
    share the scratch, so the second waits for the first; both results equal the solves run alone."""
    import torch

    g = pairs()
    dims, ref = alone
    solver = hq.HoqpBatch(dims, 12)
    sa = torch.cuda.Stream()
    d_a = torch.from_numpy(g["rec_a"]).cuda()
    o1 = device_outputs(torch, 12)
    torch.cuda.synchronize()
    solver.solve_device(d_a, *o1, stream=sa)
    assert same_bits(solver.solve(g["rec_b"]), ref["b"])
    torch.cuda.synchronize()
    assert same_bits(o1, ref["a"])
    solver.close()


def test_closed_loop_wbc_sim(hq):
    """WbcSim(warm=True), 4 standing Go1 robots, 10 ticks: every tick re-solved cold from the logged state."""
    import torch

    from legged_mpc_control_amd import rbd, sim
    from test_gpu_sim import standing_cases

    md, states, targets = standing_cases()
    model = rbd.model_go1()
    ws = sim.WbcSim(model, 4, sim.cfg(dt=0.002, ground_z=0.0), warm=True)
    ref = rbd.WbcPipeline(model, 4)
    d_target = torch.from_numpy(rbd.pack([rbd.target(**t) for t in targets])).cuda()
    first = rbd.pack([rbd.state_from_vector(s) for s in states])
    d_state = torch.from_numpy(first.copy()).cuda()
    log = {k: v.cpu().numpy() for k, v in ws.run_device(d_state, d_target, 10, log=True).items()}
    assert np.all(log["wbc_status"] == 0) and np.all(log["sim_status"] == 0)
    worst = 0.0
    for t in range(10):
        before = first if t == 0 else log["states"][t - 1]
        d_x, d_st = ref.solve_device(torch.from_numpy(before.copy()).cuda(), d_target)
        torch.cuda.synchronize()
        assert np.all(d_st.cpu().numpy() == 0)
        assert not np.any(ref.d_iters.cpu().numpy() & (TRIED | TAKEN))
        xc = d_x.cpu().numpy()
        for b in range(4):
            worst = max(worst, rel(log["x"][t, b], xc[b]))
    it = log["wbc_iters"]
    assert not np.any(it[0] & TRIED)
    share = float(((it[1:] & TAKEN) != 0).mean())
    print(f"WbcSim warm: warm vs cold x over 10 ticks {worst:.1e}; from the second tick {100 * share:.1f} % of levels taken "
          f"warm, {100 * float(((it[1:] & TRIED) != 0).mean()):.1f} % tried")
    assert worst <= TOL
    # reset_warm: the next tick is a cold one again
    ws.pipeline.reset_warm()
    ws.run_device(d_state, d_target, 1)
    torch.cuda.synchronize()
    assert not np.any(ws.pipeline.d_iters.cpu().numpy() & TRIED)
    ws.close()
    ref.close()


def trot(gpu, wbc_warm, T=50, W=8):
    from legged_mpc_control_amd import _native as N
    from legged_mpc_control_amd import rbd, rollout, sim, stack, synth
    from test_gpu_sim import standing_cases
    from test_gpu_stack import H, lowered

    md, states, _ = standing_cases()
    states = lowered(states)
    specs = [((0.0, 0.0), 0.0), ((0.3, 0.0), 0.0), ((0.0, 0.15), 0.0), ((0.2, 0.0), 0.3)]  # test_gpu_stack's trot
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    sts = [rbd.state_from_vector(s) for s in states]
    robots, outs = [], []
    for st, (vd, yr) in zip(sts, specs):
        rb, o = stack.robot_init(cfg, model, st, vd, yr, float(st.pos[2]), N.GAIT_TROT, 4.0)
        robots.append(rb)
        outs.append(o)
    loop = stack.StackLoop(model, p, H, 4, cfg, sim.cfg(dt=0.00125, ground_z=0.0), W, wbc_warm=wbc_warm)
    d_rb, d_st, d_out = [gpu.from_numpy(stack.to_bytes(v)).cuda() for v in (robots, sts, outs)]
    log = {k: v.cpu().numpy() for k, v in loop.run_device(d_rb, d_st, d_out, T, log=True).items()}
    gpu.cuda.synchronize()
    loop.close()
    return states, log


def test_trot_with_warm_wbc(hq):
    """test_gpu_stack's four trotting robots, 50 MPC ticks, the WBC warm: nobody falls (that test's condition), every
    status 0.  The same loop with wbc_warm=False (10 ticks) logs no bit 18 or 19."""
    import torch

    states, log = trot(torch, True)
    bad = [int((log[k] != 0).sum()) for k in ("qp_status", "wbc_status", "sim_status")]
    assert bad == [0, 0, 0]
    x = log["states"].view(np.float64)
    assert np.all(np.abs(x[:, :, 2]) < 0.5) and np.all(np.abs(x[:, :, 1]) < 0.5)
    for b in range(4):
        assert np.all(x[:, b, 5] > 0.5 * states[b][5])
    it = log["wbc_iters"]
    assert it.shape == (400, 4, 3)
    taken, tried = (it[1:] & TAKEN) != 0, (it[1:] & TRIED) != 0
    rounds = (it[1:][taken] >> 20) & 15
    print(f"trot, WBC warm: {100 * taken.mean():.1f} % of levels taken warm after the first tick ({100 * tried.mean():.1f} % "
          f"tried), per level {[round(100 * float(v), 1) for v in taken.mean(axis=(0, 1))]}, repair rounds mean "
          f"{rounds.mean():.2f} max {rounds.max()}")
    assert not np.any(it[0] & TRIED)
    _, cold_log = trot(torch, False, T=10)
    assert cold_log["wbc_iters"].shape == (80, 4, 3)
    assert not np.any(cold_log["wbc_iters"] & (TRIED | TAKEN))
