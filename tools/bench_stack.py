#!/usr/bin/env python3
"""Benchmark of the full loop (include/lmpc/lmpc_stack.h: MPC -> WBC -> rigid-body plant) on MI355X.

    python tools/bench_stack.py [--ticks T] [--repeats R] [--out FILE] [--wbc-warm] [--batches 1024,4096] [--whole-only]
                                [--low-level [--fused]]

1024 and 4096 Go1 trot robots from a standing pose with seeded commands, H = 10, the reference's rates (10 ms MPC tick,
8 low-level ticks of 1.25 ms).  One HIP event pair around a whole `StackLoop.run_device` of T MPC ticks, after a
warm-up run from the same start; the best of R repeats.  In the same process, from the same start:

    solve_only   the T ticks' commands (logged by the warm-up run) through lmpc_solve_commands_device alone, one call
                 per tick -- tools/bench_rollout.py's solve-only tick
    wbc_sim      the 8 T low-level ticks replayed: what one sim.WbcSim tick does (WbcPipeline.solve_device, then
                 lmpc_sim_step_device) on the logged state, targets and candidates of each tick.  The hierarchical
                 solve's time depends on its data, so the parts run on the loop's own data, not on constant targets.

glue_us_per_mpc_tick = the whole - solve_only - the 8 replayed wbc_sim ticks: the advance launch (which also expands
the records), the targets launch and the 8 candidate launches, with their host calls.  Prints ONE JSON line.

--wbc-warm: `StackLoop(..., wbc_warm=True)`, every timed run from zeroed active-set blocks; the row gains `wbc_warm`:
the share of WBC levels tried and taken warm after the first low-level tick, the mean repair rounds of the taken ones
and the mean interior-point iterations per level, from the warm-up run's `wbc_iters`.  --whole-only: the whole loop's
time alone (the A/B of the option needs no parts).

--low-level: `StackLoop(..., low_level=lowlevel.cfg_go1(model))`, the reference's joint-PD controller in place of the
WBC, beside the WBC loop of the same build from the same start in ALTERNATING timed runs (WBC, low-level, WBC, ...; the
best of R each).  The row's `lowlevel` holds the whole MPC tick, solve_only as above, and the 8 T low-level ticks
replayed on the loop's own logged data in two parts: `controller` (lmpc_lowlevel_device with the candidates, one launch)
and `plant` (lmpc_sim_step_device reading the logged torques), with the controller's share of the two; `wbc` holds the
WBC loop's whole tick.  The trot's height / roll / pitch bands of both loops come from their warm-up runs.

--low-level --fused: `StackLoop(..., low_level=..., fused_low_level=True)` (include/lmpc/lmpc_lowsim.h: the 8 low-level
ticks of an MPC tick as one launch) beside the unfused joint-PD loop of the same build from the same start, in
ALTERNATING timed runs (unfused, fused, unfused, ...; R each).  The row holds both loops' best whole MPC tick, every
single run (`runs_ms_per_mpc_tick`: the unfused runs' spread is the noise the gain is held against), whether the two
loops' final buffers are bytewise equal, and the low-level ticks alone replayed on the unfused loop's logged data:
`fused_launch_us_per_mpc_tick` (lmpc_lowsim_run_device, one launch per MPC tick) against `unfused_launches_us_per_mpc_tick`
(its 8 controller + 8 plant launches).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

BATCHES = (1024, 4096)
H, WBC_PER_MPC, SIM_DT = 10, 8, 0.00125


def timed(fn, repeats):
    import torch

    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def start_of(batch, seed):
    """Standing Go1 robots (joints 0, 0.8, -1.6; the feet on the ground) at seeded places and headings, with seeded
    commands -> (robots, states, first outs) as uint8 arrays."""
    from legged_mpc_control_amd import _native as N, rbd, rollout, stack

    rng = np.random.default_rng(seed)
    cfg, model = rollout.cfg_go1(), rbd.model_go1()
    s = np.zeros(36)
    s[6:18] = np.tile([0.0, 0.8, -1.6], 4)
    z = -rbd.terms_dict(rbd.compute(model, rbd.state_from_vector(s)))["foot_pos"][2]
    robots, states, outs = [], [], []
    for _ in range(batch):
        s[0] = rng.uniform(-3.0, 3.0)
        s[3:6] = [rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), z]
        st = rbd.state_from_vector(s)
        rb, o = stack.robot_init(cfg, model, st, (rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)),
                                 rng.uniform(-0.3, 0.3), z, N.GAIT_TROT, 4.0)
        robots.append(rb)
        states.append(st)
        outs.append(o)
    return tuple(stack.to_bytes(x) for x in (robots, states, outs))


def bands(x):
    """[K][B][36] states -> the trot's height / roll / pitch bands over every robot and tick."""
    f = lambda t: float(t)
    return dict(height=[f(x[:, :, 5].min()), f(x[:, :, 5].max())], roll=[f(x[:, :, 2].min()), f(x[:, :, 2].max())],
                pitch=[f(x[:, :, 1].min()), f(x[:, :, 1].max())])


def fallen_count(x):
    return int(((x[:, :, 1].abs() > 0.5) | (x[:, :, 2].abs() > 0.5) | (x[:, :, 5] < 0.5 * x[0, :, 5])).any(dim=0).sum())


def low_level_rows(args):
    """--low-level: the joint-PD loop beside the WBC loop, alternating runs, and the low-level tick's two parts."""
    import torch

    from legged_mpc_control_amd import BatchedConvexQPSolver, est, lowlevel, rbd, rollout, sim, stack, synth

    dev = torch.device("cuda:0")
    T, W = args.ticks, WBC_PER_MPC
    rows = []
    for batch in [int(b) for b in args.batches.split(",")]:
        p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
        sc = sim.cfg(dt=SIM_DT, ground_z=0.0)
        ll_cfg = lowlevel.cfg_go1(model)
        wbc = stack.StackLoop(model, p, H, batch, cfg, sc, W)
        ll = stack.StackLoop(model, p, H, batch, cfg, sc, W, low_level=ll_cfg)
        start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
        bufs = [a.clone() for a in start]
        wlog = wbc.run_device(*bufs, T, log=True)  # warm-up runs, and the records of what the loops do
        xw = wlog["states"].view(torch.float64)
        row = dict(batch=batch, H=H, mpc_ticks=T, wbc_per_mpc=W, dense_path=ll.solver.dense_path)
        row["wbc"] = dict(nonzero_status=dict(qp=int((wlog["qp_status"] != 0).sum()), wbc=int((wlog["wbc_status"] != 0).sum()),
                                              sim=int((wlog["sim_status"] != 0).sum())),
                          fallen=fallen_count(xw), bands=bands(xw))
        del wlog, xw
        for d, s in zip(bufs, start):
            d.copy_(s)
        log = ll.run_device(*bufs, T, log=True)
        torch.cuda.synchronize()
        x = log["states"].view(torch.float64)
        row["lowlevel"] = dict(nonzero_status=dict(qp=int((log["qp_status"] != 0).sum()),
                                                   nonfinite_tau=int((log["ll_flags"] & lowlevel.TAU_NONFINITE != 0).sum()),
                                                   sim=int((log["sim_status"] != 0).sum())),
                               flag_words=sorted(int(v) for v in torch.unique(log["ll_flags"]).cpu()),
                               fallen=fallen_count(x), bands=bands(x), kp=ll_cfg.kp[0][0], kd=ll_cfg.kd[0][0])

        def whole(loop):
            def run():
                for d, s in zip(bufs, start):
                    d.copy_(s)
                loop.run_device(*bufs, T)
            return run

        ms_w = ms_l = float("inf")
        for _ in range(args.repeats):  # alternating: a drift of the box hits both loops alike
            ms_w = min(ms_w, timed(whole(wbc), 1))
            ms_l = min(ms_l, timed(whole(ll), 1))
        row["wbc"]["whole"] = dict(ms_per_mpc_tick=ms_w / T, robot_ticks_per_s=batch * T / (ms_w * 1e-3))
        row["lowlevel"]["whole"] = dict(ms_per_mpc_tick=ms_l / T, robot_ticks_per_s=batch * T / (ms_l * 1e-3))
        cmds = log["cmd"].contiguous()
        grf = torch.empty((batch, H, 12), dtype=torch.float64, device=dev)
        solver = BatchedConvexQPSolver(p, H, max_batch=0)

        def solve_only():
            for t in range(T):
                solver.solve_commands_device(cmds[t], grf)

        solve_only()
        torch.cuda.synchronize()
        ms_solve = timed(solve_only, args.repeats)
        K = W * T
        prev = [start[1]] + [log["states"][k] for k in range(K - 1)]
        prev_out = [start[2]] + [log["out"][k] for k in range(K - 1)]
        gait = log["robots"].view(torch.int32)[:, :, est.GAIT_OFFSET]  # [T][B], the robots' stride
        d_ll = torch.empty((batch, lowlevel.OUT_BYTES), dtype=torch.uint8, device=dev)
        d_cand = torch.empty((batch, 4), dtype=torch.int32, device=dev)
        d_next, d_o = torch.empty_like(start[1]), torch.empty_like(start[2])

        def controller():
            for k in range(K):
                lowlevel.lowlevel_device(ll_cfg, prev[k], log["target"][k // W], d_ll, gait[k // W], prev_out[k], d_cand)

        def plant():
            for k in range(K):
                sim.step_device(model, sc, prev[k], lowlevel.tau_view(log["ll_out"][k]), log["candidates"][k], d_next,
                                d_o, 1)

        parts = {}
        for name, fn in (("controller", controller), ("plant", plant)):
            fn()
            torch.cuda.synchronize()
            parts[name] = 1e3 * timed(fn, args.repeats) / K
        row["lowlevel"].update(solve_only=dict(ms_per_tick=ms_solve / T), controller_us_per_tick=parts["controller"],
                               plant_us_per_tick=parts["plant"],
                               controller_share_of_low_level_tick=parts["controller"] / (parts["controller"] + parts["plant"]),
                               glue_us_per_mpc_tick=1e3 * (ms_l - ms_solve) / T - W * (parts["controller"] + parts["plant"]))
        rows.append(row)
        solver.close()
        wbc.close()
        ll.close()
    return rows


def fused_rows(args):
    """--low-level --fused: the fused joint-PD loop beside the unfused one, alternating runs, and the low-level ticks of
    an MPC tick alone in both forms."""
    import torch

    from legged_mpc_control_amd import est, lowlevel, lowsim, rbd, rollout, sim, stack, synth

    dev = torch.device("cuda:0")
    T, W = args.ticks, WBC_PER_MPC
    rows = []
    for batch in [int(b) for b in args.batches.split(",")]:
        p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
        sc = sim.cfg(dt=SIM_DT, ground_z=0.0)
        ll_cfg = lowlevel.cfg_go1(model)
        loops = dict(unfused=stack.StackLoop(model, p, H, batch, cfg, sc, W, low_level=ll_cfg),
                     fused=stack.StackLoop(model, p, H, batch, cfg, sc, W, low_level=ll_cfg, fused_low_level=True))
        start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
        bufs = [a.clone() for a in start]
        finals, log = {}, None
        for name, loop in loops.items():  # warm-up runs; the unfused one's log feeds the replays
            for d, s in zip(bufs, start):
                d.copy_(s)
            lg = loop.run_device(*bufs, T, log=True)
            torch.cuda.synchronize()
            finals[name] = [b.clone() for b in bufs] + [lg["states"], lg["out"], lg["ll_out"], lg["candidates"]]
            log = lg if name == "unfused" else log
        row = dict(batch=batch, H=H, mpc_ticks=T, wbc_per_mpc=W, dense_path=loops["fused"].solver.dense_path,
                   bytewise_equal=all(torch.equal(a, b) for a, b in zip(finals["unfused"], finals["fused"])),
                   fallen=fallen_count(log["states"].view(torch.float64)))
        finals.clear()

        def whole(loop):
            def run():
                for d, s in zip(bufs, start):
                    d.copy_(s)
                loop.run_device(*bufs, T)
            return run

        runs = dict(unfused=[], fused=[])
        for _ in range(args.repeats):  # alternating: a drift of the box hits both loops alike
            for name, loop in loops.items():
                runs[name].append(timed(whole(loop), 1) / T)
        for name in loops:
            best = min(runs[name])
            row[name] = dict(ms_per_mpc_tick=best, robot_ticks_per_s=batch / (best * 1e-3), runs_ms_per_mpc_tick=runs[name])
        row["unfused_spread_ms"] = max(runs["unfused"]) - min(runs["unfused"])
        row["gain_ms_per_mpc_tick"] = row["unfused"]["ms_per_mpc_tick"] - row["fused"]["ms_per_mpc_tick"]
        row["fused_is_faster_beyond_spread"] = row["gain_ms_per_mpc_tick"] > row["unfused_spread_ms"]
        # the low-level ticks of every MPC tick alone, from the state the unfused loop had before them
        before = [start[1]] + [log["states"][t * W - 1] for t in range(1, T)]
        before_out = [start[2]] + [log["out"][t * W - 1] for t in range(1, T)]
        gait = log["robots"].view(torch.int32)[:, :, est.GAIT_OFFSET]  # [T][B], the robots' stride
        d_st, d_o = torch.empty_like(start[1]), torch.empty_like(start[2])
        d_ll = torch.empty((batch, lowlevel.OUT_BYTES), dtype=torch.uint8, device=dev)
        d_cand = torch.empty((batch, 4), dtype=torch.int32, device=dev)
        tau = lowlevel.tau_view(d_ll)

        def fused():
            for t in range(T):
                d_st.copy_(before[t]), d_o.copy_(before_out[t])
                lowsim.run_device(model, sc, ll_cfg, d_st, log["target"][t], d_o, d_cand, d_ll, W, 1, gait[t])

        def unfused():
            for t in range(T):
                d_st.copy_(before[t]), d_o.copy_(before_out[t])
                for _ in range(W):
                    lowlevel.lowlevel_device(ll_cfg, d_st, log["target"][t], d_ll, gait[t], d_o, d_cand)
                    sim.step_device(model, sc, d_st, tau, d_cand, d_st, d_o, 1)

        def copies():
            for t in range(T):
                d_st.copy_(before[t]), d_o.copy_(before_out[t])

        parts = {}
        for name, fn in (("copies", copies), ("fused", fused), ("unfused", unfused)):
            fn()
            torch.cuda.synchronize()
            parts[name] = 1e3 * timed(fn, args.repeats) / T
        row.update(fused_launch_us_per_mpc_tick=parts["fused"] - parts["copies"],
                   unfused_launches_us_per_mpc_tick=parts["unfused"] - parts["copies"])
        rows.append(row)
        for loop in loops.values():
            loop.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wbc-warm", action="store_true")
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--low-level", action="store_true")
    ap.add_argument("--fused", action="store_true")
    args = ap.parse_args()
    if args.fused and not args.low_level:
        ap.error("--fused needs --low-level")
    import torch

    if args.low_level:
        line = json.dumps(dict(bench="stack_low_level_fused" if args.fused else "stack_low_level",
                               device=torch.cuda.get_device_name(0),
                               configs=fused_rows(args) if args.fused else low_level_rows(args)))
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    from legged_mpc_control_amd import BatchedConvexQPSolver, rbd, rollout, sim, stack, synth

    dev = torch.device("cuda:0")
    T = args.ticks
    rows = []
    for batch in [int(b) for b in args.batches.split(",")]:
        p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
        loop = stack.StackLoop(model, p, H, batch, cfg, sim.cfg(dt=SIM_DT, ground_z=0.0), WBC_PER_MPC,
                               wbc_warm=args.wbc_warm)
        start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
        bufs = [a.clone() for a in start]
        log = loop.run_device(*bufs, T, log=True)  # warm-up, and the record of what the run does
        torch.cuda.synchronize()
        x = log["states"].view(torch.float64)
        row = dict(batch=batch, H=H, mpc_ticks=T, wbc_per_mpc=WBC_PER_MPC, dense_path=loop.solver.dense_path,
                   nonzero_status=dict(qp=int((log["qp_status"] != 0).sum()), wbc=int((log["wbc_status"] != 0).sum()),
                                       sim=int((log["sim_status"] != 0).sum())),
                   fallen=int(((x[:, :, 1].abs() > 0.5) | (x[:, :, 2].abs() > 0.5) |
                               (x[:, :, 5] < 0.5 * x[0, :, 5])).any(dim=0).sum()))
        cmds = log["cmd"].contiguous()
        it = log["wbc_iters"].cpu().numpy()
        row["wbc_ipm_iters_per_level_mean"] = [float(v) for v in (it & 0xFFFF).mean(axis=(0, 1))]
        if args.wbc_warm:
            taken, tried = (it[1:] >> 19) & 1, (it[1:] >> 18) & 1
            rounds = ((it[1:] >> 20) & 15)[taken == 1]
            row["wbc_warm"] = dict(tried_share=float(tried.mean()), taken_share=float(taken.mean()),
                                   taken_share_per_level=[float(v) for v in taken.mean(axis=(0, 1))],
                                   repair_rounds_mean=float(rounds.mean()) if rounds.size else 0.0,
                                   repair_rounds_max=int(rounds.max()) if rounds.size else 0)

        def whole():
            for d, s in zip(bufs, start):
                d.copy_(s)
            loop.pipeline.reset_warm()
            loop.run_device(*bufs, T)

        ms = timed(whole, args.repeats)
        row["whole"] = dict(ms_per_mpc_tick=ms / T, robot_ticks_per_s=batch * T / (ms * 1e-3))
        if args.whole_only:
            rows.append(row)
            loop.close()
            continue
        grf = torch.empty((batch, H, 12), dtype=torch.float64, device=dev)
        solver = BatchedConvexQPSolver(p, H, max_batch=0)

        def solve_only():
            for t in range(T):
                solver.solve_commands_device(cmds[t], grf)

        solve_only()
        torch.cuda.synchronize()
        ms_solve = timed(solve_only, args.repeats)
        row["solve_only"] = dict(ms_per_tick=ms_solve / T)
        pipe = loop.pipeline  # the loop's own pipeline: the same buffers, nothing new allocated
        d_sim_cfg = loop.sim_cfg
        prev = [start[1]] + [log["states"][k] for k in range(WBC_PER_MPC * T - 1)]
        d_next, d_o = torch.empty_like(start[1]), torch.empty_like(start[2])

        def wbc_sim():
            for k in range(WBC_PER_MPC * T):
                d_x, _ = pipe.solve_device(prev[k], log["target"][k // WBC_PER_MPC])
                sim.step_device(model, d_sim_cfg, prev[k], d_x[:, sim.TAU_OFFSET:sim.TAU_OFFSET + 12],
                                log["candidates"][k], d_next, d_o, 1)

        wbc_sim()
        torch.cuda.synchronize()
        ms_ws = timed(wbc_sim, args.repeats)
        row["wbc_sim"] = dict(ms_per_tick=ms_ws / (WBC_PER_MPC * T))
        row["glue_us_per_mpc_tick"] = 1e3 * (ms - ms_solve - ms_ws) / T
        rows.append(row)
        solver.close()
        loop.close()
    line = json.dumps(dict(bench="stack", device=torch.cuda.get_device_name(0), configs=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
