#!/usr/bin/env python3
"""Benchmark of the hierarchical QP's warm start (lmpc_hoqp_solve_device_warm; DESIGN.md 4c "Warm start") on MI355X.

    python tools/bench_hoqp_warm.py [--steps K] [--warmup W] [--repeats R] [--out FILE]

4096 WBC chains resident in HBM, ms per launch, timed as tools/bench_hoqp.py times its launches (warm-up launches and
at least 30 ms of device time, then one HIP event pair around K launches); the best and the spread of R repeats of:

    cold        lmpc_hoqp_solve_device on tools/bench_hoqp.py's 1024 distinct synthetic chains, tiled
    warm_same   the warm entry point on the same records, the blocks left by the solve before
    trot_cold / trot_warm
                the low-level ticks k and k + 1 of a logged trot: 512 Go1 robots with seeded commands run 12 MPC ticks
                in `StackLoop`; the records of 8 consecutive low-level ticks of the 11th MPC tick and of the tick after
                each (4096 pairs) are rebuilt from the logged states and targets.  trot_cold = the cold entry point on
                the later ticks' records; trot_warm = the warm one on them from the blocks the earlier ticks' solves
                left, restored by a device copy before every launch (the copy is timed alone and subtracted).

Also: share of levels tried / taken warm, repair rounds, interior-point iterations, and the largest differences of
warm against cold results (final x relative, slacks absolute).  Prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

B = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warm-rounds", type=int, default=None, help="lmpc_hoqp_options.warm_rounds (A/B)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench_hoqp
    import bench_stack
    from legged_mpc_control_amd import hoqp as HQ
    from legged_mpc_control_amd import rbd, rollout, sim, stack, synth
    from legged_mpc_control_amd import wbc as W

    dev = torch.device("cuda:0")
    torch.cuda.init()
    chains = [W.synth_wbc_tasks(bench_hoqp.SEED0 + i) for i in range(1024)]
    dims = HQ.dims_of(chains[0])
    base = np.stack([HQ.pack(c, dims) for c in chains])
    d_synth = torch.from_numpy(np.ascontiguousarray(np.resize(base, (B, base.shape[1])))).to(dev)
    solver = HQ.HoqpBatch(dims, B)
    if args.warm_rounds is not None:
        solver.set_options(warm_rounds=args.warm_rounds)
    L, n = dims.num_levels, dims.num_vars

    def outs():
        return (torch.empty((B, L, n), dtype=torch.float64, device=dev),
                torch.empty((B, max(solver.slack_len, 1)), dtype=torch.float64, device=dev),
                torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, L), dtype=torch.int32, device=dev))

    o_cold, o_warm = outs(), outs()
    d_act = torch.zeros((B, solver.act_len), dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)

    def timed(fn):
        """bench_hoqp.py's method -> ms per call, R times"""
        run, tw = 0, time.perf_counter()
        while run < args.warmup or time.perf_counter() - tw < 0.03:
            fn()
            run += 1
            torch.cuda.synchronize(dev)
        res = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            res.append(e0.elapsed_time(e1) / args.steps)
        return res

    def stats(o):
        it = o[3].cpu().numpy()
        taken, tried = (it >> 19) & 1, (it >> 18) & 1
        rounds = ((it >> 20) & 15)[taken == 1]
        st = o[2].cpu().numpy()
        return dict(status=[int((st == v).sum()) for v in (0, 1, 2)],
                    ipm_iters_per_level_mean=[float(v) for v in (it & 0xFFFF).mean(axis=0)],
                    tried_share=float(tried.mean()), taken_share=float(taken.mean()),
                    taken_share_per_level=[float(v) for v in taken.mean(axis=0)],
                    repair_rounds_mean=float(rounds.mean()) if rounds.size else 0.0,
                    repair_rounds_max=int(rounds.max()) if rounds.size else 0)

    def diff(a, b):
        xa, xb = a[0][:, -1].cpu().numpy(), b[0][:, -1].cpu().numpy()
        wa, wb = a[1].cpu().numpy()[:, :solver.slack_len], b[1].cpu().numpy()[:, :solver.slack_len]
        return dict(final_x_rel=float(np.max(np.abs(xa - xb) / (1.0 + np.max(np.abs(xb), axis=1, keepdims=True)))),
                    slack_abs=float(np.max(np.abs(wa - wb))))

    def ms(v):
        return dict(ms_per_launch_best=min(v), ms_per_launch_all=v)

    res = {}
    # ---- synthetic chains: cold, and warm on identical records ---------------------------------------------------
    res["cold"] = ms(timed(lambda: solver.solve_device(d_synth, *o_cold, stream)))
    res["cold"].update(stats(o_cold))
    d_act.zero_()
    solver.solve_device(d_synth, *o_warm, stream, d_act=d_act)  # seeds the blocks (a cold solve)
    res["warm_same"] = ms(timed(lambda: solver.solve_device(d_synth, *o_warm, stream, d_act=d_act)))
    res["warm_same"].update(stats(o_warm))
    res["warm_same"]["vs_cold"] = diff(o_warm, o_cold)

    # ---- consecutive low-level ticks of a logged trot -------------------------------------------------------------
    R, T, Wm = 512, 12, bench_stack.WBC_PER_MPC
    p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
    loop = stack.StackLoop(model, p, bench_stack.H, R, cfg, sim.cfg(dt=bench_stack.SIM_DT, ground_z=0.0), Wm)
    bufs = [torch.from_numpy(a).to(dev) for a in bench_stack.start_of(R, 4000 + R)]
    log = loop.run_device(*bufs, T, log=True, stream=stream)
    torch.cuda.synchronize(dev)
    bad = [int((log[k] != 0).sum()) for k in ("qp_status", "wbc_status", "sim_status")]
    pipe = loop.pipeline
    d_a = torch.empty((B, W.WBC_RECORD_LEN), dtype=torch.float64, device=dev)
    d_b = torch.empty_like(d_a)
    k0 = 10 * Wm
    for j in range(8):  # tick k reads the state the tick before left, and its MPC tick's targets
        for d_dst, k in ((d_a, k0 + j), (d_b, k0 + j + 1)):
            rbd.wbc_inputs_device(model, log["states"][k - 1], log["target"][k // Wm], pipe.d_inputs[:R], stream)
            W.records_device(pipe.d_inputs[:R], d_dst[j * R:(j + 1) * R], stream)
    torch.cuda.synchronize(dev)
    res["trot_cold"] = ms(timed(lambda: solver.solve_device(d_b, *o_cold, stream)))
    res["trot_cold"].update(stats(o_cold))
    d_act.zero_()
    solver.solve_device(d_a, *o_warm, stream, d_act=d_act)
    d_act_a = d_act.clone()

    def warm_next():
        d_act.copy_(d_act_a)
        solver.solve_device(d_b, *o_warm, stream, d_act=d_act)

    both = timed(warm_next)
    copy = timed(lambda: d_act.copy_(d_act_a))
    res["trot_warm"] = dict(ms_per_launch_best=min(both) - min(copy), ms_with_block_copy_all=both, ms_block_copy_all=copy)
    warm_next()
    torch.cuda.synchronize(dev)
    res["trot_warm"].update(stats(o_warm))
    res["trot_warm"]["vs_cold"] = diff(o_warm, o_cold)
    res["trot_source"] = dict(robots=R, mpc_ticks=T, nonzero_status_qp_wbc_sim=bad,
                              ticks=f"low-level ticks {k0}..{k0 + 7} (A) and {k0 + 1}..{k0 + 8} (B)")
    loop.close()
    solver.close()
    line = json.dumps(dict(bench="hoqp_warm", device=torch.cuda.get_device_name(0), batch=B, steps=args.steps,
                           repeats=args.repeats, warm_rounds=args.warm_rounds, results=res))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
