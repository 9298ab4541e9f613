#!/usr/bin/env python3
"""Benchmark of the device-resident closed-loop rollout (include/lmpc/lmpc_rollout.h) on MI355X.

    python tools/bench_rollout.py [--ticks T] [--repeats R]

Go1 trot robots from standing at 0.30 m with seeded commands, two configurations: 1024 robots at H = 10 and 4096 at
H = 30.  Each runs cold (d_act = NULL: the context's normal routing) and warm (the active set carried on the device,
every QP on the scratch Riccati kernel).  One HIP event pair around the whole rollout of T ticks, after a warm-up
rollout from the same start; the best of R repeats.  The same T ticks' commands (logged by the warm-up rollout) then go
through lmpc_solve_commands_device alone, one call per tick on the context's normal routing: the difference is what
the advance launches and the rollout's host loop add to a tick.  Prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = ((1024, 10), (4096, 30))


def robots_for(batch, seed):
    from legged_mpc_control_amd import _native as N, rollout as R

    rng = np.random.default_rng(seed)
    x0 = np.zeros((batch, 12))
    x0[:, 2] = rng.uniform(-3.0, 3.0, batch)
    x0[:, 5] = 0.30
    vd = np.stack([rng.uniform(-0.6, 0.6, batch), rng.uniform(-0.3, 0.3, batch)], axis=1)
    return R.robots_init(R.cfg_go1(), x0, vd, rng.uniform(-0.5, 0.5, batch), 0.30, N.GAIT_TROT, 4.0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from legged_mpc_control_amd import BatchedConvexQPSolver, rollout as R, synth

    dev = torch.device("cuda:0")
    T = args.ticks
    rows = []
    for batch, H in CONFIGS:
        p = synth.params()
        s = BatchedConvexQPSolver(p, H, max_batch=0)
        s.reserve_warm(batch)
        start = R.to_device(robots_for(batch, 1000 + H), dev)
        row = dict(batch=batch, H=H, ticks=T, dense_path=s.dense_path, riccati_path=s.riccati_path)
        cmd_log = None
        for mode in ("cold", "warm"):
            d_rb = start.clone()
            act = torch.zeros((batch, H, 4), dtype=torch.uint8, device=dev) if mode == "warm" else None
            log = s.rollout_device(d_rb, T, act=act, log=True)  # warm-up, and the record of what the run does
            torch.cuda.synchronize()
            if mode == "cold":
                cmd_log = log.cmd
            st, it = log.status.cpu().numpy(), log.iters.cpu().numpy()

            def go():
                d_rb.copy_(start)
                if act is not None:
                    act.zero_()
                s.rollout_device(d_rb, T, act=act, log=False)

            ms = timed(go, args.repeats)
            row[mode] = dict(ms_per_tick=ms / T, robot_ticks_per_s=batch * T / (ms * 1e-3),
                             nonconverged=int((st != 0).sum()), ipm_iters_per_qp=float((it[1:] & 0xFFFF).mean()),
                             polish_rounds_per_qp=float((it[1:] >> 16).mean()))
        grf = torch.empty((batch, H, 12), dtype=torch.float64, device=dev)

        def solve_only():
            for t in range(T):
                s.solve_commands_device(cmd_log[t], grf)

        solve_only()
        torch.cuda.synchronize()
        ms = timed(solve_only, args.repeats)
        row["solve_only"] = dict(ms_per_tick=ms / T, robot_ticks_per_s=batch * T / (ms * 1e-3))
        row["tick_overhead_us"] = 1e3 * (row["cold"]["ms_per_tick"] - ms / T)
        row["warm_over_cold"] = row["warm"]["ms_per_tick"] / row["cold"]["ms_per_tick"]
        rows.append(row)
    print(json.dumps(dict(bench="rollout", device=torch.cuda.get_device_name(0), configs=rows)))


if __name__ == "__main__":
    main()
