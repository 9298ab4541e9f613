#!/usr/bin/env python3
"""Benchmark of the state estimator (include/lmpc/lmpc_est.h) on MI355X, alone and inside the full loop.

    python tools/bench_est.py [--ticks T] [--repeats R] [--launches L] [--out FILE]

1024 and 4096 Go1 trot robots from tools/bench_stack.py's seeded start, H = 10, the reference's rates (10 ms MPC tick,
8 low-level ticks of 1.25 ms), exact sensors.  In one process, per batch:

    sensors_us, update_us   L back-to-back launches of lmpc_est_sensors_from_plant_device / lmpc_est_update_device (the
                            update with the state estimate, lmpc_est_out and the shadow block) on the loop's buffers after
                            a warm-up run, one HIP event pair around all L, divided by L; the best of R repeats
    wbc_sim_us              the 8 T low-level ticks of the plain loop replayed as tools/bench_stack.py replays them
                            (WbcPipeline.solve_device, then lmpc_sim_step_device, on the logged data): the yardstick the
                            two estimator launches are held against (est_share = (sensors_us + update_us) / wbc_sim_us)
    loop_ms, loop_est_ms    one HIP event pair around a whole StackLoop.run_device of T MPC ticks without and with the
                            estimator, from the same start; the best of R repeats

Prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_stack import BATCHES, H, SIM_DT, WBC_PER_MPC, start_of, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from legged_mpc_control_amd import est, rbd, rollout, sim, stack, synth

    dev = torch.device("cuda:0")
    T, L = args.ticks, args.launches
    rows = []
    for batch in BATCHES:
        p, cfg, model = synth.params(), rollout.cfg_go1(), rbd.model_go1()
        ecfg = est.cfg(dt=SIM_DT)
        start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
        row = dict(batch=batch, H=H, mpc_ticks=T, wbc_per_mpc=WBC_PER_MPC)
        for key, estimator in (("loop", None), ("loop_est", ecfg)):
            loop = stack.StackLoop(model, p, H, batch, cfg, sim.cfg(dt=SIM_DT, ground_z=0.0), WBC_PER_MPC,
                                   estimator=estimator)
            bufs = [a.clone() for a in start]
            log = loop.run_device(*bufs, T, log=True)  # warm-up, and the record of what the run does
            torch.cuda.synchronize()
            x = log["states"].view(torch.float64)
            status = dict(qp=int((log["qp_status"] != 0).sum()), wbc=int((log["wbc_status"] != 0).sum()),
                          sim=int((log["sim_status"] != 0).sum()))
            if estimator is not None:
                status["est"] = int((log["est_status"] != 0).sum())
            fallen = int(((x[:, :, 1].abs() > 0.5) | (x[:, :, 2].abs() > 0.5) | (x[:, :, 5] < 0.5 * x[0, :, 5])).any(dim=0).sum())

            def whole():
                for d, s in zip(bufs, start):
                    d.copy_(s)
                if estimator is not None:
                    loop.reset_estimator()
                loop.run_device(*bufs, T)

            ms = timed(whole, args.repeats)
            row[key] = dict(ms_per_mpc_tick=ms / T, nonzero_status=status, fallen=fallen)
            if estimator is None:
                prev = [start[1]] + [log["states"][k] for k in range(WBC_PER_MPC * T - 1)]
                d_next, d_o = torch.empty_like(start[1]), torch.empty_like(start[2])

                def wbc_sim():
                    for k in range(WBC_PER_MPC * T):
                        d_x, _ = loop.pipeline.solve_device(prev[k], log["target"][k // WBC_PER_MPC])
                        sim.step_device(model, loop.sim_cfg, prev[k], d_x[:, sim.TAU_OFFSET:sim.TAU_OFFSET + 12],
                                        log["candidates"][k], d_next, d_o, 1)

                wbc_sim()
                torch.cuda.synchronize()
                row["wbc_sim_us"] = 1e3 * timed(wbc_sim, args.repeats) / (WBC_PER_MPC * T)
            else:
                d_st, d_so = bufs[1], bufs[2]
                d_gait = est.gait_view(bufs[0])
                d_f0 = loop.d_filter.clone()

                def sensors():
                    for i in range(L):
                        est.sensors_from_plant_device(model, ecfg, d_st, d_so, loop.d_sensors, i + 1, 0, d_gait)

                def update():
                    loop.d_filter.copy_(d_f0)
                    for i in range(L):
                        est.update_device(model, ecfg, loop.d_sensors, loop.d_filter, loop.d_state_est, loop.d_est_out,
                                          d_so, loop.d_shadow)

                sensors(), update()
                torch.cuda.synchronize()
                row["sensors_us"] = 1e3 * timed(sensors, args.repeats) / L
                row["update_us"] = 1e3 * timed(update, args.repeats) / L
                xe = log["state_est"].view(torch.float64)
                row["estimate"] = dict(vel_err_max=float((xe[:, :, 21:24] - x[:, :, 21:24]).abs().max()),
                                       height_err_max=float((xe[:, :, 5] - x[:, :, 5]).abs().max()))
            loop.close()
        row["est_share_of_wbc_sim"] = (row["sensors_us"] + row["update_us"]) / row["wbc_sim_us"]
        row["loop_est_over_loop"] = row["loop_est"]["ms_per_mpc_tick"] / row["loop"]["ms_per_mpc_tick"]
        rows.append(row)
    line = json.dumps(dict(bench="est", device=torch.cuda.get_device_name(0), configs=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
