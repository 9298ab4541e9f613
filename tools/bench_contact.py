#!/usr/bin/env python3
"""Benchmark of the frictional contact model on MI355X (include/lmpc/lmpc_contact.h), beside the present plant.

    python tools/bench_contact.py [--batch B] [--steps K] [--warmup W] [--rounds R] [--ticks T]
                                  [--out profiles/contact/bench_contact.json]

tools/bench_sim.py's method and batch: B Go1 robots resident in HBM (standing and trotting states around the nominal
pose), the torques of one WBC solve on them.  Timed in R alternating rounds, each stage with one HIP event pair around K
launches after W warm-up launches; the median over the rounds is reported:

    lmpc_sim_step_device, 1 and 9 substeps          the present plant, the targets' contact flags as candidates
    lmpc_contact_step_device, 1 and 9 substeps      the contact model with the same flags as its mask ("stance"), and
                                                    with every foot in the mask as the loop runs it ("all")
    the same four in the three-launch form          terms and K into a workspace, the bare solve, the back-substitution
    lmpc_contact_solve_device                       the bare problem alone (K = 2 I + 0.05, every foot pressed straight
                                                    down: the sticking trial verifies, one polish round, no sweep)

then the StackLoop's MPC tick (tools/bench_stack.py's start, 10 ms / 1.25 ms, T ticks, best of R repeats) with each
plant (the contact model fused and in three launches) at 1024 and 4096 robots: the contact model drops the eight
candidate launches of an MPC tick; and the estimator's velocity error over 1024 trotting robots on the present plant
(geometric touch) and on the contact model with the force-threshold touch flag.  Nothing here has a threshold.  Prints ONE JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

LOOP_BATCHES = (1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=512, help="distinct robots, tiled to the batch")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--est-ticks", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact", "bench_contact.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_contact.py needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    from bench_rbd import make_batch
    from bench_stack import H, SIM_DT, WBC_PER_MPC, start_of, timed as best_of
    from legged_mpc_control_amd import contact, rbd, rollout, sim, stack, synth

    B = args.batch
    model = rbd.model_go1()
    nd = min(args.distinct, B)
    states, targets = make_batch(rbd, model, nd)
    d_state = torch.from_numpy(np.resize(rbd.pack(states), (B, rbd.STATE_BYTES))).to(dev)
    d_target = torch.from_numpy(np.resize(rbd.pack(targets), (B, rbd.TARGET_BYTES))).to(dev)
    cf = sim.cfg(dt=0.002, ground_z=0.0)
    cc = contact.cfg(dt=0.002, ground_z=0.0)
    ws = sim.WbcSim(model, B, cf)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    d_x, d_status = ws.pipeline.solve_device(d_state, d_target, stream)
    d_tau = d_x[:, sim.TAU_OFFSET:sim.TAU_OFFSET + 12]
    d_flags = sim.target_contacts(d_target)
    d_ones = torch.ones((B, 4), dtype=torch.int32, device=dev)
    d_next = torch.empty_like(d_state)
    d_out = ws.d_out
    d_cout = torch.empty((B, contact.OUT_BYTES), dtype=torch.uint8, device=dev)
    d_K = (torch.eye(12, dtype=torch.float64, device=dev) * 2.0 + 0.05).reshape(1, 144).repeat(B, 1).contiguous()
    d_c = torch.zeros((B, 12), dtype=torch.float64, device=dev)
    d_c[:, 2::3] = -1.0  # every foot pressed straight down: the sticking trial verifies, no sweep
    d_P = torch.empty((B, 12), dtype=torch.float64, device=dev)
    d_work = torch.empty(contact.work_bytes(B), dtype=torch.uint8, device=dev)

    def cstep(mask, n, work=None):
        return lambda: contact.step_device(model, cc, d_state, d_tau, mask, d_next, d_out, d_cout, n, stream, work)

    stages = {
        "sim_step_1": lambda: sim.step_device(model, cf, d_state, d_tau, d_flags, d_next, d_out, 1, stream),
        "sim_step_9": lambda: sim.step_device(model, cf, d_state, d_tau, d_flags, d_next, d_out, 9, stream),
        "contact_stance_1": cstep(d_flags, 1), "contact_stance_9": cstep(d_flags, 9),
        "contact_all_1": cstep(d_ones, 1), "contact_all_9": cstep(d_ones, 9),
        "contact_split_stance_1": cstep(d_flags, 1, d_work), "contact_split_stance_9": cstep(d_flags, 9, d_work),
        "contact_split_all_1": cstep(d_ones, 1, d_work), "contact_split_all_9": cstep(d_ones, 9, d_work),
        "contact_solve": lambda: contact.solve_device(cc, d_K, d_c, d_ones, d_P, d_cout, stream),
    }

    def timed(launch, count):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(count):
            launch()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        return ev0.elapsed_time(ev1) * 1e3 / count  # us

    for launch in stages.values():
        for _ in range(args.warmup):
            launch()
    torch.cuda.synchronize(dev)
    rounds = {k: [] for k in stages}
    for _ in range(args.rounds):  # alternating: every stage once per round
        for name, launch in stages.items():
            rounds[name].append(timed(launch, args.steps))
    us = {k: statistics.median(v) for k, v in rounds.items()}
    stages["contact_all_1"]()
    torch.cuda.synchronize(dev)
    ci = d_cout.view(torch.int32)
    used = dict(sweeps=np.bincount(ci[:, 40].cpu().numpy()).tolist(), polish=np.bincount(ci[:, 41].cpu().numpy()).tolist(),
                status=np.bincount(ci[:, 42].cpu().numpy(), minlength=3).tolist(),
                modes=np.bincount(ci[:, 36:40].cpu().numpy().ravel(), minlength=11).tolist())
    ws.close()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))

    # the StackLoop's MPC tick with each plant, alternating
    loops = []
    for batch in LOOP_BATCHES:
        p, rcfg = synth.params(), rollout.cfg_go1()
        start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
        row = dict(batch=batch, H=H, mpc_ticks=args.ticks, wbc_per_mpc=WBC_PER_MPC)
        runs = {}
        for name, plant, split in (("sim", None, False), ("contact", contact.cfg(dt=SIM_DT, ground_z=0.0), False),
                                   ("contact_split", contact.cfg(dt=SIM_DT, ground_z=0.0), True)):
            loop = stack.StackLoop(model, p, H, batch, rcfg, sim.cfg(dt=SIM_DT, ground_z=0.0), WBC_PER_MPC, plant=plant,
                                   plant_split=split)
            bufs = [a.clone() for a in start]
            log = loop.run_device(*bufs, args.ticks, log=True)  # warm-up, and the record of what the run does
            torch.cuda.synchronize()
            x = log["states"].view(torch.float64)
            row[name + "_status"] = dict(qp=int((log["qp_status"] != 0).sum()), wbc=int((log["wbc_status"] != 0).sum()),
                                         sim=int((log["sim_status"] != 0).sum()),
                                         fallen=int(((x[:, :, 1].abs() > 0.5) | (x[:, :, 2].abs() > 0.5) |
                                                     (x[:, :, 5] < 0.5 * x[0, :, 5])).any(dim=0).sum()))

            def whole(loop=loop, bufs=bufs):
                for d, s in zip(bufs, start):
                    d.copy_(s)
                loop.run_device(*bufs, args.ticks)

            runs[name] = (loop, whole)
        ms = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, (_, whole) in runs.items():
                ms[name].append(best_of(whole, 1) / args.ticks)
        for name, (loop, _) in runs.items():
            row[name + "_ms_per_mpc_tick"] = statistics.median(ms[name])
            loop.close()
        row["contact_over_sim"] = row["contact_ms_per_mpc_tick"] / row["sim_ms_per_mpc_tick"]
        row["contact_split_over_sim"] = row["contact_split_ms_per_mpc_tick"] / row["sim_ms_per_mpc_tick"]
        loops.append(row)

    # the estimator's velocity error over 1024 trotting robots (exact sensors), 50 MPC ticks: the present plant with its
    # geometric touch flag beside the contact model with the force-threshold flag
    from legged_mpc_control_amd import est

    est_rows = {}
    batch, T = 1024, args.est_ticks
    p, rcfg = synth.params(), rollout.cfg_go1()
    start = [torch.from_numpy(a).to(dev) for a in start_of(batch, 4000 + batch)]
    for name, plant in (("sim_geometric_touch", None),
                        ("contact_force_touch", contact.cfg(dt=SIM_DT, ground_z=0.0, touch_rule=1, force_threshold=10.0))):
        loop = stack.StackLoop(model, p, H, batch, rcfg, sim.cfg(dt=SIM_DT, ground_z=0.0), WBC_PER_MPC,
                               estimator=est.cfg(dt=SIM_DT), plant=plant)
        log = loop.run_device(*[a.clone() for a in start], T, log=True)
        torch.cuda.synchronize()
        x = log["states"].view(torch.float64)
        ev = (log["state_est"].view(torch.float64)[:, :, 21:24] - x[:, :, 21:24]).norm(dim=2).cpu().numpy()
        est_rows[name] = dict(
            median=float(np.median(ev)), p90=float(np.percentile(ev, 90)), p99=float(np.percentile(ev, 99)),
            max=float(ev.max()), robots_above_1_m_s=int((ev.max(axis=0) > 1.0).sum()),
            nonzero_status=dict(qp=int((log["qp_status"] != 0).sum()), wbc=int((log["wbc_status"] != 0).sum()),
                                sim=int((log["sim_status"] != 0).sum()), est=int((log["est_status"] != 0).sum())),
            fallen=int(((x[:, :, 1].abs() > 0.5) | (x[:, :, 2].abs() > 0.5) |
                        (x[:, :, 5] < 0.5 * x[0, :, 5])).any(dim=0).sum()))
        loop.close()
        del log

    line = {
        "metric": "contact model beside the present plant, us per launch (median of alternating rounds)",
        "batch": B, "distinct": nd, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "robot": "go1",
        "dtype": "f64", "us": us, "us_rounds": rounds,
        "sim_us_per_substep": (us["sim_step_9"] - us["sim_step_1"]) / 8.0,
        "contact_stance_us_per_substep": (us["contact_stance_9"] - us["contact_stance_1"]) / 8.0,
        "contact_all_us_per_substep": (us["contact_all_9"] - us["contact_all_1"]) / 8.0,
        "contact_stance_over_sim_1": us["contact_stance_1"] / us["sim_step_1"],
        "contact_stance_over_sim_9": us["contact_stance_9"] / us["sim_step_9"],
        "contact_all_over_sim_1": us["contact_all_1"] / us["sim_step_1"],
        "contact_all_over_sim_9": us["contact_all_9"] / us["sim_step_9"],
        "contact_all_used": used, "wbc_not_converged": int((d_status != 0).sum().item()),
        "contact_split_all_over_fused_1": us["contact_split_all_1"] / us["contact_all_1"],
        "contact_split_all_over_fused_9": us["contact_split_all_9"] / us["contact_all_9"],
        "contact_split_stance_over_fused_1": us["contact_split_stance_1"] / us["contact_stance_1"],
        "contact_split_stance_over_fused_9": us["contact_split_stance_9"] / us["contact_stance_9"],
        "stack_loop": loops,
        "estimator_velocity_error_m_s": dict(batch=batch, mpc_ticks=T, wbc_per_mpc=WBC_PER_MPC, **est_rows),
    }
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
