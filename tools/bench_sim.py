#!/usr/bin/env python3
"""Benchmark of the rigid-body plant on MI355X (include/lmpc/lmpc_sim.h).

    python tools/bench_sim.py [--batch B] [--steps K] [--warmup W] [--rounds R] [--out profiles/sim/bench_sim.json]

B Go1 robots resident in HBM (tools/bench_rbd.py's batch: standing and trotting states around the nominal pose), the
torques of one WBC solve on them, the targets' contact flags as candidates.  Timed in R alternating rounds, each stage
with one HIP event pair around K launches after W warm-up launches; the median over the rounds is reported:

    lmpc_sim_step_device, 1 and 9 substeps     the plant kernel; (t9 - t1) / 8 is one substep with the state in registers
    lmpc_rbd_forward_dynamics_device           the acceleration-level solve alone
    lmpc_rbd_compute_device                    the dynamics terms alone, on the same batch (it writes 5072 B per robot)
    hipMemcpyAsync                             device-to-device copy of the bytes one step reads and writes (1160 B per robot)

and then one WbcSim tick (WBC pipeline + plant step, state updated in place).  Nothing here has a threshold: the times
are reported, with the plant's share of the tick.  Prints ONE JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

STEP_BYTES = 288 + 96 + 16 + 288 + 472  # state, tau, contact in; next state, lmpc_sim_out out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=512, help="distinct robots, tiled to the batch")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim", "bench_sim.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_sim.py needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    from bench_rbd import hip_runtime, make_batch
    from legged_mpc_control_amd import rbd, sim

    B = args.batch
    model = rbd.model_go1()
    nd = min(args.distinct, B)
    states, targets = make_batch(rbd, model, nd)
    state0 = torch.from_numpy(np.resize(rbd.pack(states), (B, rbd.STATE_BYTES))).to(dev)
    d_target = torch.from_numpy(np.resize(rbd.pack(targets), (B, rbd.TARGET_BYTES))).to(dev)
    cf = sim.cfg(dt=0.002, ground_z=0.0)
    ws = sim.WbcSim(model, B, cf)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    d_state = state0.clone()
    d_x, d_status = ws.pipeline.solve_device(d_state, d_target, stream)
    d_tau = d_x[:, sim.TAU_OFFSET:sim.TAU_OFFSET + 12]
    d_contact = sim.target_contacts(d_target)
    d_next = torch.empty_like(d_state)
    d_out = ws.d_out
    d_terms = torch.empty((B, rbd.TERMS_BYTES), dtype=torch.uint8, device=dev)
    d_src = torch.zeros(B * STEP_BYTES, dtype=torch.uint8, device=dev)
    d_dst = torch.empty_like(d_src)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int

    def copy():
        rc = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), B * STEP_BYTES, 3, stream.cuda_stream)  # 3 = DtoD
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

    stages = {
        "step_1": lambda: sim.step_device(model, cf, d_state, d_tau, d_contact, d_next, d_out, 1, stream),
        "step_9": lambda: sim.step_device(model, cf, d_state, d_tau, d_contact, d_next, d_out, 9, stream),
        "forward_dynamics": lambda: sim.forward_dynamics_device(model, d_state, d_tau, d_contact, d_out, True, stream),
        "rbd_compute": lambda: rbd.compute_device(model, d_state, d_terms, stream),
        "copy_d2d": copy,
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
    flags = d_out.view(torch.int32)[:, sim.OUT_BYTES // 4 - 10:].cpu().numpy()

    # one controller tick: WBC pipeline + plant step, the state updated in place
    tick, pipe_us = [], []
    for _ in range(args.rounds):
        d_state.copy_(state0)
        ws.run_device(d_state, d_target, args.warmup, stream=stream)
        torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        ws.run_device(d_state, d_target, args.ticks, stream=stream)
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        tick.append(ev0.elapsed_time(ev1) * 1e3 / args.ticks)
        pipe_us.append(timed(lambda: ws.pipeline.solve_device(d_state, d_target, stream), args.ticks))
    tick_us, pipeline_us = statistics.median(tick), statistics.median(pipe_us)
    substep = (us["step_9"] - us["step_1"]) / 8.0
    line = {
        "metric": "rigid-body plant, us per launch (median of alternating rounds)",
        "batch": B, "distinct": nd, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "robot": "go1",
        "dtype": "f64", "us": us, "us_rounds": rounds,
        "us_per_substep_in_registers": substep,
        "bytes_per_robot_step": STEP_BYTES,
        "step_over_copy": us["step_1"] / us["copy_d2d"],
        "step_over_rbd_compute": us["step_1"] / us["rbd_compute"],
        "robot_steps_per_s": B / (us["step_1"] * 1e-6),
        "tick_us": tick_us, "pipeline_us": pipeline_us, "ticks": args.ticks,
        "plant_share_of_tick": us["step_1"] / tick_us,
        "status": {"plant_failed": int((flags[:, 8] != 0).sum()), "wbc_not_converged": int((d_status != 0).sum().item()),
                   "feet_held": int(flags[:, 0:4].sum()), "candidates": int(d_contact.sum().item())},
    }
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    ws.close()


if __name__ == "__main__":
    main()
