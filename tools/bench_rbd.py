#!/usr/bin/env python3
"""Benchmark of the state -> torques pipeline of the whole-body controller on MI355X (include/lmpc/lmpc_rbd.h).

    python tools/bench_rbd.py [--batch B] [--steps K] [--warmup W] [--out profiles/rbd/bench_rbd.json]

B Go1 robots resident in HBM (standing and trotting states around the nominal pose, the weight split over the
stance feet, foot targets 2 cm / 0.3 m/s away).  Timed separately, each with one HIP event pair around K launches
after W warm-up launches and at least 30 ms of device time (as tools/bench_hoqp.py):

    lmpc_wbc_inputs_device      state + targets -> lmpc_wbc_input blocks (the rigid-body dynamics kernel)
    lmpc_wbc_tasks_device       blocks -> hierarchical-QP records
    lmpc_hoqp_solve_device      the hierarchical solve
    hipMemcpyAsync              device-to-device copy of B x 4848 B: the floor of any kernel that writes those bytes
    WbcPipeline.solve_device    the three launches back to back

Prints ONE JSON line and writes it to --out: the times, the inputs kernel as a multiple of the copy and as a share of
the pipeline, and the solve's status counts.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GAITS = ((1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1))


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's), for hipMemcpyAsync."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            return ctypes.CDLL(path)
    return ctypes.CDLL("libamdhip64.so")


def make_batch(rbd, model, count, seed=20261019):
    """Distinct states and targets: the host computes each robot's measured feet so the targets sit next to them."""
    rng = np.random.default_rng(seed)
    weight = sum(model.mass) * model.gravity
    stand = np.tile([0.0, 0.8, -1.6], 4)
    states, targets = [], []
    for i in range(count):
        contact = GAITS[i % len(GAITS)]
        moving = sum(contact) < 4
        euler = rng.uniform(-0.1, 0.1, 3) + [rng.uniform(-3.0, 3.0), 0.0, 0.0]
        s = np.concatenate([euler, [rng.uniform(-5, 5), rng.uniform(-5, 5), 0.3], stand + rng.uniform(-0.15, 0.15, 12),
                            rng.normal(0.0, 0.3 if moving else 0.05, 3), rng.normal(0.0, 0.1, 3) + [0.5 * moving, 0, 0],
                            rng.normal(0.0, 1.0 if moving else 0.1, 12)])
        st = rbd.state_from_vector(s)
        t = rbd.terms_dict(rbd.compute(model, st))
        forces = np.zeros(12)
        forces[2::3] = np.array(contact) * weight / sum(contact)
        states.append(st)
        targets.append(rbd.target(forces, t["foot_pos"] + rng.normal(0.0, 0.0115, 12),
                                  t["foot_vel"] + rng.normal(0.0, 0.17, 12), contact))
    return states, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=512, help="distinct robots, tiled to the batch")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbd", "bench_rbd.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_rbd.py needs a GPU"
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    from legged_mpc_control_amd import rbd
    from legged_mpc_control_amd import wbc as W

    B = args.batch
    model = rbd.model_go1()
    nd = min(args.distinct, B)
    states, targets = make_batch(rbd, model, nd)
    d_state = torch.from_numpy(np.resize(rbd.pack(states), (B, rbd.STATE_BYTES))).to(dev)
    d_target = torch.from_numpy(np.resize(rbd.pack(targets), (B, rbd.TARGET_BYTES))).to(dev)
    pipe = rbd.WbcPipeline(model, B, 0)
    d_copy = torch.empty_like(pipe.d_inputs)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    nbytes = B * rbd.INPUT_BYTES

    def copy():
        rc = hip.hipMemcpyAsync(d_copy.data_ptr(), pipe.d_inputs.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3 = DtoD
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed ({rc})")

    stages = {
        "wbc_inputs": lambda: rbd.wbc_inputs_device(model, d_state, d_target, pipe.d_inputs, stream),
        "wbc_tasks": lambda: W.records_device(pipe.d_inputs, pipe.d_records, stream),
        "hoqp_solve": lambda: pipe.solver.solve_device(pipe.d_records, pipe.d_levels, pipe.d_slack, pipe.d_status,
                                                       pipe.d_iters, stream),
        "copy_d2d": copy,
        "pipeline": lambda: pipe.solve_device(d_state, d_target, stream),
    }
    ms = {}
    for name, launch in stages.items():  # in pipeline order: each stage's input is the previous one's output
        warm, tw = 0, time.perf_counter()
        while warm < args.warmup or time.perf_counter() - tw < 0.03:
            launch()
            warm += 1
            torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.steps):
            launch()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        ms[name] = ev0.elapsed_time(ev1) / args.steps
    assert torch.equal(d_copy, pipe.d_inputs)
    status = pipe.d_status.cpu().numpy()
    total = ms["wbc_inputs"] + ms["wbc_tasks"] + ms["hoqp_solve"]
    line = {
        "metric": "state -> torques pipeline of the WBC, per stage (ms per launch)",
        "batch": B, "distinct": nd, "steps": args.steps, "warmup": args.warmup, "robot": "go1", "dtype": "f64",
        "ms": ms,
        "bytes_written_per_robot": rbd.INPUT_BYTES,
        "wbc_inputs_gbs_written": nbytes / (ms["wbc_inputs"] * 1e-3) / 1e9,
        "copy_d2d_gbs": nbytes / (ms["copy_d2d"] * 1e-3) / 1e9,
        "wbc_inputs_over_copy": ms["wbc_inputs"] / ms["copy_d2d"],
        "wbc_inputs_share_of_pipeline": ms["wbc_inputs"] / total,
        "stages_sum_ms": total,
        "robots_per_s_pipeline": B / (ms["pipeline"] * 1e-3),
        "status": {"converged": int((status == 0).sum()), "max_iter": int((status == 1).sum()),
                   "nan": int((status == 2).sum())},
    }
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
