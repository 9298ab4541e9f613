"""Generates tests/golden/rollout_trot_h10.npz: the closed loop of tests/rollout_ref.py (NumPy restatement + the
oracle's exact QP solve, CPU only) for the robots tests/test_gpu_rollout.py runs end to end.

    python tests/golden/make_rollout_golden.py

Stored: x [ticks, B, 12] (state after each tick's plant step), u0 [ticks, B, 12], and sens [B]: the largest state
difference between that run and a second one in which every u_0 is perturbed by a relative 1e-7 (uniform in +-1e-7
per component, fixed seed).  1e-7 is the suite's parity guard on the forces (tests/test_gpu_parity.py), so sens is
the state error a solver exactly at the guard would be allowed to build up over the run.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import rollout_ref as RR  # noqa: E402
from oracle import oracle as O  # noqa: E402

GO1_Q = [50.0, 100.0, 0.0, 0.0, 0.0, 3500.0, 0.01, 0.01, 10.0, 15.0, 15.0, 20.0]  # gazebo_go1_convex.yaml:39-71
EPS, SEED = 1e-7, 20261019


def main():
    op = O.make_params(GO1_Q, [1e-4] * 12)
    H, ticks = RR.GOLDEN_H, RR.GOLDEN_TICKS
    x, u0 = RR.run(op, H, RR.golden_robots(), ticks)
    xp, _ = RR.run(op, H, RR.golden_robots(), ticks, rng=np.random.default_rng(SEED), eps=EPS)
    sens = np.abs(xp - x).max(axis=(0, 2))
    out = os.path.join(HERE, "rollout_trot_h10.npz")
    np.savez_compressed(out, x=x, u0=u0, sens=sens, eps=EPS, H=H, ticks=ticks,
                        vel_d=np.array([r[0] for r in RR.GOLDEN_ROBOTS]), yaw_rate=np.array([r[1] for r in RR.GOLDEN_ROBOTS]))
    print(out, os.path.getsize(out), "bytes; sens =", sens)
    for b in range(x.shape[1]):
        xe = x[-1, b]
        c, s = np.cos(xe[2]), np.sin(xe[2])
        print(b, "z in", x[:, b, 5].min(), x[:, b, 5].max(), "max |roll|,|pitch|", np.abs(x[:, b, 0:2]).max(),
              "v_body", c * xe[9] + s * xe[10], -s * xe[9] + c * xe[10], "yaw rate", xe[8])


if __name__ == "__main__":
    main()
