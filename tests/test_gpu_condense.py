"""The dense path's condensation on the GPU at the shapes where its indexing can go wrong (csrc/lmpc_dense_common.h:
the step-lane scans, the leg-step -> tile / slot counters of the H-column pass, the store sinks), on both dense
paths, against the CPU oracle.

16 QPs per case: states from `synth`, contact arrays built by hand.  Every QP must come back converged and within
the project's regression guard (TOL_REGRESS = 1e-7, tests/test_gpu_parity.py) of oracle.solve_batch, and the oracle
must certify every instance (no QP is skipped): the seeds below were picked on the CPU for that.

The cases run with the Go1 preset and, so that the closed-form condensation sees a non-uniform R and a full inertia at
every shape it distinguishes, with two sets of tests/param_sets.py.
"""
import functools

import numpy as np
import pytest

import param_sets as PS
from conftest import rel_err

from legged_mpc_control_amd import BatchedConvexQPSolver, synth
from oracle import oracle as O

TOL_REGRESS = 1e-7
NQP = 16


def _contact(H, steps):
    """steps: {step: legs}"""
    c = np.zeros((H, 4), dtype=np.uint8)
    for k, legs in steps.items():
        c[k, list(legs)] = 1
    return c


def _trot(H):
    return {k: (0, 3) if (k // 2) % 2 == 0 else (1, 2) for k in range(H)}


# name -> (H, contact [H, 4], tilted terrain, seed)
CASES = {
    "h1": (1, _contact(1, {0: (0, 1, 2, 3)}), False, 11),
    "h2": (2, _contact(2, {0: (0, 3), 1: (1, 2)}), False, 12),
    # the dense path's longest horizon: one stance leg per step, four in the last -- 19 leg-steps
    "h16": (16, _contact(16, {**{k: (k % 4,) for k in range(15)}, 15: (0, 1, 2, 3)}), False, 13),
    # 20 leg-steps: every step's four legs straddle a 5 | 6 tile boundary
    "h5_all": (5, _contact(5, {k: (0, 1, 2, 3) for k in range(5)}), False, 14),
    "h10_trot": (10, _contact(10, _trot(10)), False, 15),
    "h10_ends": (10, _contact(10, {0: (0, 1, 2, 3), 9: (0, 1, 2, 3)}), False, 16),
    "h10_last1": (10, _contact(10, {9: (2,)}), False, 17),
    "h10_trot_tilted": (10, _contact(10, _trot(10)), True, 18),
    "h5_all_tilted": (5, _contact(5, {k: (0, 1, 2, 3) for k in range(5)}), True, 19),
}


@functools.lru_cache(maxsize=None)
def case(name, pset="go1"):
    """-> (params, H, rec, contact, normals, oracle forces) under the parameter set `pset` (tests/param_sets.py; "go1"
    is the preset); the oracle certifies all NQP instances"""
    H, con1, tilted, seed = CASES[name]
    p = PS.params(pset)
    rec, _ = synth.fill(p, synth.synth_cfg("go1"), H, NQP, seed)
    con = np.ascontiguousarray(np.broadcast_to(con1, (NQP, H, 4)))
    nrm = synth.normals(NQP, seed) if tilted else None
    ref, _, fails = O.solve_batch(O.params_from(p), H, rec, con, n_threads=8, normals=nrm)
    assert fails == 0, f"{name} {pset}: the oracle did not certify {fails} of {NQP} instances"
    ref.setflags(write=False)
    return p, H, rec, con, nrm, ref


def test_cases_cover_the_shapes():
    nls = {n: int(c[1].sum()) for n, c in CASES.items()}
    assert nls["h16"] == 19 and nls["h5_all"] == 20 and nls["h10_last1"] == 1 and nls["h10_ends"] == 8
    assert max(nls.values()) <= 20  # every case is the dense path's


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ipm", "gi"])
@pytest.mark.parametrize("name", list(CASES))
def test_condensed_paths_vs_oracle(name, mode):
    p, H, rec, con, nrm, ref = case(name)
    s = BatchedConvexQPSolver(p, H, max_batch=NQP, dense_path=mode)
    grf, status, iters = s.solve(rec, con, normals=nrm)
    err = rel_err(grf, ref)
    print(f"{name} {mode}: max rel err {err:.3e}, status {np.bincount(status)}")
    assert np.all(status == 0), status
    assert err <= TOL_REGRESS, f"{name} {mode}: {err:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ipm", "gi"])
@pytest.mark.parametrize("pset", ["aniso_r", "everything"])
@pytest.mark.parametrize("name", list(CASES))
def test_condensed_paths_general_params(name, pset, mode):
    """Every shape again off the presets: per-leg, per-component r (the input Hessian block R' diag(r) R has
    off-diagonal entries on tilted terrain) and, under `everything`, a full trunk inertia and weights on yaw, x, y."""
    p, H, rec, con, nrm, ref = case(name, pset)
    s = BatchedConvexQPSolver(p, H, max_batch=NQP, dense_path=mode)
    grf, status, iters = s.solve(rec, con, normals=nrm)
    err = rel_err(grf, ref)
    print(f"{name} {pset} {mode}: max rel err {err:.3e}, status {np.bincount(status)}")
    assert np.all(status == 0), status
    assert err <= TOL_REGRESS, f"{name} {pset} {mode}: {err:.3e}"
