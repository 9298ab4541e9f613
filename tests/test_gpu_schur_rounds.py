"""The dense polish's range-space rounds under the re-tuned cost rule (lmpc_dense_kernel.h: LMPC_SCHUR_SLOPE2 /
LMPC_SCHUR_LIM2, the sparse column product h_col3, K factorised at its own size, the rule's integer face counts).

The product against the test-only "noschur" build, which refactorises every polish round (build.py TEST_VARIANTS), with
the bounds of tests/test_gpu_kkt.py::test_range_space_rounds_match_refactorised_rounds: status 0 everywhere, the same
iteration word QP for QP, forces within 1e-9 of each other and both within 2e-10 of the exact oracle, and at least one
QP whose bits differ (so the updates ran).  Two small batches: the first 256 config-2 QPs, which hold four of the
launch's slowest QPs (33, 57, 201, 226: four polish rounds each, the multi-round chains the rule decides about), and
128 config-2 QPs on terrain (per-leg normals from config 4's generator: the TERRAIN instance of the kernel).

That the batches reach the code is shown by the test-only "schurdiag" build (LMPC_SCHUR_DIAG: per-QP counters of the
range-space rounds, read back like lmpc_refine_diag): each batch must hold a round with a column entry (h_col3 runs
only there), a round of two or more entries (the K factorisations above size 1) and a QP with two consecutive
range-space rounds; the build also compares leg_free's counts with the nonzero columns of the bases leg_basis builds,
on every changed leg-step of every range-space round.  Entries are not reused across rounds (not built), so there is
no reuse counter and no "schurfresh" comparison.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_kkt import _per_qp_err, _variant


def _solve(L, p, H, rec, con, normals):
    """lmpc_solve_batch_ex on the dense path (interior point + polish), flat ground or per-leg terrain normals."""
    B = rec.shape[0]
    dp, i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ctx = ctypes.c_void_p()
    assert L.lmpc_create(ctypes.byref(p), H, B, 0, ctypes.byref(ctx)) == 0
    try:
        assert L.lmpc_set_dense_path(ctx, 1) == 0
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        con = np.ascontiguousarray(con, dtype=np.uint8)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
        g = np.zeros((B, H, 12))
        st = np.zeros(B, dtype=np.int32)
        it = np.zeros(B, dtype=np.int32)
        rc = L.lmpc_solve_batch_ex(ctx, rec.ctypes.data_as(dp), con.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                   None if nrm is None else nrm.ctypes.data_as(dp), B, g.ctypes.data_as(dp),
                                   st.ctypes.data_as(i32), it.ctypes.data_as(i32))
        assert rc == 0
        return g, st, it
    finally:
        L.lmpc_destroy(ctx)


def _batch(name):
    from legged_mpc_control_amd import synth

    if name == "window":
        p, H, rec, con = synth.config_batch(2, count=256, first_index=0)
        return p, H, rec, con, None
    p, H, rec, con = synth.config_batch(2, count=128, first_index=0)
    return p, H, rec, con, synth.config_normals(4, count=128)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window", "terrain"])
def test_range_space_rounds_match_refactorised_rounds_on(name):
    from legged_mpc_control_amd import _native as N
    from oracle import oracle as O

    p, H, rec, con, nrm = _batch(name)
    ref, _, _ = O.solve_batch(O.params_from(p), H, rec, con, n_threads=8, normals=nrm)
    g0, st0, it0 = _solve(N.lib(), p, H, rec, con, nrm)
    g1, st1, it1 = _solve(_variant("noschur"), p, H, rec, con, nrm)
    e0, e1 = _per_qp_err(g0, ref), _per_qp_err(g1, ref)
    print(f"{name}: range-space updates max err {e0.max():.3g}; refactorised {e1.max():.3g}; max |difference| "
          f"{np.max(np.abs(g0 - g1)):.3g}; QPs whose bits differ {(g0 != g1).any(axis=(1, 2)).sum()}; iteration words "
          f"differ on {(it0 != it1).sum()}; polish rounds {np.bincount(it0 >> 16).tolist()}")
    assert (st0 == 0).all() and (st1 == 0).all()
    assert (it0 == it1).all(), f"iteration words differ on {(it0 != it1).sum()} QPs"
    assert e0.max() <= 2e-10 and e1.max() <= 2e-10
    assert np.max(np.abs(g0 - g1)) <= 1e-9
    assert (g0 != g1).any(axis=(1, 2)).sum() > 0, "no range-space round ran: the test proves nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window", "terrain"])
def test_batches_reach_columns_larger_rounds_and_chains(name):
    """Counters of the "schurdiag" build: [range-space rounds, entries built, column entries, largest nsch, longest
    run of consecutive range-space rounds, leg-steps where leg_free disagrees with the bases' nonzero columns]."""
    p, H, rec, con, nrm = _batch(name)
    L = _variant("schurdiag")
    dp = ctypes.POINTER(ctypes.c_double)
    L.lmpc_debug_schur.argtypes = [dp, ctypes.c_int]
    assert L.lmpc_debug_schur_clear() == 0
    g, st, it = _solve(L, p, H, rec, con, nrm)
    B = rec.shape[0]
    d = np.zeros((B, 6))
    assert L.lmpc_debug_schur(d.ctypes.data_as(dp), B) == B
    rounds, ent, col, nmax, run, mis = (d[:, i] for i in range(6))
    print(f"{name}: range-space rounds {rounds.sum():.0f} on {(rounds > 0).sum()} QPs, entries {ent.sum():.0f}, column "
          f"entries {col.sum():.0f} on {(col > 0).sum()} QPs, largest nsch {nmax.max():.0f} ({(nmax >= 2).sum()} QPs >= 2), "
          f"longest run {run.max():.0f} ({(run >= 2).sum()} QPs >= 2), leg_free mismatches {mis.sum():.0f}")
    assert (st == 0).all()
    assert (rounds <= (it >> 16)).all() and (ent >= rounds).all() and (nmax <= 6).all()
    assert col.sum() > 0, "no round with a column entry: h_col3 never ran, the test proves nothing"
    assert (nmax >= 2).sum() > 0, "no round with two or more entries: the test proves nothing"
    assert (run >= 2).sum() > 0, "no QP with two consecutive range-space rounds: the test proves nothing"
    assert mis.sum() == 0, "leg_free disagrees with the nonzero columns of leg_basis"
