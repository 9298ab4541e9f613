"""GPU tests (MI355X) of the convex-MPC QP kernels off the two robot presets: the parameter sets of
tests/param_sets.py (per-leg, per-component r; a full trunk inertia; weights on yaw, x and y; other mu, f_max, mass,
gravity, dt) on every kernel and instance, against the CPU oracle at the suite's regression guard.

tests/test_params_host.py pins the reference on the CPU first: the oracle's assembly and answers on these sets are
certified there, and each set moves the optimum by 1e4 x the bar or more on the batches below.
"""
import ctypes

import numpy as np
import pytest

import param_sets as PS
from conftest import rel_err
from test_gpu_parity import terrain_violation

from legged_mpc_control_amd import BatchedConvexQPSolver, _native as N

pytestmark = pytest.mark.gpu

TOL_REGRESS = 1e-7
TERRAIN = pytest.mark.parametrize("terrain", [False, True], ids=["flat", "terrain"])


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def solve_and_check(name, H, count, terrain, tag, cid=4, **ctx):
    """One host-path solve of PS.batch(name, H, count, cid) on a fresh context -> (forces, iters); every QP status 0
    and the batch within TOL_REGRESS of the oracle."""
    rec, con, nrm = PS.batch(name, H, count, cid)
    s = BatchedConvexQPSolver(PS.params(name), H, max_batch=count, **ctx)
    grf, status, iters = s.solve(rec, con, normals=nrm if terrain else None)
    err = rel_err(grf, PS.reference(name, H, count, terrain, cid))
    print(f"{name} {'terrain' if terrain else 'flat'} H={H} {tag}: max rel err {err:.3e}, status {np.bincount(status)}")
    assert np.all(status == 0), status
    assert err <= TOL_REGRESS, f"{name} {tag}: {err:.3e}"
    return grf, iters


@pytest.mark.parametrize("mode", ["ipm", "gi", "off"])
@TERRAIN
@pytest.mark.parametrize("name", PS.NAMES)
def test_mixed_batch_every_dense_path(name, terrain, mode):
    """64 mixed-gait QPs at H = 10: the trots (at most 20 stance leg-steps) run on the dense kernel of `mode`, the
    rest on the LDS Riccati kernel in the same call; with "off" all run on the Riccati kernel."""
    _, con, _ = PS.batch(name, 10, 64)
    nls = con.sum((1, 2))
    dense = (nls >= 1) & (nls <= 20)
    assert dense.any() and not dense.all()  # both groups are in the batch
    grf, _ = solve_and_check(name, 10, 64, terrain, f"dense={mode}", dense_path=mode)
    ref = PS.reference(name, 10, 64, terrain)
    err_d, err_r = rel_err(grf[dense], ref[dense]), rel_err(grf[~dense], ref[~dense])
    print(f"    {dense.sum()} dense-eligible QPs {err_d:.3e}, the other {(~dense).sum()} {err_r:.3e}")
    assert err_d <= TOL_REGRESS and err_r <= TOL_REGRESS


@TERRAIN
@pytest.mark.parametrize("name", ["aniso_r", "full_inertia", "everything"])
def test_scratch_riccati_kernel(name, terrain):
    solve_and_check(name, 10, 32, terrain, "scratch Riccati", dense_path="off", riccati_path="scratch")


@pytest.mark.parametrize("H,count", [(16, 32), (20, 24)], ids=["LS1", "LS2"])
@TERRAIN
@pytest.mark.parametrize("name", ["everything", "heavy_slow"])
def test_lds_kernel_instances(name, terrain, H, count):
    """The LDS Riccati kernel's one- and two-leg-step-per-lane instances (H <= 16, H > 16); no QP of these batches has
    20 stance leg-steps or fewer, so at H = 16 none is taken by the dense path either."""
    _, con, _ = PS.batch(name, H, count)
    assert con.sum((1, 2)).min() > 20
    solve_and_check(name, H, count, terrain, "LDS Riccati")


def test_two_wave_instance(torch_dev):
    """More QPs than 4 x CUs: the Riccati kernel runs two waves per SIMD.  The first 128 QPs against the oracle, all
    of them converged and feasible in every leg's contact frame."""
    import torch

    name, H = "everything", 10
    cus = torch.cuda.get_device_properties(torch_dev).multi_processor_count
    count = 4 * cus + 64
    rec, con, nrm = PS.batch(name, H, count)
    v = PS.vector(name)
    s = BatchedConvexQPSolver(PS.params(name), H, max_batch=count, dense_path="off")
    grf, status, _ = s.solve(rec, con, normals=nrm)
    assert np.all(status == 0), np.bincount(status)
    viol = terrain_violation(grf, con, nrm, v[34], v[35])
    assert viol <= 1e-9 * v[35], viol
    assert not np.any(grf.reshape(count, H, 4, 3)[~con.astype(bool)] != 0.0)
    ref = PS.solve_ref(v, H, rec[:128], con[:128], nrm[:128])
    err = rel_err(grf[:128], ref)
    print(f"two-wave instance, {count} QPs: max rel err of the first 128 {err:.3e}, violation {viol:.2e}")
    assert err <= TOL_REGRESS


@pytest.mark.parametrize("H", [10, 20])
def test_warm_start(H):
    """lmpc_solve_batch_warm cold, then warm from the verified set shifted one step, flat and with terrain: the
    oracle's optimum and status 0 each time."""
    name, count = "everything", 24
    rec, con, nrm = PS.batch(name, H, count)
    s = BatchedConvexQPSolver(PS.params(name), H, max_batch=count)
    for terrain in (False, True):
        n = nrm if terrain else None
        ref = PS.reference(name, H, count, terrain)
        g0, st0, it0, a0 = s.solve_warm(rec, con, normals=n)
        assert np.all(st0 == 0) and rel_err(g0, ref) <= TOL_REGRESS
        assert np.all(a0[con == 0] == 0) and a0.any()
        sh = BatchedConvexQPSolver.shift_active_set(a0)
        g2, st2, it2, _ = s.solve_warm(rec, con, act_in=sh, normals=n)
        err = rel_err(g2, ref)
        print(f"H={H} {'terrain' if terrain else 'flat'}: warm from the shifted set {err:.3e}, cold {rel_err(g0, ref):.3e}")
        assert np.all(st2 == 0) and err <= TOL_REGRESS


def test_device_path_equals_host_path(torch_dev):
    """64 QPs are within one per SIMD: the device path runs the fused dense + Riccati launch.  Same bits as the host
    path, which is checked against the oracle."""
    import torch

    name, H, count = "everything", 10, 64
    rec, con, nrm = PS.batch(name, H, count)
    grf_h, it_h = solve_and_check(name, H, count, True, "host path")
    s = BatchedConvexQPSolver(PS.params(name), H, max_batch=0)
    out = torch.empty((count, H, 12), dtype=torch.float64, device=torch_dev)
    st = torch.empty(count, dtype=torch.int32, device=torch_dev)
    it = torch.empty(count, dtype=torch.int32, device=torch_dev)
    s.solve_device(torch.from_numpy(rec.copy()).to(torch_dev), torch.from_numpy(con.copy()).to(torch_dev), out, st, it,
                   normals=torch.from_numpy(nrm.copy()).to(torch_dev))
    torch.cuda.synchronize()
    assert np.all(st.cpu().numpy() == 0)
    assert np.array_equal(out.cpu().numpy(), grf_h) and np.array_equal(it.cpu().numpy(), it_h)


@pytest.mark.parametrize("mode", ["ipm", "off"])
def test_set_params_on_a_live_context(mode):
    """lmpc_set_params replaces every parameter the kernels read: Go1 -> everything -> Go1 on one context gives the
    bits of fresh contexts, and a refused set leaves the context as it was."""
    H, count = 10, 64
    rec, con, nrm = PS.batch("go1", H, count)
    s = BatchedConvexQPSolver(PS.params("go1"), H, max_batch=count, dense_path=mode)
    g1, st1, it1 = s.solve(rec, con, normals=nrm)
    s.set_params(PS.params("everything"))
    g2, st2, it2 = s.solve(rec, con, normals=nrm)
    gf, stf, itf = BatchedConvexQPSolver(PS.params("everything"), H, max_batch=count, dense_path=mode).solve(
        rec, con, normals=nrm)
    assert np.all(st1 == 0) and np.all(st2 == 0) and np.all(stf == 0)
    assert np.array_equal(g2, gf) and np.array_equal(it2, itf)
    assert rel_err(g2, PS.solve_ref(PS.vector("everything"), H, rec, con, nrm)) <= TOL_REGRESS
    assert np.abs(g2 - g1).max() > 1e-3  # the sets do pose different problems
    for field, i, value in (("trunk_inertia", 4, 0.0), ("trunk_inertia", 1, np.nan), ("r_weights", 5, np.inf)):
        bad = PS.params("everything")
        getattr(bad, field)[i] = value  # singular inertia, non-finite inertia, non-finite r
        assert N.lib().lmpc_set_params(s._ctx, ctypes.byref(bad)) == -1
    g2b, _, _ = s.solve(rec, con, normals=nrm)
    assert np.array_equal(g2b, g2)
    for name in PS.NAMES:  # every set is accepted on a live context (set_params raises otherwise)
        s.set_params(PS.params(name))
    s.set_params(PS.params("go1"))
    g3, st3, it3 = s.solve(rec, con, normals=nrm)
    assert np.array_equal(g3, g1) and np.array_equal(st3, st1) and np.array_equal(it3, it1)
    assert rel_err(g1, PS.reference("go1", H, count, True)) <= TOL_REGRESS


@pytest.mark.parametrize("mode", ["ipm", "gi", "off"])
@TERRAIN
def test_slippery_capped_trot_batch(terrain, mode):
    """`slippery_capped` on 64 trot QPs (config 2) at H = 10, every one dense-eligible: the batch on which the cap
    binds on most stance leg-steps (test_slippery_capped_bound_is_active), on both dense kernels and the Riccati one."""
    _, con, _ = PS.batch("slippery_capped", 10, 64, 2)
    assert np.all(con.sum((1, 2)) == 20)
    solve_and_check("slippery_capped", 10, 64, terrain, f"trot batch, dense={mode}", cid=2, dense_path=mode)


def test_slippery_capped_bound_is_active():
    """On the reference, no kernel involved: under mu = 0.1, f_max = 60 on flat ground more than half of the stance
    leg-steps of the oracle's answer sit at f_max, so that the set keeps testing the bound rows.

    This holds where the gait leaves two legs in stance: two legs at the cap give 120 N against the robot's 127.4 N
    weight, so a trot presses both to f_max -- config 2's 64 trots, the batch of test_slippery_capped_trot_batch
    (655 of 1280 stance leg-steps, 51 %).  It cannot hold on the mixed-gait batch of
    test_mixed_batch_every_dense_path: its crawl and stand QPs share the weight among three or four legs, 32-42 N
    each, under the cap (670 of 1756 at f_max, 38 %, against 82 under the Go1 preset; the cap or a pyramid face is
    active on 1743).  That count is printed and not asserted."""
    v = PS.vector("slippery_capped")
    assert 2 * v[35] < v[24] * v[36] < 3 * v[35]  # two legs at the cap cannot carry the weight, three can

    def at_cap(cid):
        _, con, _ = PS.batch("slippery_capped", 10, 64, cid)
        fz = PS.reference("slippery_capped", 10, 64, False, cid).reshape(64, 10, 4, 3)[..., 2]
        stance = con.astype(bool)
        assert np.all(fz[~stance] == 0.0)
        return int((np.abs(fz[stance] - v[35]) <= 1e-9 * v[35]).sum()), int(stance.sum())

    n, total = at_cap(2)
    m, mixed_total = at_cap(4)
    print(f"at f_max: {n} of {total} stance leg-steps of the trot batch, {m} of {mixed_total} of the mixed batch")
    assert n > 0.5 * total
