"""CPU tests of the hierarchical QP's warm start (include/lmpc/lmpc_hoqp.h "Warm start"): the exports and the
active-set block's length, argument checks without a GPU, and the numpy prototype of the warm chain
(tools/hoqp_warm_proto.py) on the committed fixture tests/golden/hoqp_warm_golden.npz -- tick A solved cold, tick B
from tick A's active sets -- against the CPU restatement's answers (oracle/hoqp.py) at tests/test_gpu_hoqp.py's bar."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from legged_mpc_control_amd import _native as N
from test_gpu_hoqp import TOL, check_against, dims_from

sys.path.insert(0, os.path.join(ROOT, "tools"))


def fixture():
    return np.load(os.path.join(GOLDEN, "hoqp_warm_golden.npz"), allow_pickle=False)


def test_act_len_and_abi():
    lib = N.lib()
    assert lib.lmpc_hoqp_abi_version() == N.HOQP_ABI_VERSION == 2
    d = N.LmpcHoqpDims()
    lib.lmpc_hoqp_dims_wbc(ctypes.byref(d))
    assert lib.lmpc_hoqp_act_len(ctypes.byref(d)) == 15  # per level: a validity word and 2 x 128 flag bits
    one = N.LmpcHoqpDims()
    one.num_vars, one.num_levels = 8, 1
    one.eq_rows[0], one.ineq_rows[0] = 3, 5
    assert lib.lmpc_hoqp_act_len(ctypes.byref(one)) == 5
    bad = N.LmpcHoqpDims()
    bad.num_vars, bad.num_levels = 65, 1
    assert lib.lmpc_hoqp_act_len(ctypes.byref(bad)) < 0
    bad.num_vars, bad.num_levels = 8, 5
    assert lib.lmpc_hoqp_act_len(ctypes.byref(bad)) < 0
    bad.num_levels = 3
    bad.ineq_rows[0] = bad.ineq_rows[1] = bad.ineq_rows[2] = 60  # 180 stacked rows > 128
    assert lib.lmpc_hoqp_act_len(ctypes.byref(bad)) < 0
    assert lib.lmpc_hoqp_act_len(None) < 0


def test_options_and_argument_checks_without_gpu():
    lib = N.lib()
    o = N.LmpcHoqpOptions()
    lib.lmpc_hoqp_options_default(ctypes.byref(o))
    assert o.warm_rounds == 12 and o.crossover == 1 and o.max_iter == 60
    assert ctypes.sizeof(N.LmpcHoqpOptions) == 32  # warm_rounds sits in what was the struct's tail padding
    act = (ctypes.c_uint64 * 15)()
    assert lib.lmpc_hoqp_solve_batch_warm(None, None, 1, None, None, None, None, act) == -1
    assert lib.lmpc_hoqp_solve_device_warm(None, None, 1, None, None, None, None, None, None) == -1
    assert lib.lmpc_hoqp_set_options(None, ctypes.byref(o)) == -1


def test_fixture_shape_and_choice():
    g = fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "hoqp_warm_golden.npz")) <= 300_000
    assert g["rec_a"].shape == g["rec_b"].shape == (12, 4472)
    assert g["x_a"].shape == g["x_b"].shape == (12, 3, 42) and g["w_a"].shape == g["w_b"].shape == (12, 44)
    assert list(g["contact_changed"]) == [0] * 8 + [1] * 4
    # same contacts: level 0's swing-force rows (equalities 18..29) select the same forces; changed: they differ
    for k in range(12):
        same = np.array_equal(g["rec_a"][k][18 * 42:30 * 42] != 0.0, g["rec_b"][k][18 * 42:30 * 42] != 0.0)
        assert same == (g["contact_changed"][k] == 0), k
    # the 8 next-tick pairs were chosen so that the prototype takes every level warm in at most 2 repair rounds
    proto = g["proto"]
    assert np.all(proto[:8, :, 0] == 1) and np.all(proto[:8, :, 1] == 1) and np.all(proto[:8, :, 2] <= 2)
    assert np.all(proto[8:, :, 0] == 1)


@pytest.mark.parametrize("k", [0, 3, 5, 7])
def test_prototype_takes_every_level_warm_and_meets_the_oracle(k):
    import hoqp_warm_proto as WP

    g = fixture()
    dims = dims_from(g["dims"])
    ta, tb = WP.unpack(g["rec_a"][k], g["dims"]), WP.unpack(g["rec_b"][k], g["dims"])
    xa, wa, act, out_a = WP.warm_chain(ta)
    assert all(a is not None for a in act) and not any(o[0] for o in out_a)
    check_against(g["rec_a"][k], dims, np.stack(xa), np.concatenate(wa), g["x_a"][k], g["w_a"][k], True, TOL)
    xb, wb, _, out_b = WP.warm_chain(tb, act)
    assert all(o[0] and o[1] and o[2] <= 2 for o in out_b), out_b  # every level taken warm, as the fixture records
    check_against(g["rec_b"][k], dims, np.stack(xb), np.concatenate(wb), g["x_b"][k], g["w_b"][k], True, TOL)
    err = float(np.max(np.abs(xb[-1] - g["x_b"][k][-1])) / (1.0 + np.max(np.abs(g["x_b"][k][-1]))))
    print(f"pair {k}: warm prototype vs oracle, final x {err:.1e}")
