"""The device-argument helpers of the Python wrappers (legged_mpc_control_amd/_device.py) on a stand-in for a device
tensor: every rule of DESIGN.md "Device arguments" without a device.  Then the layout of the hand-written NumPy dtypes
of the packed structs against their ctypes structs, leaf field by leaf field."""
import ctypes

import numpy as np
import pytest
import torch

from legged_mpc_control_amd import _device as D
from legged_mpc_control_amd import _native as N

DEV0, DEV1 = torch.device("cuda", 0), torch.device("cuda", 1)


class FakeTensor:
    """What the helpers read of a torch device tensor, and nothing else."""

    def __init__(self, shape, dtype=torch.float64, strides=None, device=DEV0, ptr=0x7F0000001000):
        self.is_cuda, self.device, self.dtype, self.shape = True, device, dtype, tuple(shape)
        self._strides = tuple(strides) if strides is not None else self._packed()
        self._ptr = ptr

    def _packed(self):
        out, n = [], 1
        for s in reversed(self.shape):
            out.append(n)
            n *= s
        return tuple(reversed(out))

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def is_contiguous(self):
        return all(n == 1 or s == p for n, s, p in zip(self.shape, self._strides, self._packed()))

    def data_ptr(self):
        return self._ptr


# ---- accepted ----------------------------------------------------------------------------------------------------
def test_batch_takes_the_tensors_device_or_the_contexts():
    t = FakeTensor((5, 7), device=DEV1)
    assert D.batch("t", t) == (5, DEV1)
    assert D.batch("t", t, device=0) == (5, DEV0)  # a context's index: the contiguous check then rejects t
    assert D.batch("t", t, device=DEV1) == (5, DEV1)
    assert D.batch("t", t, max_batch=5) == (5, DEV1)


def test_check_accepts_exact_contiguous_allow_shape_and_optional_none():
    D.check("t", FakeTensor((3, 4, 2)), torch.float64, (3, 4, 2), DEV0)
    D.check("t", FakeTensor((3, 0)), torch.float64, (3, 1), DEV0, allow_shape=(3, 0))
    D.check("t", FakeTensor((3,), torch.int32), torch.int32, [3], DEV0)
    D.check("t", None, torch.int32, (3,), DEV0, optional=True)


def test_view_accepts_strided_rows_and_returns_the_element_stride():
    assert D.view("t", FakeTensor((4, 12)), torch.float64, 4, 12, DEV0) == 12
    assert D.view("t", FakeTensor((4, 12), strides=(42, 1)), torch.float64, 4, 12, DEV0) == 42
    assert D.view("t", FakeTensor((4,), torch.int32), torch.int32, 4, None, DEV0) == 1
    assert D.view("t", FakeTensor((4,), torch.int32, strides=(240,)), torch.int32, 4, None, DEV0) == 240
    assert D.view("t", None, torch.int32, 4, None, DEV0, optional=True) == 0


@pytest.mark.parametrize("row_stride", [0, 1, 5, 12, 1000])
def test_view_of_one_robot_ignores_the_row_stride(row_stride):
    assert D.view("t", FakeTensor((1, 12), strides=(row_stride, 1)), torch.float64, 1, 12, DEV0) == 12
    assert D.view("t", FakeTensor((1,), torch.int32, strides=(row_stride,)), torch.int32, 1, None, DEV0) == 1


def test_ptr():
    assert D.ptr(None) is None
    p = D.ptr(FakeTensor((2, 2), ptr=0x7F00DEAD0000))
    assert type(p) is int and p == 0x7F00DEAD0000


def test_stream_takes_a_torch_stream_or_a_raw_handle():
    class FakeStream:
        cuda_stream = 0x5EED

    assert D.stream(FakeStream(), DEV0) == 0x5EED
    assert D.stream(0x1234, DEV0) == 0x1234
    assert D.stream(0, DEV0) == 0  # the null stream as a raw handle
    s = FakeStream()
    assert D.torch_stream(s, DEV0) is s
    with pytest.raises(ValueError, match="stream"):
        D.torch_stream(0x1234, DEV0)


# ---- rejected: each a ValueError that names the argument -------------------------------------------------------------
def _rejects(fn, *args, **kw):
    with pytest.raises(ValueError, match="d_arg"):
        fn("d_arg", *args, **kw)


CPU = torch.zeros((3, 4), dtype=torch.float64)


@pytest.mark.parametrize("t", [None, CPU, "not a tensor", 3, np.zeros((3, 4))])
def test_none_host_tensors_and_non_tensors_are_rejected(t):
    _rejects(D.batch, t)
    _rejects(D.check, t, torch.float64, (3, 4), DEV0)
    _rejects(D.view, t, torch.float64, 3, 4, DEV0)
    if t is not None:
        _rejects(D.check, t, torch.float64, (3, 4), DEV0, optional=True)
        _rejects(D.view, t, torch.float64, 3, 4, DEV0, optional=True)


def test_batch_rejects_zero_dim_and_batches_outside_the_range():
    _rejects(D.batch, FakeTensor(()))
    _rejects(D.batch, FakeTensor((0, 4)), max_batch=8)
    _rejects(D.batch, FakeTensor((9, 4)), max_batch=8)
    assert D.batch("d_arg", FakeTensor((8, 4)), max_batch=8)[0] == 8
    assert D.batch("d_arg", FakeTensor((1, 4)), max_batch=8)[0] == 1


@pytest.mark.parametrize("t", [
    FakeTensor((3, 4), device=DEV1),             # the wrong device
    FakeTensor((3, 4), torch.float32),           # the wrong dtype
    FakeTensor((3, 4), torch.int64),
    FakeTensor((12,)),                           # the wrong rank
    FakeTensor((3, 4, 1)),
    FakeTensor(()),
    FakeTensor((4, 4)),                          # one row too many
    FakeTensor((2, 4)),                          # one too few
    FakeTensor((3, 5)), FakeTensor((3, 3)),      # the wrong width
], ids=lambda t: f"{t.device}-{t.dtype}-{t.shape}")
def test_check_and_view_reject(t):
    _rejects(D.check, t, torch.float64, (3, 4), DEV0)
    _rejects(D.check, t, torch.float64, (3, 4), DEV0, allow_shape=(3, 0), optional=True)
    _rejects(D.view, t, torch.float64, 3, 4, DEV0)
    _rejects(D.view, t, torch.float64, 3, 4, DEV0, optional=True)


@pytest.mark.parametrize("strides", [(8, 2), (4, 2), (1, 3), (16, 1), (0, 1)])
def test_check_rejects_every_view_that_is_not_packed(strides):
    _rejects(D.check, FakeTensor((3, 4), strides=strides), torch.float64, (3, 4), DEV0)


@pytest.mark.parametrize("strides", [(8, 2), (4, 2), (4, 0), (3, 1), (0, 1), (-4, 1)])
def test_view_rejects_inner_strides_other_than_one_and_overlapping_rows(strides):
    _rejects(D.view, FakeTensor((3, 4), strides=strides), torch.float64, 3, 4, DEV0)


def test_view_rejects_inner_stride_two_even_for_one_robot():
    _rejects(D.view, FakeTensor((1, 4), strides=(8, 2)), torch.float64, 1, 4, DEV0)


@pytest.mark.parametrize("stride", [0, -1])
def test_view_rejects_a_one_dimensional_view_that_does_not_advance(stride):
    _rejects(D.view, FakeTensor((3,), torch.int32, strides=(stride,)), torch.int32, 3, None, DEV0)


@pytest.mark.parametrize("shape", [(4,), (2,), (3, 1), ()])
def test_view_rejects_one_dimensional_shapes_other_than_the_batch(shape):
    _rejects(D.view, FakeTensor(shape, torch.int32), torch.int32, 3, None, DEV0)


def test_the_published_name_of_the_check_is_the_check():
    from legged_mpc_control_amd import hoqp

    assert hoqp.check_device_tensor is D.check


# ---- host views ------------------------------------------------------------------------------------------------------
def test_host_view_and_host_structs_take_tensors_and_arrays():
    from legged_mpc_control_amd import lowlevel as LL

    raw = np.arange(2 * 3 * LL.OUT_BYTES, dtype=np.uint64).astype(np.uint8).reshape(2, 3, LL.OUT_BYTES)
    for buf in (raw, torch.from_numpy(raw), raw[:, ::2]):
        v = D.host_view(buf, LL.OUT_DTYPE)
        assert v.shape == buf.shape[:-1] and v.dtype == LL.OUT_DTYPE
        arr = D.host_structs(buf, N.LmpcLowlevelOut)
        assert len(arr) == v.size
        assert bytes(arr) == np.ascontiguousarray(np.asarray(buf)).tobytes() == v.tobytes()


# ---- the hand-written dtypes against the ctypes structs -----------------------------------------------------------------
def _ctypes_leaves(ctype, base=0):
    """[(offset, NumPy type string, element count)] of the scalar and array-of-scalar fields, nested structs opened."""
    out = []
    for name, ftype in ctype._fields_:
        off, count = base + getattr(ctype, name).offset, 1
        while issubclass(ftype, ctypes.Array):
            count, ftype = count * ftype._length_, ftype._type_
        if issubclass(ftype, ctypes.Structure):
            assert count == 1, "an array of structs has no flat NumPy counterpart here"
            out += _ctypes_leaves(ftype, off)
        else:
            out.append((off, np.dtype(ftype).str, count))
    return out


def _numpy_leaves(dtype):
    out = []
    for name in dtype.names:
        ftype, off = dtype.fields[name][:2]
        base, shape = ftype.subdtype if ftype.subdtype is not None else (ftype, ())
        assert base.names is None
        out.append((off, base.str, int(np.prod(shape, dtype=np.int64))))
    return out


def _dtype_cases():
    from legged_mpc_control_amd import est, lowlevel, rollout, stack

    return [("est.FILTER_DTYPE", est.FILTER_DTYPE, N.LmpcEstFilter),
            ("est.SENSORS_DTYPE", est.SENSORS_DTYPE, N.LmpcEstSensors),
            ("est.OUT_DTYPE", est.OUT_DTYPE, N.LmpcEstOut),
            ("lowlevel.OUT_DTYPE", lowlevel.OUT_DTYPE, N.LmpcLowlevelOut),
            ("stack.STACK_ROBOT_DTYPE", stack.STACK_ROBOT_DTYPE, N.LmpcStackRobot),
            ("rollout.ROBOT_DTYPE", rollout.ROBOT_DTYPE, N.LmpcRobot),
            ("rollout.COMMAND_DTYPE", rollout.COMMAND_DTYPE, N.LmpcCommand)]


@pytest.mark.parametrize("case", _dtype_cases(), ids=lambda c: c[0])
def test_hand_written_dtype_matches_its_ctypes_struct(case):
    _, dtype, ctype = case
    assert dtype.itemsize == ctypes.sizeof(ctype)
    want, got = _ctypes_leaves(ctype), _numpy_leaves(dtype)
    assert len(got) == len(want)
    for position, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"leaf {position} ({dtype.names[position]}): dtype {g}, struct {w}"


def test_sim_flags_view_is_the_tail_of_the_struct():
    from legged_mpc_control_amd import sim

    raw = np.zeros((2, 3, sim.OUT_BYTES), dtype=np.uint8)
    words = raw.view(np.int32)
    words[..., N.LmpcSimOut.held.offset // 4:N.LmpcSimOut.held.offset // 4 + 4] = (1, 2, 3, 4)
    words[..., N.LmpcSimOut.touch.offset // 4:N.LmpcSimOut.touch.offset // 4 + 4] = (5, 6, 7, 8)
    words[..., N.LmpcSimOut.status.offset // 4] = 9
    flags = sim.flags_view(torch.from_numpy(raw))
    assert tuple(flags.shape) == (2, 3, 10)
    assert flags[1, 2].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 0]
    assert ctypes.sizeof(N.LmpcSimOut) == N.LmpcSimOut.held.offset + 40
