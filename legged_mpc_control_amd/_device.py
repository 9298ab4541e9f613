"""Device arguments of the Python wrappers, written once (DESIGN.md "Device arguments").

The C functions behind the wrappers trust the raw pointers they are handed: a tensor of another dtype, shape, layout
or device is not a Python error there but an out-of-bounds device access.  Every device entry point of the package
takes its batch and device, checks its tensors, and makes its pointers and its stream handle with the functions below
and with nothing else.  They raise ValueError and keep no state.  The two host-view helpers at the end turn a packed
device (or NumPy) buffer into a structured array or a ctypes array.
"""
from __future__ import annotations

import numpy as np


def batch(name, t, max_batch=None, device=None):
    """(B, torch.device) of a call from its leading tensor `t`: the tensor's own device, or `device` (an index or a
    torch.device) where a context owns it.  max_batch: B must lie in 1..max_batch."""
    if t is None or not getattr(t, "is_cuda", False) or t.dim() < 1:
        raise ValueError(f"{name}: expected a device tensor with a leading batch dimension")
    B = int(t.shape[0])
    if max_batch is not None and not 1 <= B <= max_batch:
        raise ValueError(f"{name}: batch {B} outside 1..{max_batch}")
    if device is None:
        return B, t.device
    if isinstance(device, int):
        import torch

        device = torch.device("cuda", device)
    return B, device


def check(name, t, dtype, shape, device, allow_shape=None, optional=False):
    """A raw pointer handed to the device path must be a contiguous tensor of this dtype and shape (or `allow_shape`)
    on the call's device: anything else turns into out-of-bounds device writes or wrong results.  optional: None
    passes."""
    if t is None and optional:
        return
    _on_device(name, t, dtype, device)
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if tuple(t.shape) != tuple(shape) and (allow_shape is None or tuple(t.shape) != tuple(allow_shape)):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")


def view(name, t, dtype, B, width, device, optional=False) -> int:
    """A strided argument: [B][width] with unit stride within a row and any row stride >= width, or (width None) [B]
    with any stride >= 1; with B == 1 the row stride is not read and may be anything.  -> the stride between robots in
    elements, as the C function wants it (width, or 1, for B == 1; 0 for an optional None)."""
    if t is None and optional:
        return 0
    _on_device(name, t, dtype, device)
    shape, least = ((B,), 1) if width is None else ((B, width), width)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
    if (width is not None and t.stride(1) != 1) or (B > 1 and t.stride(0) < least):
        raise ValueError(f"{name}: strides {tuple(t.stride())}, expected (>= {least}{'' if width is None else ', 1'})")
    return int(t.stride(0)) if B > 1 else least


def _on_device(name, t, dtype, device):
    if t is None or not getattr(t, "is_cuda", False):
        raise ValueError(f"{name}: expected a device tensor")
    if t.device != device:
        raise ValueError(f"{name}: on {t.device}, the call is on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")


def ptr(t):
    """The device address, or None: either converts by itself where the C function's argtypes say c_void_p."""
    return None if t is None else t.data_ptr()


def stream(s, device) -> int:
    """The hipStream_t handle of `s`: a torch stream, a raw handle (int), or None = torch's current stream on `device`."""
    if s is None or hasattr(s, "cuda_stream"):
        return torch_stream(s, device).cuda_stream
    return int(s)


def torch_stream(s, device):
    """The torch stream object of `s`, for the entry points that enter `torch.cuda.stream(s)`: a torch stream or None
    as in `stream`; a raw handle cannot be entered and is a ValueError."""
    if s is None:
        import torch

        return torch.cuda.current_stream(device)
    if not hasattr(s, "cuda_stream"):
        raise ValueError("stream: this entry point enters torch.cuda.stream(s): a torch stream or None, not a raw handle")
    return s


def host_view(buf, dtype) -> np.ndarray:
    """uint8 [..., dtype.itemsize] (torch or NumPy) -> NumPy structured array [...] of `dtype` (a copy for a tensor)."""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    return np.ascontiguousarray(a, dtype=np.uint8).view(dtype)[..., 0]


def host_structs(buf, ctype):
    """uint8 [..., sizeof(ctype)] (torch or NumPy) -> flat ctypes array of `ctype` (a copy on the host)."""
    import ctypes

    a = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, ctypes.sizeof(ctype))
    return (ctype * a.shape[0]).from_buffer_copy(a.tobytes())
