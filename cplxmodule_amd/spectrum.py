"""Welch power spectra on the fused HIP FFT kernels (csrc/spectrum.hip): the autograd Function and the launch glue behind
cplxmodule_amd.utils.spectrum (reference: cplxmodule/utils/spectrum.py:7-82).

A signal enters as two real planes (re, im) that share one strided layout: the two halves of `torch.view_as_real` of a
complex tensor or of a `[..., T, 2]` real tensor (x_i = x_r + 1 element), or the planes of a `Cplx`.  The dimensions
other than the signal's are collapsed into one row stride when the strides allow it; otherwise the planes are copied
once into a [rows, T] layout first (a differentiable copy: the gradient still reaches the input).  The workspace comes
from torch's caching allocator, and nothing here reads a device value on the host, so the calls can be captured in a
hipGraph.
"""
import ctypes
import functools
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from .ops import once_differentiable

MAX_N = 1 << 22                       # CPLXAMD_WELCH_MAX_N
SCALING = {"density": 0, "spectrum": 1}
PATHS = ("direct", "four-step", "bluestein", "bluestein+four-step")   # cplxamd_welch_plan's return codes
_code = functools.partial(_lib.plane_code, "Welch spectra take float32, bfloat16 or float64 planes (complex64 / complex128)")


def compute_dtype(dtype):
    """dtype of the spectrum of planes of `dtype`: bf16 planes are computed in, and give, float32"""
    return torch.float64 if dtype == torch.float64 else torch.float32


def plan(n, rows, segments, dtype=torch.float32):
    """(path, forward workspace bytes, backward workspace bytes) of a Welch call -- a pure host call, no GPU needed.
    Raises CplxAmdError when n is outside [1, 2^22]."""
    fwd, bwd = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib.load().cplxamd_welch_plan(int(n), int(rows), int(segments), _code(dtype), ctypes.byref(fwd),
                                        ctypes.byref(bwd))
    if rc < 0:
        raise CplxAmdError(f"Welch: segment length {n} is outside [1, 2^22 = {MAX_N}], the transform lengths the "
                           "kernels support")
    return PATHS[rc], fwd.value, bwd.value


def _rows_stride(shape, strides):
    """one stride that walks the dims `shape` (row-major) as a flat row index, or None"""
    dims = [(n, s) for n, s in zip(shape, strides) if n != 1]
    if not dims:
        return 0
    for (_, s_out), (n_in, s_in) in zip(dims[:-1], dims[1:]):
        if s_out != s_in * n_in:
            return None
    return dims[-1][1]


def _layout(pr, pi, dim):
    """-> (pr, pi, dim, row stride, element stride): the planes share one layout whose non-`dim` dims form rows;
    otherwise both are copied (differentiably) with the signal last."""
    if pr.stride() == pi.stride() and pr.dtype == pi.dtype and pr.stride(dim) >= 1:
        rs = _rows_stride([n for d, n in enumerate(pr.shape) if d != dim],
                          [s for d, s in enumerate(pr.stride()) if d != dim])
        if rs is not None:
            return pr, pi, dim, rs, pr.stride(dim)
    pr = pr.movedim(dim, -1).contiguous()
    pi = pi.movedim(dim, -1).to(pr.dtype).contiguous()
    return pr, pi, pr.dim() - 1, pr.shape[-1], 1


class _Welch(torch.autograd.Function):
    """Pxx = mean_s |FFT(w . x_s)|^2 / scale of planes pr, pi -> [rows..., n]; the gradient goes to pr and pi."""

    @staticmethod
    def forward(ctx, pr, pi, window, meta):
        rows, T, rs, es, n, step, scaling, fs, dim = meta
        S = (T - n) // step + 1
        _, ws_bytes, _ = plan(n, rows, S, pr.dtype)
        shape = [s for d, s in enumerate(pr.shape) if d != dim]
        out = torch.empty(rows, n, dtype=compute_dtype(pr.dtype), device=pr.device)
        if rows:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pr.device)
            call("cplxamd_welch_fwd", ptr(pr), ptr(pi), rs, es, rows, T, ptr(window), n, step, scaling, fs, ptr(out),
                 ptr(ws), ws_bytes, _code(pr.dtype), stream_ptr())
        ctx.save_for_backward(pr, pi, window)
        ctx.meta = meta
        return out.reshape(*shape, n)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pr, pi, window = ctx.saved_tensors
        rows, T, rs, es, n, step, scaling, fs, dim = ctx.meta
        S = (T - n) // step + 1
        _, _, ws_bytes = plan(n, rows, S, pr.dtype)
        g = g.reshape(rows, n).to(compute_dtype(pr.dtype)).contiguous()
        dx = torch.empty(rows, T, 2, dtype=pr.dtype, device=pr.device)
        if rows:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pr.device)
            base = dx.data_ptr()
            call("cplxamd_welch_bwd", ptr(pr), ptr(pi), rs, es, rows, T, ptr(window), n, step, scaling, fs, ptr(g),
                 ctypes.c_void_p(base), ctypes.c_void_p(base + dx.element_size()), 2 * T, 2, ptr(ws), ws_bytes,
                 _code(pr.dtype), stream_ptr())
        shape = [s for d, s in enumerate(pr.shape) if d != dim]
        back = [dx[..., k].reshape(*shape, T).movedim(-1, dim) for k in (0, 1)]
        return back[0], back[1], None, None


def welch(pr, pi, dim, window, fs, scaling, step):
    """Welch spectrum of the signal with planes pr, pi along `dim` (non-negative), segments of len(window) every `step`
    samples: [pr.shape without dim..., n] in float32 (float32 / bf16 planes) or float64 (float64 planes, or a float64
    window, which promotes the computation as x * window does in the reference)."""
    require_device(pr, pi, window)
    if window.requires_grad:
        raise CplxAmdError("pwelch: no gradient with respect to the window is computed here; pass window.detach()")
    if window.dim() != 1:
        raise CplxAmdError(f"pwelch: the window must be one-dimensional, got shape {tuple(window.shape)}")
    n = window.shape[0]
    _code(pr.dtype)
    if n > MAX_N:
        raise CplxAmdError(f"pwelch: window length {n} exceeds 2^22 = {MAX_N}, the longest transform supported")
    cdt = compute_dtype(pr.dtype)
    if window.is_floating_point() and torch.promote_types(cdt, window.dtype) == torch.float64 and cdt != torch.float64:
        pr, pi = pr.to(torch.float64), pi.to(torch.float64)   # x * window promotes to complex128 in the reference
        cdt = torch.float64
    window = window.to(cdt).contiguous()
    pr, pi, dim, rs, es = _layout(pr, pi, dim)
    T = pr.shape[dim]
    rows = math.prod(s for d, s in enumerate(pr.shape) if d != dim)
    return _Welch.apply(pr, pi, window, (rows, T, rs, es, n, step, SCALING[scaling], float(fs), dim))
