"""Real-input and real-output Fourier transforms on the half-length kernels of csrc/rfft.hip: the argument handling, the
launch glue and the two autograd Functions behind cplx.rfft / irfft / rfft2 / irfft2 / rfftn / irfftn / hfft / ihfft.

Two linear primitives (h = n // 2; w_k = 1 at k = 0 and, n even, k = h, else 2; sg the sign of the exponent):
    R2C   y_k = scale [w_k] sum_j x_j e^{sg 2 pi i jk/n},       k <= h      real plane -> plane pair
    C2R   x_j = scale Re sum_k c_k X_k e^{sg 2 pi i jk/n},      j < n       plane pair -> real plane; c = w or c = 1
rfft is R2C (sg -), ihfft R2C (sg +), irfft C2R (sg +, c = w), hfft C2R (sg -, c = w).  They are each other's adjoints:
with autograd's convention (dL/dre + i dL/dim) the gradient of R2C is C2R of the incoming gradient with the opposite
sign, the same scale and c = w exactly when the R2C was weighted -- for rfft c = 1: NOT irfft --, and the gradient of
C2R is R2C with the opposite sign, weighted exactly when c = w.  Each backward is the other Function, so derivatives of
every order exist.  The adjoint of zero padding is `narrow`; truncation is a view.

One launch of `cplxamd_rfft` transforms every vector along ONE dim, reading the planes where they lie (runs and layouts
as cplxmodule_amd/fft.py, by _runs.py's rule; one differentiable copy only when planes share no layout or need more than three runs).  The
output is dense in the input's memory order.  rfftn is the R2C launch along the LAST listed dim, then fft.py's complex
launches over the others; irfftn the complex inverses first, the C2R launch last; for bf16 the intermediates are float32
and the result is rounded once.  The workspace comes from torch's allocator, no device value is read on the host.
"""
import ctypes

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, fill, fit_like
from .fft import MAX_N, PATHS, _arguments, _scale, transform

FLAG_INVERSE, FLAG_C2R, FLAG_WEIGHTED = 1, 4, 8                       # CPLXAMD_FFT_INVERSE, CPLXAMD_RFFT_C2R, CPLXAMD_RFFT_WEIGHTED


def plan(n, vectors, dtype=torch.float32, c2r=False):
    """(path, length of the complex transform, points actually run, vectors per workgroup, workspace bytes) of a real
    transform of length n -- a pure host call, no GPU needed.  Even n runs n / 2 complex points."""
    cn, pts, vpw, ws = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().cplxamd_rfft_plan(int(n), int(vectors), code(dtype), int(bool(c2r)), ctypes.byref(cn), ctypes.byref(pts),
                                       ctypes.byref(vpw), ctypes.byref(ws))
    if rc < 0:
        raise CplxAmdError(f"rfft: transform length {n} is outside [1, 2^22 = {MAX_N}], the lengths the kernels support")
    return PATHS[rc], cn.value, pts.value, vpw.value, ws.value


def _launch(xr, xi, yr, yi, n, n_in, dim, flags, scale, c2r, batch):
    d = _lib.FftDesc(n=n, n_in=n_in, x_es=xr.stride(dim), y_es=yr.stride(dim), inverse=flags, scale=scale)
    vectors, _ = fill(d, batch, ("x_stride", "y_stride"))
    ws_bytes = plan(n, vectors, xr.dtype, c2r)[4]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xr.device)
    call("cplxamd_rfft", ptr(xr), ptr(xi), ptr(yr), ptr(yi), ctypes.byref(d), code(xr.dtype), code(yr.dtype), ptr(ws),
         ws_bytes, stream_ptr())


class _R2C(torch.autograd.Function):
    """(yr, yi)_k = scale [w_k] sum_j x_j e^{sg 2 pi i jk/n}, k <= n // 2, along `dim` of a real plane of at most three
    batch runs; the first min(n, extent) elements of every vector are read."""

    @staticmethod
    def forward(ctx, x, meta):
        n, dim, positive, weighted, scale, out_dtype, batch, ys = meta
        ctx.meta = meta[:5]
        ctx.src = (x.shape[dim], x.dtype)
        yr = torch.empty_strided(x.shape[:dim] + (n // 2 + 1,) + x.shape[dim + 1:], ys, dtype=out_dtype, device=x.device)
        yi = torch.empty_like(yr)
        if yr.numel():
            _launch(x, None, yr, yi, n, min(n, x.shape[dim]), dim, (FLAG_INVERSE if positive else 0) | (FLAG_WEIGHTED if weighted else 0),
                    scale, False, batch)
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        n, dim, positive, weighted, scale = ctx.meta
        extent, dtype = ctx.src
        dx = c2r(gr, gi, n, dim, not positive, weighted, scale, dtype)
        return (dx.narrow(dim, 0, extent) if extent < n else dx), None


class _C2R(torch.autograd.Function):
    """x_j = scale Re sum_k c_k X_k e^{sg 2 pi i jk/n}, j < n, along `dim` of planes that share one layout of at most
    three batch runs and hold at most n // 2 + 1 entries (fewer: zero padding); c = w (`weighted`) or 1."""

    @staticmethod
    def forward(ctx, pr, pi, meta):
        n, dim, positive, weighted, scale, out_dtype, batch, ys = meta
        ctx.meta = meta[:5]
        ctx.src = (pr.shape[dim], pr.dtype)
        y = torch.empty_strided(pr.shape[:dim] + (n,) + pr.shape[dim + 1:], ys, dtype=out_dtype, device=pr.device)
        if y.numel():
            _launch(pr, pi, y, None, n, pr.shape[dim], dim, FLAG_C2R | (FLAG_INVERSE if positive else 0) | (FLAG_WEIGHTED if weighted else 0),
                    scale, True, batch)
        return y

    @staticmethod
    def backward(ctx, g):
        n, dim, positive, weighted, scale = ctx.meta
        extent, dtype = ctx.src
        dr, di = r2c(g, n, dim, not positive, weighted, scale, dtype)
        if extent < n // 2 + 1:                           # the adjoint of zero padding
            dr, di = dr.narrow(dim, 0, extent), di.narrow(dim, 0, extent)
        return dr, di, None


def r2c(x, n, dim, positive, weighted, scale, out_dtype):
    """the R2C primitive along `dim` (non-negative) of a real tensor -> planes of `out_dtype` with n // 2 + 1 entries"""
    if x.shape[dim] > n:                                  # truncation: a view (autograd pads its gradient)
        x = x.narrow(dim, 0, n)
    x, _, batch, ys = fit_like(x, None, dim, n // 2 + 1)  # at most one differentiable copy
    return _R2C.apply(x, (n, dim, bool(positive), bool(weighted), float(scale), out_dtype, batch, ys))


def c2r(pr, pi, n, dim, positive, weighted, scale, out_dtype):
    """the C2R primitive along `dim` (non-negative) of planes of one dtype and shape -> a real tensor of `out_dtype` with
    n entries; the first n // 2 + 1 entries are used"""
    if pr.shape[dim] > n // 2 + 1:
        pr, pi = pr.narrow(dim, 0, n // 2 + 1), pi.narrow(dim, 0, n // 2 + 1)
    pr, pi, batch, ys = fit_like(pr, pi, dim, n)          # at most one differentiable copy
    return _C2R.apply(pr, pi, (n, dim, bool(positive), bool(weighted), float(scale), out_dtype, batch, ys))


def arguments(input, s, dim, norm, name, real_out):
    """torch.fft's argument rules for the real transforms -> [(dim, n)] in the order of `dim`; for a real OUTPUT the n
    of the last listed dim is the output's length, 2 (m - 1) by default.  RuntimeError / IndexError as torch's."""
    todo = _arguments(input, s, dim, norm, name)
    if real_out:
        given = None if s is None else ([s] if isinstance(s, int) else list(s))[-1]
        if given is None or given == -1:
            d = todo[-1][0]
            n = 2 * (input.shape[d] - 1)
            if n < 1:
                raise RuntimeError(f"{name}: invalid number of data points ({n}) specified")
            todo[-1] = (d, n)
    return todo


def output_shape(name, shape, s=None, dim=None):
    """the shape cplx.<name> gives an input of `shape` (argument rules only: nothing is transformed)"""
    real_out = name.startswith(("irfft", "hfft"))
    if dim is None and name.endswith("2"):
        dim = (-2, -1)
    if dim is None and not name.endswith("n"):
        dim = -1
    todo = arguments(torch.empty(tuple(shape), device="meta"), s, dim, None, name, real_out)
    out = list(shape)
    for d, n in todo:
        out[d] = n
    if not real_out:
        out[todo[-1][0]] = todo[-1][1] // 2 + 1
    return tuple(out)


def _check_lengths(todo, name):
    for _, n in todo:
        if n > MAX_N:
            raise CplxAmdError(f"{name}: length {n} exceeds 2^22 = {MAX_N}, the longest transform supported")


def rfftn(input, s, dim, norm, positive, name):
    """real tensor -> planes of the half spectrum over the (dim, n) pairs torch.fft's rules give: R2C along the last
    listed dim, then the complex transforms over the others.  `positive`: the exponent's sign (ihfft)"""
    if not torch.is_tensor(input) or input.is_complex():
        raise CplxAmdError(f"{name}: the input is a {type(input).__name__}"
                           f"{' of complex dtype' if torch.is_tensor(input) else ''}, not a real torch.Tensor")
    todo = arguments(input, s, dim, norm, name, False)
    code(input.dtype)
    _check_lengths(todo, name)
    require_device(input)
    wide = torch.float32 if input.dtype == torch.bfloat16 else input.dtype
    d, n = todo[-1]
    pr, pi = r2c(input, n, d, positive, False, _scale(n, norm, positive), input.dtype if len(todo) == 1 else wide)
    for step, (d, n) in enumerate(reversed(todo[:-1])):
        out_dtype = input.dtype if step == len(todo) - 2 else wide
        pr, pi = transform(pr, pi, n, d, positive, _scale(n, norm, positive), out_dtype)
    return pr, pi


def irfftn(input, s, dim, norm, positive, name):
    """`Cplx` half spectrum -> real tensor: the complex transforms over all listed dims but the last, then C2R with the
    Hermitian extension along the last.  `positive`: the exponent's sign (False: hfft)"""
    from .cplx import Cplx
    if not isinstance(input, Cplx):
        raise CplxAmdError(f"{name}: the input is a {type(input).__name__}, not a Cplx (wrap planes with Cplx(re, im); "
                           "torch complex tensors are not taken)")
    todo = arguments(input, s, dim, norm, name, True)
    pr, pi = input.real, input.imag
    if pr.dtype != pi.dtype:
        raise CplxAmdError(f"{name}: the planes have different dtypes: {pr.dtype} and {pi.dtype}")
    code(pr.dtype)
    _check_lengths(todo, name)
    require_device(pr, pi)
    dtype = pr.dtype
    wide = torch.float32 if dtype == torch.bfloat16 else dtype
    d, n = todo[-1]
    if pr.shape[d] > n // 2 + 1:                          # what C2R will not read need not be transformed
        pr, pi = pr.narrow(d, 0, n // 2 + 1), pi.narrow(d, 0, n // 2 + 1)
    for dd, nn in reversed(todo[:-1]):
        pr, pi = transform(pr, pi, nn, dd, positive, _scale(nn, norm, positive), wide)
    return c2r(pr, pi, n, d, positive, True, _scale(n, norm, positive), dtype)
