"""Discrete Fourier transforms of planar `Cplx` tensors on the package's own FFT engine (csrc/fft.hip): the argument
handling, the launch glue and the autograd Function behind cplx.fft / ifft / fft2 / ifft2 / fftn / ifftn.

One launch of `cplxamd_fft` transforms every vector of a tensor along ONE dim, reading both planes where they lie:
the dims other than the transformed one are sorted by stride and fused into at most three batch runs, jointly for the
input and the output (_runs.py; a contiguous, channels-last, transposed, sliced or `expand`ed input needs no copy); planes
that share no layout, or that need more than three runs, are copied once, differentiably.  The output has the input's memory
order.  `n` larger than the extent is zero padding inside the kernel's loader, `n` smaller a `narrow` view.  A transform
over several dims is one launch per dim, the last listed dim first; for bf16 planes every intermediate is float32, so
the result is rounded once.

The transform is linear: with autograd's convention for complex values (dL/dre + i dL/dim) its adjoint is the same
transform with the opposite sign and the same scale, so the backward is the same Function applied to the incoming
gradient (in / out dtypes swapped), followed by the adjoint of the padding.  It is differentiable to any order.  The
workspace comes from torch's caching allocator and nothing reads a device value on the host: calls can be captured in
a hipGraph.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense_like, fill, fit_like, runs

MAX_N = 1 << 22                       # CPLXAMD_WELCH_MAX_N
PATHS = ("direct", "four-step", "bluestein", "bluestein+four-step")   # cplxamd_fft_plan's return codes
NORMS = (None, "backward", "ortho", "forward")
_ONE_PER_WORKGROUP = False            # private: True runs packed lengths with one vector per workgroup (scripts/bench_fft.py only)


def plan(n, vectors, dtype=torch.float32):
    """(path, vectors per workgroup, workspace bytes) of a length-n transform of `vectors` vectors whose input planes
    have `dtype` -- a pure host call, no GPU needed.  Raises CplxAmdError when n is outside [1, 2^22]."""
    vpw, ws = ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().cplxamd_fft_plan(int(n), int(vectors), code(dtype), ctypes.byref(vpw), ctypes.byref(ws))
    if rc < 0:
        raise CplxAmdError(f"fft: transform length {n} is outside [1, 2^22 = {MAX_N}], the lengths the kernels support")
    return PATHS[rc], vpw.value, ws.value


_dense_like = dense_like                              # the names the tests know the run rule of one skipped dim by
_runs = lambda shape, xs, ys, dim: runs(shape, (xs, ys), dim)        # noqa: E731


class _Transform(torch.autograd.Function):
    """(yr, yi) = scale * DFT_n along `dim` of planes (pr, pi) that share one layout of at most three batch runs; the
    first min(n, extent) elements of every vector are read."""

    @staticmethod
    def forward(ctx, pr, pi, meta):
        n, dim, inverse, scale, out_dtype, batch, ys = meta
        ctx.meta = meta[:4]
        ctx.src = (pr.shape[dim], pr.dtype)
        yr = torch.empty_strided(pr.shape[:dim] + (n,) + pr.shape[dim + 1:], ys, dtype=out_dtype, device=pr.device)
        yi = torch.empty_like(yr)
        if yr.numel() == 0:
            return yr, yi
        d = _lib.FftDesc(n=n, n_in=min(n, pr.shape[dim]), x_es=pr.stride(dim), y_es=yr.stride(dim),
                         inverse=(1 if inverse else 0) | (2 if _ONE_PER_WORKGROUP else 0), scale=scale)
        vectors, _ = fill(d, batch, ("x_stride", "y_stride"))
        _, _, ws_bytes = plan(n, vectors, pr.dtype)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pr.device)
        call("cplxamd_fft", ptr(pr), ptr(pi), ptr(yr), ptr(yi), ctypes.byref(d), code(pr.dtype), code(out_dtype),
             ptr(ws), ws_bytes, stream_ptr())
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        n, dim, inverse, scale = ctx.meta
        extent, dtype = ctx.src
        dr, di = transform(gr, gi, n, dim, not inverse, scale, dtype)
        if extent < n:                                    # the adjoint of zero padding
            dr, di = dr.narrow(dim, 0, extent), di.narrow(dim, 0, extent)
        return dr, di, None


def transform(pr, pi, n, dim, inverse, scale, out_dtype):
    """scale * DFT_n (inverse: the unnormalised inverse) along `dim` (non-negative) of planes pr, pi of one dtype and
    shape -> planes of `out_dtype`.  Differentiable to any order."""
    extent = pr.shape[dim]
    if extent > n:                                        # truncation: a view (autograd pads its gradient)
        pr, pi = pr.narrow(dim, 0, n), pi.narrow(dim, 0, n)
    pr, pi, batch, ys = fit_like(pr, pi, dim, n)          # at most one differentiable copy
    return _Transform.apply(pr, pi, (n, dim, bool(inverse), float(scale), out_dtype, batch, ys))


def _scale(n, norm, inverse):
    if norm == "ortho":
        return 1.0 / math.sqrt(n)
    if (norm == "forward") != inverse:                    # forward: the forward transform carries 1 / n; else the inverse
        return 1.0 / n
    return 1.0


def _arguments(input, s, dim, norm, name):
    """torch.fft's argument rules -> [(dim, n)], in the order of `dim`.  RuntimeError as torch raises them."""
    nd = input.real.dim()
    if norm not in NORMS:
        raise RuntimeError(f"{name}: invalid normalization mode: {norm!r} (expected 'backward', 'ortho' or 'forward')")
    if nd == 0:
        raise RuntimeError(f"{name}: the input has no dimension to transform")
    if s is not None:
        s = [int(v) for v in ([s] if isinstance(s, int) else s)]
    if dim is not None:
        dim = [int(v) for v in ([dim] if isinstance(dim, int) else dim)]
        for v in dim:
            if not -nd <= v < nd:
                raise IndexError(f"{name}: dimension out of range (expected to be in range of [{-nd}, {nd - 1}], got {v})")
        dim = [v % nd for v in dim]
        if len(set(dim)) != len(dim):
            raise RuntimeError(f"{name}: FFT dims must be unique")
    if s is not None and dim is not None and len(s) != len(dim):
        raise RuntimeError(f"{name}: when given, dim and shape arguments must have the same length")
    if dim is None:
        if s is not None and len(s) > nd:
            raise RuntimeError(f"{name}: got shape with {len(s)} values but input tensor only has {nd} dimensions")
        dim = list(range(nd)) if s is None else list(range(nd - len(s), nd))
    if s is None:
        s = [input.shape[d] for d in dim]
    s = [input.shape[d] if v == -1 else v for d, v in zip(dim, s)]
    for d, v in zip(dim, s):
        if v < 1 or input.shape[d] < 1:
            raise RuntimeError(f"{name}: invalid number of data points ({min(v, input.shape[d])}) specified")
    return list(zip(dim, s))


def fftn(input, s, dim, norm, inverse, name):
    """the transform of a `Cplx` over the (dim, n) pairs torch.fft's rules give, last listed dim first -> planes"""
    from .cplx import Cplx
    if not isinstance(input, Cplx):
        raise CplxAmdError(f"{name}: the input is a {type(input).__name__}, not a Cplx (wrap planes with Cplx(re, im); "
                           "torch complex tensors are not taken)")
    todo = _arguments(input, s, dim, norm, name)
    pr, pi = input.real, input.imag
    if pr.dtype != pi.dtype:
        raise CplxAmdError(f"{name}: the planes have different dtypes: {pr.dtype} and {pi.dtype}")
    code(pr.dtype)
    for _, n in todo:
        if n > MAX_N:
            raise CplxAmdError(f"{name}: length {n} exceeds 2^22 = {MAX_N}, the longest transform supported")
    require_device(pr, pi)
    wide = torch.float32 if pr.dtype == torch.bfloat16 else pr.dtype     # intermediates: bf16 planes round once, at the end
    for step, (d, n) in enumerate(reversed(todo)):
        out_dtype = input.real.dtype if step == len(todo) - 1 else wide
        pr, pi = transform(pr, pi, n, d, inverse, _scale(n, norm, inverse), out_dtype)
    return pr, pi
