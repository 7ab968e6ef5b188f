"""Rational rate change along the last dim on the polyphase kernels of csrc/upfirdn.hip: the argument handling, the plan,
the filter design, the launch glue and the two autograd Functions behind cplx.upfirdn and cplx.resample_poly.

Write xu for x upsampled by `up`: xu[i up] = x[i], zero elsewhere and outside the row (never materialised).  Two
primitives, each an autograd Function whose backward calls the other's:
    P1 `conv`    y[n] = sum_k h[k] xu[n down + off - k]     (conj: y[n] = sum_k conj(h[k]) xu[n down + off + k]),  n < length
    P2 `wgrad`   y[k] = sum_rows sum_n conj(au[n down + off - k]) c[n],  k < K       summed over the rows that share a result
With autograd's convention (dL/dre + i dL/dim) and incoming gradient g the rates swap in every x-side gradient:
    P1 conv(x, h):  dx = P1 corr(g, h; down, up, -off),  dh = P2(x, g; up, down, off)
    P1 corr(x, h):  dx = P1 conv(g, h; down, up, -off),  dh = P2(g, x; down, up, -off)
    P2(a, c):       da = P1 corr(c, g; down, up, -off),  dc = P1 conv(a, g; up, down, off)
so derivatives of every order stay on the two kernels, and no pass flips, conjugates, zero-stuffs or copies an operand.
A real operand is a null imaginary plane (never read, no zero plane allocated; the kernels are compiled per operand
pair); the gradient of a real operand is the real part (the null output plane is not stored).

Leading dims broadcast by torch's rules and are read where they lie, under _runs.py's rule: at most three batch runs
jointly for both operands and the result, otherwise one differentiable copy.  The weight gradient's workspace comes from
torch's allocator and nothing reads a device value on the host: calls can be captured in a hipGraph.

Filters longer than 4096 taps take the COMPOSED path, which is not the hot path: the signal is zero-stuffed with torch,
convolved by cplx.fftconvolve and sliced with a step, all differentiable; it raises where fftconvolve would.
"""
import ctypes
import functools
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense, fill, fit, fit_wgrad, planes

PATHS = ("fused", "composed")                              # cplxamd_upfirdn_plan's return codes
FUSED_MAX_K = 4096


def plan(a_len, k, c_len, up=1, down=1, off=0, rows=1, filters=1, dtype=torch.float32, conj=False, a_cplx=True, b_cplx=True):
    """The plan of both primitives for rows of `a_len` entries, `k` taps and `c_len` results (P2: entries of c) -- a pure
    host call, no GPU needed -> dict: path ("fused" / "composed") and the fields of _lib.UPFIRDN_PLAN_FIELDS (tile,
    tiles per row and per workgroup, staged span, taps per phase and segment, LDS bytes, threads, grid; the weight
    gradient's tile, tap blocks, chunks and workspace bytes)."""
    out = (ctypes.c_int64 * len(_lib.UPFIRDN_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_upfirdn_plan(int(a_len), int(k), int(c_len), int(up), int(down), int(off), int(rows), int(filters),
                                          code(dtype), int(bool(conj)), int(bool(a_cplx)), int(bool(b_cplx)), out)
    if rc == -3:
        raise CplxAmdError(f"upfirdn: lengths {a_len}, {k}, {c_len} at rates {up}/{down} and offset {off} exceed what the "
                           "kernels index (rates up to 2^30, lengths up to 2^40, 2^31 - 1 workgroups)")
    if rc < 0:
        raise CplxAmdError(f"upfirdn: no plan for lengths {a_len}, {k}, {c_len} at rates {up}/{down} (all must be >= 1)")
    p = dict(zip(_lib.UPFIRDN_PLAN_FIELDS, out))
    p["path"] = PATHS[rc]
    return p


def _launch(name, ar, ai, br, bi, yr, yi, runs, a_len, k, c_len, up, down, off, conj, wgrad):
    """one call of cplxamd_upfirdn / _wgrad over the batch runs of (a, b, y); b is read with its broadcast strides"""
    d = _lib.UpfirdnDesc(a_len=a_len, k=k, c_len=c_len, up=up, down=down, off=off, a_es=ar.stride(-1), b_es=br.stride(-1),
                         conj=int(conj))
    rows, filters = fill(d, runs, ("a_stride", "b_stride", "y_stride"), "y_stride" if wgrad else "b_stride")
    args = (ptr(ar), ptr(ai), ptr(br), ptr(bi), ptr(yr), ptr(yi), ctypes.byref(d), code(ar.dtype))
    if not wgrad:
        return call(name, *args, stream_ptr())
    ws_bytes = plan(a_len, k, c_len, up, down, off, rows, filters, ar.dtype, False, ai is not None,
                    bi is not None)["wgrad_ws_bytes"]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ar.device)
    call(name, *args, ptr(ws), ws_bytes, stream_ptr())


class _P1(torch.autograd.Function):
    """(yr, yi) = the rate-changing conv / corr of x [*B, N] with the filter h [*Bh, K] (Bh broadcastable to B, same number
    of dims) at n < length; xi, hi may be None; yi is None unless `out_imag`."""

    @staticmethod
    def forward(ctx, xr, xi, hr, hi, meta):
        up, down, off, length, conj, out_imag, runs = meta
        ctx.meta = meta[:6]
        ctx.save_for_backward(xr, xi, hr, hi)
        yr = torch.empty(tuple(xr.shape[:-1]) + (length,), dtype=xr.dtype, device=xr.device)
        yi = torch.empty_like(yr) if out_imag else None
        if yr.numel():
            _launch("cplxamd_upfirdn", xr, xi, hr, hi, yr, yi, runs, xr.shape[-1], hr.shape[-1], length, up, down, off, conj,
                    False)
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        xr, xi, hr, hi = ctx.saved_tensors
        up, down, off, length, conj, out_imag = ctx.meta
        gi = gi if out_imag else None
        dx = dh = (None, None)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dx = conv(gr, gi, hr, hi, down, up, -off, xr.shape[-1], not conj, xi is not None)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            first, second, rates = ((gr, gi), (xr, xi), (down, up, -off)) if conj else ((xr, xi), (gr, gi), (up, down, off))
            dh = wgrad(*first, *second, *rates, hr.shape[-1], tuple(hr.shape[:-1]), hi is not None)
        return dx[0], dx[1], dh[0], dh[1], None


class _P2(torch.autograd.Function):
    """(yr, yi)[*F, k] = sum over the rows of B that F broadcasts over, and over n, of conj(au[n down + off - k]) c[n],
    k < K, for a [*B, A] and c [*B, C]; F has B's number of dims.  ai, ci may be None; yi is None unless `out_imag`."""

    @staticmethod
    def forward(ctx, ar, ai, cr, ci, meta):
        up, down, off, k, fshape, out_imag, runs = meta
        ctx.meta = meta[:6]
        ctx.save_for_backward(ar, ai, cr, ci)
        yr = torch.empty(fshape + (k,), dtype=ar.dtype, device=ar.device)
        yi = torch.empty_like(yr) if out_imag else None
        if yr.numel() and ar.numel():
            _launch("cplxamd_upfirdn_wgrad", ar, ai, cr, ci, yr, yi, runs, ar.shape[-1], k, cr.shape[-1], up, down, off, False,
                    True)
        elif yr.numel():                                  # no rows to sum
            yr.zero_()
            if yi is not None:
                yi.zero_()
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, cr, ci = ctx.saved_tensors
        up, down, off, k, fshape, out_imag = ctx.meta
        gi = gi if out_imag else None
        da = dc = (None, None)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            da = conv(cr, ci, gr, gi, down, up, -off, ar.shape[-1], True, ai is not None)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dc = conv(ar, ai, gr, gi, up, down, off, cr.shape[-1], False, ci is not None)
        return da[0], da[1], dc[0], dc[1], None


def conv(xr, xi, hr, hi, up, down, off, length, conj=False, out_imag=True):
    """P1 on planes: x [*B, N] (views welcome), filter h [*Bh, K] with Bh broadcastable to B and as many dims -> (yr, yi)
    of [*B, length], yi None unless `out_imag`.  Differentiable to any order."""
    shape = tuple(xr.shape[:-1]) + (length,)
    ((xr, xi), (hr, hi)), runs = fit(shape, [(xr, xi), (hr, hi)], dense(shape), [(0,), (1,)])     # copies: x, then h expanded
    return _P1.apply(xr, xi, hr, hi, (int(up), int(down), int(off), int(length), bool(conj), bool(out_imag), runs))


def wgrad(ar, ai, cr, ci, up, down, off, k, fshape, out_imag=True):
    """P2 on planes: a [*B, A], c [*B, C] -> (yr, yi) of [*fshape, k] (fshape broadcastable to B, as many dims): the
    rows that fshape broadcasts over are summed inside the kernel.  Differentiable to any order."""
    (ar, ai), (cr, ci), runs, f = fit_wgrad((ar, ai), (cr, ci), k, fshape)
    yr, yi = _P2.apply(ar, ai, cr, ci, (int(up), int(down), int(off), int(k), f, bool(out_imag), runs))
    if f == tuple(fshape):
        return yr, yi
    to = tuple(fshape) + (k,)                             # the broadcast pattern itself: per-row results, summed by torch
    return yr.sum_to_size(to), None if yi is None else yi.sum_to_size(to)


def _composed(xr, xi, hr, hi, up, down, off, length):
    """filters beyond the fused kernels: zero-stuffing, cplx.fftconvolve and a strided slice (not the hot path)"""
    from . import cplx
    from .cplx import Cplx
    n = xr.shape[-1]

    def stuff(p):
        if p is None or up == 1:
            return p
        return torch.nn.functional.pad(p.unsqueeze(-1), (0, up - 1)).flatten(-2)[..., :(n - 1) * up + 1]

    full = cplx.fftconvolve(stuff(xr) if xi is None else Cplx(stuff(xr), stuff(xi)), hr if hi is None else Cplx(hr, hi))

    def pick(p):
        short = off + (length - 1) * down + 1 - p.shape[-1]
        if short > 0:
            p = torch.nn.functional.pad(p, (0, short))
        return p[..., off::down][..., :length].contiguous()

    if torch.is_tensor(full):
        return pick(full), None
    return pick(full.real), pick(full.imag)


def _rate_change(fn, x, h, up, down, off, length_of):
    """the shared body of upfirdn and resample_poly: y[n] = sum_k h[k] xu[n down + off - k], n < length_of(N, K)"""
    from .cplx import Cplx
    (xr, xi), (hr, hi) = planes(x, "x", fn), planes(h, "h", fn)
    for t, name in ((xr, "x"), (hr, "h")):
        if t.dim() == 0:
            raise ValueError(f"{fn}: `{name}` is 0-d: there is no dim to filter along")
        if t.shape[-1] == 0:
            raise ValueError(f"{fn}: the last dim of `{name}` is empty")
    batch = tuple(torch.broadcast_shapes(xr.shape[:-1], hr.shape[:-1]))       # RuntimeError, as torch raises it
    if xr.dtype != hr.dtype:
        raise CplxAmdError(f"{fn}: the operands have different dtypes: {xr.dtype} and {hr.dtype}")
    code(xr.dtype)
    n, k = xr.shape[-1], hr.shape[-1]
    length = length_of(n, k)
    path = plan(n, k, length, up, down, off, 1, 1, xr.dtype, False, xi is not None, hi is not None)["path"]
    require_device(xr, xi, hr, hi)
    if path == "composed":
        yr, yi = _composed(xr, xi, hr, hi, up, down, off, length)
    else:
        lead = (None,) * (len(batch) - (hr.dim() - 1))
        expand = lambda t: None if t is None else t.expand(batch + (t.shape[-1],))
        yr, yi = conv(expand(xr), expand(xi), hr[lead], None if hi is None else hi[lead], up, down, off, length, False,
                      xi is not None or hi is not None)
    return yr if yi is None else Cplx(yr, yi)


def _rates(fn, up, down):
    if int(up) != up or int(down) != down or up < 1 or down < 1:
        raise ValueError(f"{fn}: up and down must be integers >= 1, got {up!r} and {down!r}")
    return int(up), int(down)


def upfirdn(h, x, up=1, down=1):
    """cplx.upfirdn (which documents it)"""
    up, down = _rates("upfirdn", up, down)
    return _rate_change("upfirdn", x, h, up, down, 0, lambda n, k: -(-((n - 1) * up + k) // down))


def design(up, down, beta=5.0, dtype=torch.float64, device="cpu"):
    """the default low-pass of resample_poly for the REDUCED rates: K = 20 max(up, down) + 1 taps of a Kaiser-windowed
    sinc with its cut-off at 1 / max(up, down) of Nyquist, scaled so that the taps sum to `up`; designed in float64 on
    the host, cached per (up, down, beta, dtype, device)"""
    return _design(int(up), int(down), float(beta), dtype, str(device))


@functools.lru_cache(maxsize=64)
def _design(up, down, beta, dtype, device):
    half = 10 * max(up, down)
    fc = 1.0 / max(up, down)
    n = torch.arange(-half, half + 1, dtype=torch.float64)
    h = fc * torch.sinc(fc * n) * torch.kaiser_window(2 * half + 1, periodic=False, beta=beta, dtype=torch.float64)
    return (h * (up / h.sum())).to(dtype).to(device)


def resample_poly(x, up, down, window=("kaiser", 5.0)):
    """cplx.resample_poly (which documents it)"""
    up, down = _rates("resample_poly", up, down)
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if torch.is_tensor(window):
        if window.dim() != 1 or window.is_complex():
            raise ValueError("resample_poly: a tensor `window` must be 1-d and real: the filter's taps")
        h = window * up                                   # as scipy scales the taps it is given
    elif isinstance(window, tuple) and len(window) == 2 and window[0] == "kaiser":
        h = None
    else:
        raise ValueError(f"resample_poly: window must be ('kaiser', beta) or a 1-d tensor of taps, got {window!r}")
    xr, xi = planes(x, "x", "resample_poly")
    if up == down:                                        # the input, as scipy returns a copy of it
        return xr.clone() if xi is None else type(x)(xr.clone(), xi.clone())
    if h is None:
        h = design(up, down, window[1], xr.dtype if xr.is_floating_point() else torch.float32, xr.device)
    half = (h.shape[-1] - 1) // 2
    return _rate_change("resample_poly", x, h, up, down, half, lambda n, k: -(-n * up // down))
