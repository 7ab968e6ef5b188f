"""Linear convolution along the last dim on the fused overlap-save kernels of csrc/fftconv.hip: the argument handling,
the plan, the launch glue and the two autograd Functions behind cplx.fftconvolve.

The shorter operand (K entries) is the filter; convolution commutes, so `mode` is a (start, length) window of the full
result.  Two primitives, each an autograd Function whose backward calls the other's (a reads as zero outside its row):
    P1 `conv`    y[n] = sum_m a[n + start - m] b[m]          (conj: y[n] = sum_m a[n + start + m] conj(b[m])),  n < length
    P2 `wgrad`   y[m] = sum_rows sum_n conj(a[n]) c[n + m + start],  m < K      summed over the rows that share a result
With autograd's convention (dL/dre + i dL/dim) and incoming gradient g:
    P1 conv(a, b):  da = P1 corr(g, b; -start),  db = P2(a, g; -start)
    P1 corr(a, b):  da = P1 conv(g, b; -start),  db = P2(g, a; start)
    P2(a, c):       da = P1 corr(c, g; start),   dc = P1 conv(a, g; -start)
so derivatives of every order stay on the two kernels, and no gradient flips, conjugates or copies an operand in a pass of
its own: the conjugation is a flag (the block is multiplied by conj(H-hat)), the window is (start, length).  A real
operand is a null imaginary plane (never read, no zero plane allocated); the gradient of a real operand is the real part
(the null output plane is not stored).

Leading dims broadcast by torch's rules and are read where they lie: they are sorted by stride and fused into at most
three batch runs jointly for both operands and the result (_runs.py: `runs`, `fit`), so contiguous, step-sliced, `expand`ed
and transposed operands need no copy; an operand whose planes share no layout, or that needs more than three runs, is
copied once, differentiably.  The workspace (twiddles, filter spectra, partial spectra) comes from torch's allocator and
nothing reads a device value on the host: calls can be captured in a hipGraph.

Filters longer than 4096 taps take the COMPOSED path, which is not the hot path: cplx.fft of both operands at the next
power of two >= A + K - 1, the `Cplx` product, cplx.ifft and `narrow`, all differentiable launches of fft.py (float32
intermediates for bf16 planes); that length may not exceed 2^22.
"""
import ctypes

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense, fill, fit, fit_wgrad, planes
from .fft import MAX_N

MODES = ("full", "same", "valid")
PATHS = ("fused", "composed")                              # cplxamd_fftconv_plan's return codes
FUSED_MAX_K = 4096


def plan(a_len, k, start, length, rows=1, filters=1, dtype=torch.float32, conj=False, log_l=None):
    """The plan of both primitives for operands of `a_len` and `k` entries and the window (start, length) -- a pure host
    call, no GPU needed -> dict: path ("fused" / "composed"), L, and the fields of _lib.FFTCONV_PLAN_FIELDS (block
    stride S, blocks per row, blocks per workgroup, the block's offsets, workspace bytes; the same for the weight
    gradient with its chunks).  `log_l` forces L = 2^log_l >= k (measurements and exact tests)."""
    out = (ctypes.c_int64 * len(_lib.FFTCONV_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_fftconv_plan(int(a_len), int(k), int(start), int(length), int(rows), int(filters), code(dtype),
                                          int(bool(conj)), int(log_l or 0), out)
    if rc == -3 and k <= FUSED_MAX_K:
        raise CplxAmdError(f"fftconvolve: {rows} rows and {filters} filters of lengths {a_len} and {k} need more blocks or "
                           "workspace than the kernels index (2^31 - 1 blocks, 1 TiB of spectra)")
    if rc == -3:
        raise CplxAmdError(f"fftconvolve: a filter of {k} > {FUSED_MAX_K} taps is composed from transforms of "
                           f"2^ceil(log2({a_len} + {k} - 1)) points, which exceeds 2^22 = {MAX_N}, the longest supported")
    if rc < 0:
        raise CplxAmdError(f"fftconvolve: no plan for lengths {a_len} and {k}, window ({start}, {length}), log_l={log_l} "
                           "(lengths must be >= 1; log_l at most 13 with 2^log_l >= the filter's length)")
    p = dict(zip(_lib.FFTCONV_PLAN_FIELDS, out))
    p["path"], p["L"] = PATHS[rc], 1 << p["log_l"]
    return p


def window(n, m, mode):
    """(start, length) of `mode` in the full convolution of `input` (n entries) with `other` (m entries)"""
    if mode == "full":
        return 0, n + m - 1
    if mode == "same":
        return (m - 1) // 2, n
    return min(n, m) - 1, max(n, m) - min(n, m) + 1


def _launch(name, ar, ai, br, bi, yr, yi, runs, a_len, k, c_len, start, conj, log_l, ws_key):
    """one call of cplxamd_fftconv / _wgrad over the batch runs of (a, b, y); b is read with its broadcast strides"""
    d = _lib.FftConvDesc(a_len=a_len, k=k, c_len=c_len, start=start, a_es=ar.stride(-1), b_es=br.stride(-1), conj=int(conj),
                         log_l=int(log_l or 0), reserved=0)
    rows, filters = fill(d, runs, ("a_stride", "b_stride", "y_stride"), "y_stride" if ws_key == "wgrad_ws_bytes" else "b_stride")
    ws_bytes = plan(a_len, k, start, c_len, rows, filters, ar.dtype, conj, log_l)[ws_key]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ar.device)
    call(name, ptr(ar), ptr(ai), ptr(br), ptr(bi), ptr(yr), ptr(yi), ctypes.byref(d), code(ar.dtype), ptr(ws), ws_bytes,
         stream_ptr())


class _P1(torch.autograd.Function):
    """(yr, yi) = conv / corr of a [*B, A] with the filter b [*Bb, K] (Bb broadcastable to B, same number of dims) over
    the window (start, length); ai, bi may be None; yi is None unless `out_imag`."""

    @staticmethod
    def forward(ctx, ar, ai, br, bi, meta):
        start, length, conj, out_imag, log_l, runs = meta
        ctx.meta = meta[:5]
        ctx.save_for_backward(ar, ai, br, bi)
        yr = torch.empty(tuple(ar.shape[:-1]) + (length,), dtype=ar.dtype, device=ar.device)
        yi = torch.empty_like(yr) if out_imag else None
        if yr.numel():
            _launch("cplxamd_fftconv", ar, ai, br, bi, yr, yi, runs, ar.shape[-1], br.shape[-1], length, start, conj, log_l,
                    "ws_bytes")
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, br, bi = ctx.saved_tensors
        start, length, conj, out_imag, log_l = ctx.meta
        gi = gi if out_imag else None
        da = db = (None, None)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            da = conv(gr, gi, br, bi, -start, ar.shape[-1], not conj, ai is not None, log_l)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            first, second, s = ((gr, gi), (ar, ai), start) if conj else ((ar, ai), (gr, gi), -start)
            db = wgrad(*first, *second, s, br.shape[-1], tuple(br.shape[:-1]), bi is not None, log_l)
        return da[0], da[1], db[0], db[1], None


class _P2(torch.autograd.Function):
    """(yr, yi)[*F, m] = sum over the rows of B that F broadcasts over, and over n, of conj(a[n]) c[n + m + start], m < K,
    for a [*B, A] and c [*B, C]; F has B's number of dims.  ai, ci may be None; yi is None unless `out_imag`."""

    @staticmethod
    def forward(ctx, ar, ai, cr, ci, meta):
        start, k, fshape, out_imag, log_l, runs = meta
        ctx.meta = meta[:5]
        ctx.save_for_backward(ar, ai, cr, ci)
        yr = torch.empty(fshape + (k,), dtype=ar.dtype, device=ar.device)
        yi = torch.empty_like(yr) if out_imag else None
        if yr.numel() and ar.numel():
            _launch("cplxamd_fftconv_wgrad", ar, ai, cr, ci, yr, yi, runs, ar.shape[-1], k, cr.shape[-1], start, False, log_l,
                    "wgrad_ws_bytes")
        elif yr.numel():                                  # no rows to sum
            yr.zero_()
            if yi is not None:
                yi.zero_()
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, cr, ci = ctx.saved_tensors
        start, k, fshape, out_imag, log_l = ctx.meta
        gi = gi if out_imag else None
        da = dc = (None, None)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            da = conv(cr, ci, gr, gi, start, ar.shape[-1], True, ai is not None, log_l)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dc = conv(ar, ai, gr, gi, -start, cr.shape[-1], False, ci is not None, log_l)
        return da[0], da[1], dc[0], dc[1], None


def conv(ar, ai, br, bi, start, length, conj=False, out_imag=True, log_l=None):
    """P1 on planes: a [*B, A] (views welcome), filter b [*Bb, K] with Bb broadcastable to B and as many dims -> (yr, yi)
    of [*B, length], yi None unless `out_imag`.  Differentiable to any order."""
    shape = tuple(ar.shape[:-1]) + (length,)
    ((ar, ai), (br, bi)), runs = fit(shape, [(ar, ai), (br, bi)], dense(shape), [(0,), (1,)])     # copies: a, then b expanded
    return _P1.apply(ar, ai, br, bi, (int(start), int(length), bool(conj), bool(out_imag), log_l, runs))


def wgrad(ar, ai, cr, ci, start, k, fshape, out_imag=True, log_l=None):
    """P2 on planes: a [*B, A], c [*B, C] -> (yr, yi) of [*fshape, k] (fshape broadcastable to B, as many dims): the
    rows that fshape broadcasts over are summed inside the kernel.  Differentiable to any order."""
    (ar, ai), (cr, ci), runs, f = fit_wgrad((ar, ai), (cr, ci), k, fshape)
    yr, yi = _P2.apply(ar, ai, cr, ci, (int(start), int(k), f, bool(out_imag), log_l, runs))
    if f == tuple(fshape):
        return yr, yi
    to = tuple(fshape) + (k,)                             # the broadcast pattern itself: per-row results, summed by torch
    return yr.sum_to_size(to), None if yi is None else yi.sum_to_size(to)


def _composed(ar, ai, br, bi, start, length, dtype):
    """filters beyond the fused kernels: the differentiable launches of fft.py (not the hot path)"""
    from . import cplx
    from .cplx import Cplx
    n = 1 << (ar.shape[-1] + br.shape[-1] - 2).bit_length()
    wide = torch.float32 if dtype == torch.bfloat16 else dtype

    def lift(pr, pi):
        pr = pr.to(wide)
        return Cplx(pr, torch.zeros_like(pr) if pi is None else pi.to(wide))

    y = cplx.ifft(cplx.fft(lift(ar, ai), n) * cplx.fft(lift(br, bi), n))
    yr = y.real.narrow(-1, start, length).to(dtype).contiguous()
    if ai is None and bi is None:
        return yr, None
    return yr, y.imag.narrow(-1, start, length).to(dtype).contiguous()


def fftconvolve(input, other, mode="full", log_l=None):
    """cplx.fftconvolve (which documents it), plus `log_l`: force blocks of 2^log_l >= min(N, M) points."""
    from .cplx import Cplx
    if mode not in MODES:
        raise ValueError(f"fftconvolve: mode must be one of {MODES}, got {mode!r}")
    (xr, xi), (hr, hi) = planes(input, "input", "fftconvolve"), planes(other, "other", "fftconvolve")
    for t, name in ((xr, "input"), (hr, "other")):
        if t.dim() == 0:
            raise ValueError(f"fftconvolve: `{name}` is 0-d: there is no dim to convolve along")
        if t.shape[-1] == 0:
            raise ValueError(f"fftconvolve: the last dim of `{name}` is empty")
    batch = tuple(torch.broadcast_shapes(xr.shape[:-1], hr.shape[:-1]))       # RuntimeError, as torch raises it
    if xr.dtype != hr.dtype:
        raise CplxAmdError(f"fftconvolve: the operands have different dtypes: {xr.dtype} and {hr.dtype}")
    code(xr.dtype)
    n, m = xr.shape[-1], hr.shape[-1]
    start, length = window(n, m, mode)
    (ar, ai), (br, bi) = ((xr, xi), (hr, hi)) if n >= m else ((hr, hi), (xr, xi))
    path = plan(ar.shape[-1], br.shape[-1], start, length, 1, 1, xr.dtype, False, log_l)["path"]
    require_device(ar, ai, br, bi)
    if path == "composed":
        yr, yi = _composed(ar, ai, br, bi, start, length, xr.dtype)
    else:
        lead = (None,) * (len(batch) - (br.dim() - 1))
        expand = lambda t: None if t is None else t.expand(batch + (t.shape[-1],))
        yr, yi = conv(expand(ar), expand(ai), br[lead], None if bi is None else bi[lead], start, length, False,
                      ai is not None or bi is not None, log_l)
    return yr if yi is None else Cplx(yr, yi)
