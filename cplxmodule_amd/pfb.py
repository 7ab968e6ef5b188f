"""The polyphase filter bank along the last dim on the kernels of csrc/pfb.hip: the argument handling, the plan, the
launch glue and the two autograd Functions behind cplx.pfb_analysis and cplx.pfb_synthesis.

M channels (a power of two), K = P M real taps, a frame every `hop` samples, the phase referred to the start of the frame:

    analysis    y[f, k] = sum_{n < K} h[n] x[f hop + n] e^{-2 pi i k n / M} = FFT_M(u[f])[k],
                u[f, r] = sum_{p < P} h[p M + r] x[f hop + p M + r]
    synthesis   out[t] = sum_f g[t - f hop] sum_k y[f, k] e^{+2 pi i k (t - f hop) / M},   0 <= t - f hop < K

With autograd's convention (dL/dre + i dL/dim) each is the other's adjoint for the same taps, so each Function's backward
is the other Function and derivatives of every order in the signal stay on the kernels.  The taps are fixed designs: they
get no gradient.  A real signal is a null imaginary plane (never read, no zero plane allocated), and its gradient is the
real plane of the synthesis (the imaginary one is neither summed nor stored).

Leading dims are batch and are read where they lie under _runs.py's rule of three batch runs, otherwise one copy.  The
synthesis workspace comes from torch's allocator and nothing reads a device value on the host: calls can be captured in
a hipGraph.  float64 is not taken: `cplx.stft(x, n_fft=K, hop_length=hop, window=h, center=False)[..., ::P, :]` is the
parity route.
"""
import ctypes

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import MAX_RUNS, code, dense, fill, fit, planes, runs, share

MAX_CHANNELS, MAX_TAPS = 4096, 64


def _geometry(fn, M, K, hop):
    """the checks of (n_channels, taps, hop) -> (M, P, hop)"""
    if int(M) != M or M < 2 or M > MAX_CHANNELS or int(M) & (int(M) - 1):
        raise ValueError(f"{fn}: the number of channels must be a power of two in 2 .. {MAX_CHANNELS}, got {M!r}")
    M = int(M)
    if K < M or K % M or K // M > MAX_TAPS:
        raise ValueError(f"{fn}: the taps must be P * {M} with 1 <= P <= {MAX_TAPS}, got {K}")
    hop = M if hop is None else hop
    if int(hop) != hop or hop < 1 or hop > K:
        raise ValueError(f"{fn}: hop must be an integer in 1 .. {K} (the taps), got {hop!r}")
    return M, K // M, int(hop)


def _plan(d, cx):
    out = (ctypes.c_int64 * len(_lib.PFB_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_pfb_plan(ctypes.byref(d), int(bool(cx)), out)
    if rc == -3:
        raise CplxAmdError(f"pfb: {d.frames} frames of {d.channels} channels exceed what the kernels index "
                           "(2^31 - 1 workgroups)")
    if rc < 0:
        raise CplxAmdError(f"pfb: no plan for {d.channels} channels, {d.taps} taps per channel, hop {d.hop} (error {rc})")
    p = dict(zip(_lib.PFB_PLAN_FIELDS, out))
    p["plan"] = _lib.PFB_PLANS[rc]
    return p


def plan(n_channels, taps_per_channel, hop=None, frames=1, rows=1, cplx=True):
    """The plan of the analysis for `rows` rows of `frames` frames -- a pure host call, no GPU needed -> dict: `plan`
    ("staged": the tile's samples go through LDS once; "direct": they are read from global memory, P loads per point) and
    the fields of _lib.PFB_PLAN_FIELDS -- frames per tile (what one workgroup owns), tiles per row, frames transformed
    at a time (> 1: packed), the staged span in samples, LDS bytes, threads, grid, and the synthesis workspace bytes.
    `cplx`: two signal planes, or one."""
    M, P, hop = _geometry("pfb.plan", n_channels, int(n_channels) * int(taps_per_channel), hop)
    d = _lib.PfbDesc(channels=M, taps=P, hop=hop, frames=int(frames))
    fill(d, [[int(rows), 0, 0]] * (rows != 1), ("sig_stride", "spec_stride"))
    return _plan(d, cplx)


def _run_analysis(xr, xi, h, M, hop, F):
    """planes x [*B, T] (views welcome; xi may be None) -> (yr, yi) [*B, F, M], dense, in x's dtype; no autograd"""
    batch, T = tuple(xr.shape[:-1]), xr.shape[-1]
    yr = torch.empty(batch + (F, M), dtype=xr.dtype, device=xr.device)
    yi = torch.empty_like(yr)
    if yr.numel():
        ((xr, xi),), rr = fit(batch + (T,), [(xr, xi)], dense(batch + (F * M,)), [(0,)])
        d = _lib.PfbDesc(channels=M, taps=h.shape[0] // M, hop=hop, frames=F, length=T, sig_es=xr.stride(-1))
        fill(d, rr, ("sig_stride", "spec_stride"))
        call("cplxamd_pfb_analysis", ptr(xr), ptr(xi), ptr(h), ptr(yr), ptr(yi), ctypes.byref(d), code(xr.dtype),
             stream_ptr())
    return yr, yi


def _run_synthesis(yr, yi, g, hop, length, out_imag):
    """planes y [*B, F, M] (views welcome) -> (outr, outi) [*B, length], dense; outi None unless `out_imag`; no autograd"""
    batch, (F, M) = tuple(yr.shape[:-2]), yr.shape[-2:]
    outr = torch.empty(batch + (length,), dtype=yr.dtype, device=yr.device)
    outi = torch.empty_like(outr) if out_imag else None
    if outr.numel():
        yr, yi = share(yr, yi)
        rows = batch + (1,)
        for last in (False, True):
            rr = runs(rows, (tuple(yr.stride()[:-2]) + (1,), dense(rows)))
            if last or len(rr) <= MAX_RUNS:
                break
            yr, yi = yr.contiguous(), yi.contiguous()
        d = _lib.PfbDesc(channels=M, taps=g.shape[0] // M, hop=hop, frames=F, length=length, spec_fs=yr.stride(-2),
                         spec_es=yr.stride(-1))
        fill(d, rr, ("spec_stride", "sig_stride"))
        ws_bytes = _plan(d, out_imag)["ws_bytes"]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=yr.device)
        call("cplxamd_pfb_synthesis", ptr(yr), ptr(yi), ptr(g), ptr(outr), ptr(outi), ctypes.byref(d), code(yr.dtype),
             ptr(ws), ws_bytes, stream_ptr())
    return outr, outi


class _Analysis(torch.autograd.Function):
    """(yr, yi) [*B, F, M] = the analysis bank of x [*B, T] with the taps h [K]; xi may be None.  meta = (M, hop, F)."""

    @staticmethod
    def forward(ctx, xr, xi, h, meta):
        ctx.meta = meta + (xr.shape[-1], xi is not None)
        ctx.save_for_backward(h)
        return _run_analysis(xr, xi, h, *meta)

    @staticmethod
    def backward(ctx, gr, gi):
        (h,) = ctx.saved_tensors
        M, hop, F, T, cx = ctx.meta
        dr, di = synthesis(gr, gi, h, hop, T, cx)
        return dr, di, None, None


class _Synthesis(torch.autograd.Function):
    """(outr, outi) [*B, length] = the synthesis bank of y [*B, F, M] with the taps g [K]; outi is None unless out_imag.
    meta = (hop, length, out_imag)."""

    @staticmethod
    def forward(ctx, yr, yi, g, meta):
        ctx.meta = meta + tuple(yr.shape[-2:])
        ctx.save_for_backward(g)
        return _run_synthesis(yr, yi, g, *meta)

    @staticmethod
    def backward(ctx, gr, gi):
        (g,) = ctx.saved_tensors
        hop, length, out_imag, F, M = ctx.meta
        dr, di = analysis(gr, gi if out_imag else None, g, M, hop, F)
        return dr, di, None, None


def analysis(xr, xi, h, M, hop, F):
    """the analysis on planes, differentiable to any order in x: x [*B, T] with T >= (F - 1) hop + K -> (yr, yi)"""
    return _Analysis.apply(xr, xi, h, (int(M), int(hop), int(F)))


def synthesis(yr, yi, g, hop, length, out_imag=True):
    """the synthesis on planes, differentiable to any order in y: y [*B, F, M] -> (outr, outi) [*B, length]"""
    return _Synthesis.apply(yr, yi, g, (int(hop), int(length), bool(out_imag)))


def _taps(fn, h, name):
    """the taps as they are given: a real 1-d tensor without a gradient"""
    from .cplx import Cplx
    if isinstance(h, Cplx) or not torch.is_tensor(h) or h.is_complex():
        raise CplxAmdError(f"{fn}: `{name}` must be a real torch.Tensor of taps (Cplx and complex taps are not taken), "
                           f"got a {type(h).__name__}")
    if h.requires_grad:
        raise CplxAmdError(f"{fn}: `{name}` requires grad, but the taps are a fixed design and get no gradient: "
                           "detach them")
    if h.dtype not in (torch.float32, torch.bfloat16):
        raise CplxAmdError(f"{fn}: `{name}` must be float32 (or bfloat16, widened once), got {h.dtype}")
    if h.dim() != 1:
        raise ValueError(f"{fn}: `{name}` must be 1-d, got shape {tuple(h.shape)}")
    return h


def _signal(fn, x, name):
    pr, pi = planes(x, name, fn)
    if pi is not None and pr.device != pi.device:
        raise CplxAmdError(f"{fn}: the planes of `{name}` are on different devices: {pr.device} and {pi.device}")
    if pr.dtype not in (torch.float32, torch.bfloat16):
        raise CplxAmdError(f"{fn}: `{name}` must be float32 or bfloat16, got {pr.dtype} (float64: compose cplx.stft and "
                           "a slice)")
    return pr, pi


def pfb_analysis(x, h, n_channels, hop=None):
    """cplx.pfb_analysis (which documents it)"""
    from .cplx import Cplx
    fn = "pfb_analysis"
    xr, xi = _signal(fn, x, "x")
    h = _taps(fn, h, "h")
    if xr.dim() == 0:
        raise ValueError(f"{fn}: `x` is 0-d: there is no dim to filter along")
    M, P, hop = _geometry(fn, n_channels, h.shape[0], hop)
    T, K = xr.shape[-1], P * M
    if T < K:
        raise ValueError(f"{fn}: the last dim of `x` has {T} samples, fewer than the {K} taps (there is no padding)")
    require_device(xr, xi, h)
    return Cplx(*analysis(xr, xi, h.float().contiguous(), M, hop, (T - K) // hop + 1))


def pfb_synthesis(y, g, hop=None, length=None):
    """cplx.pfb_synthesis (which documents it)"""
    from .cplx import Cplx
    fn = "pfb_synthesis"
    yr, yi = _signal(fn, y, "y")
    if yi is None:
        raise CplxAmdError(f"{fn}: `y` is a real tensor, not the Cplx [..., frames, channels] of an analysis")
    g = _taps(fn, g, "g")
    if yr.dim() < 2:
        raise ValueError(f"{fn}: `y` must be [..., frames, channels], got shape {tuple(yr.shape)}")
    F = yr.shape[-2]
    M, P, hop = _geometry(fn, yr.shape[-1], g.shape[0], hop)
    if F < 1:
        raise ValueError(f"{fn}: `y` has no frames")
    least = (F - 1) * hop + P * M
    length = least if length is None else length
    if int(length) != length or length < least:
        raise ValueError(f"{fn}: length must be an integer >= (frames - 1) * hop + taps = {least}, got {length!r}")
    require_device(yr, yi, g)
    return Cplx(*synthesis(yr, yi, g.float().contiguous(), hop, int(length), True))
