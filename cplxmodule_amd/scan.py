"""The first-order linear recurrence with a coefficient per step, along the last dim, on the time-parallel scan kernel of
csrc/scan.hip: the argument handling, the plan, the launch glue and the autograd Function behind cplx.linear_recurrence,
cplx.cumsum and cplx.cumprod.

One primitive (cplxamd_scan).  In processing order p = 0 .. T - 1 (step p is sample p, or sample T - 1 - p in reverse)

    h[p] = c[p] h[p - 1] + x[p],   h[-1] = h0 (or zero)

where c[p] is the coefficient of step p, conjugated under `conj`; under `lag` it is the coefficient of step p - 1 -- the
position the state comes from -- and step 0 has none.  With autograd's convention (dL/dre + i dL/dim), incoming gradient
g and lambda = the same primitive on (a, g) with all three flags flipped:

    dx = lambda,   da[p] = lambda[p] conj(h[p - 1])  (lag: da[p] = lambda[p + 1] conj(h[p])),   dh0 = conj(c[0]) lambda[0]

and da is conjugated once more under `conj`.  The products are torch arithmetic on shifted views of the planes: they
are differentiable, and lambda is the Function itself, so derivatives of every order stay on this kernel.  The products
and the `sum_to_size` that autograd applies where `a` or `h0` broadcast over rows are NOT the hot path.

A real operand is a null imaginary plane (never read); all-real operands run the one-plane instances.  Leading dims
broadcast by torch's rules and are read where they lie under _runs.py's rule of three batch runs, otherwise one
differentiable copy.  The result is dense in x's memory order; where that makes time strided (a [B, T, D] tensor seen
through .transpose(-1, -2)) the kernel's column plan puts the lanes along the dense run.  The workspace of the split path
comes from torch's allocator and nothing reads a device value on the host: calls can be captured in a hipGraph.
"""
import ctypes

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense_like, fill, fit, planes
from .iir import _cmul, _ct, _operands, _wrap

_FORCE_SEGMENTS = 0                                        # private: > 0 cuts every row into that many segments (tests, bench)
_FIELDS = ("a_stride", "x_stride", "h_stride", "y_stride")


def _plan(d, dtype, cx):
    out = (ctypes.c_int64 * len(_lib.SCAN_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_scan_plan(ctypes.byref(d), code(dtype), int(bool(cx)), out)
    if rc == -3:
        raise CplxAmdError(f"scan: rows of {d.n} steps exceed what the kernel indexes (2^40 steps, 2^31 - 1 workgroups)")
    if rc < 0:
        raise CplxAmdError(f"scan: no plan for this layout (error {rc})")
    p = dict(zip(_lib.SCAN_PLAN_FIELDS, out))
    p["lanes"] = _lib.SCAN_PLANS[rc]
    p["path"] = "split" if p["segments"] > 1 else p["lanes"]
    return p


def plan(T, rows=1, channels=None, dtype=torch.float32, cplx=True, force_segments=None):
    """The plan for `rows` rows of `T` steps -- a pure host call, no GPU needed.  `channels` None: dense [rows, T]
    operands; `channels` = D: a dense [rows, T, D] tensor seen through .transpose(-1, -2).  -> dict: `path` ("row",
    "column" or "split"), `lanes` ("row" / "column": what a lane holds, whatever the cut) and the fields of
    _lib.SCAN_PLAN_FIELDS -- chunk (the L steps a thread keeps in registers), tile, tiles, segments, seg_len, window
    (the consecutive coefficients whose product the kernel forms), units, LDS bytes, threads, grid, workspace bytes."""
    force = _FORCE_SEGMENTS if force_segments is None else force_segments
    D = 1 if channels is None else int(channels)
    d = _lib.ScanDesc(n=int(T), force_segments=int(force), a_es=D, x_es=D, y_es=D)
    rr = [[int(rows)] + [int(T) * D] * 4] * (rows != 1) + [[D, 1, 1, 1, 1]] * (D != 1)
    fill(d, rr, _FIELDS)
    return _plan(d, dtype, cplx)


def _fit(ar, ai, xr, xi, hr, hi):
    """a [*B, T] planes, x [*B, T] planes or (None, None), h0 [*B, 1] planes or (None, None) -> (the planes again, after
    the copies the kernel's layouts ask for; the result's strides; runs [size, a, x, h0, result])"""
    for copy in (False, True):
        if copy:                                          # time is strided and no dense run serves as lanes
            full = lambda t: None if t is None else t.expand(shape).contiguous()  # noqa: E731
            ar, ai, xr, xi = full(ar), full(ai), full(xr), full(xi)
        lead = ar if xr is None else xr
        shape = tuple(lead.shape)
        ys = dense_like(lead, -1, shape[-1])[1]
        named = [("a", (ar, ai))] + [("x", (xr, xi))] * (xr is not None) + [("h", (hr, hi))] * (hr is not None)
        ops, rr = fit(shape, [p for _, p in named], ys, [(k,) for k in sorted(range(len(named)), key=lambda k: named[k][0] != "x")])
        at = {name: k + 1 for k, (name, _) in enumerate(named)}
        got = dict(zip((name for name, _ in named), ops))
        (ar, ai), (xr, xi), (hr, hi) = got["a"], got.get("x", (None, None)), got.get("h", (None, None))
        # (a null x takes the result's strides, a null h0 zeros: neither is read)
        rr = [[r[0], r[at["a"]], r[at["x"]] if "x" in at else r[-1], r[at["h"]] if "h" in at else 0, r[-1]] for r in rr]
        column = bool(rr) and rr[-1][1] in (0, 1) and rr[-1][2] == 1 and rr[-1][4] == 1
        if shape[-1] == 1 or ys[-1] == 1 or column or copy:
            return (ar, ai), (xr, xi), (hr, hi), ys, rr


def run(ar, ai, xr, xi, hr, hi, reverse=False, conj=False, lag=False, cx=None, force_segments=None):
    """The module-level primitive, without autograd: a [*B, T] planes (views welcome, stride 0 along any dim), x [*B, T]
    planes or None (a null input), h0 [*B] planes or None -> (yr, yi) [*B, T] in the operands' dtype, dense in x's memory
    order.  ai, xi, hi may be None; yi is None when every operand is real (`cx` False)."""
    one = lambda t: None if t is None else t.unsqueeze(-1)    # noqa: E731
    (ar, ai), (xr, xi), (hr, hi), ys, rr = _fit(ar, ai, xr, xi, one(hr), one(hi))
    if cx is None:
        cx = any(t is not None for t in (ai, xi, hi))
    shape, dtype, dev = tuple(ar.shape), ar.dtype, ar.device
    T = shape[-1]
    yr = torch.empty_strided(shape, ys, dtype=dtype, device=dev)
    yi = torch.empty_like(yr) if cx else None
    es = lambda t: 1 if T == 1 else t.stride(-1)              # noqa: E731
    flags = (_lib.SCAN_REVERSE if reverse else 0) | (_lib.SCAN_CONJ if conj else 0) | (_lib.SCAN_LAG if lag else 0)
    d = _lib.ScanDesc(n=T, force_segments=_FORCE_SEGMENTS if force_segments is None else force_segments, a_es=es(ar),
                      x_es=es(yr if xr is None else xr), y_es=es(yr), flags=flags)
    fill(d, rr, _FIELDS)
    ws_bytes = _plan(d, dtype, cx)["ws_bytes"]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    call("cplxamd_scan", ptr(ar), ptr(ai) if cx else None, ptr(xr), ptr(xi) if cx else None, ptr(hr),
         ptr(hi) if cx else None, ptr(yr), ptr(yi), ctypes.byref(d), int(cx), code(dtype), ptr(ws), ws_bytes, stream_ptr())
    return yr, yi


def _cmulc(ar, ai, br, bi):
    """a conj(b) on (re, im | None) planes"""
    return _cmul(ar, ai, br, None if bi is None else -bi)


def _before(t, first, reverse):
    """t [*B, T] -> the plane whose entry at step p is t at step p - 1, and `first` [*B, 1] (None: zeros) at step 0"""
    if t is None:
        return None
    if first is None:
        first = torch.zeros_like(t[..., :1])
    return torch.cat([t[..., 1:], first], -1) if reverse else torch.cat([first, t[..., :-1]], -1)


class _Scan(torch.autograd.Function):
    """(yr, yi) = the recurrence of the module docstring over a (broadcastable to `shape` = [*B, T]), x [*B, T] (or None)
    from h0 (broadcastable to [*B], or None); ai, xi, hi may be None; yi is None unless `cx`.  meta = (reverse, conj, lag,
    cx, shape).  The gradients of a and h0 are formed per row in the compute type, reduced to the operand's shape with
    sum_to_size and rounded once: torch arithmetic, not the hot path."""

    @staticmethod
    def forward(ctx, ar, ai, xr, xi, hr, hi, meta):
        reverse, conj, lag, cx, shape = meta
        yr, yi = run(_over(ar, shape), _over(ai, shape), xr, xi, _over(hr, shape[:-1]), _over(hi, shape[:-1]), reverse, conj,
                     lag, cx)
        ctx.meta = meta
        ctx.save_for_backward(ar, ai, hr, hi, yr, yi)
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, hr, hi, yr, yi = ctx.saved_tensors
        reverse, conj, lag, cx, shape = ctx.meta
        need = ctx.needs_input_grad
        lr, li = recur(ar, ai, gr, gi if cx else None, None, None, not reverse, not conj, not lag, cx, shape)
        da = dh = (None, None)
        ct = lambda t: None if t is None else t.to(_ct(ar.dtype))     # noqa: E731
        back = lambda p, like: tuple(None if t is None else t.sum_to_size(like.shape).to(like.dtype) for t in p)  # noqa: E731
        if need[0] or need[1]:
            one = lambda t: None if t is None else ct(_over(t, shape[:-1])).unsqueeze(-1)     # noqa: E731
            if lag:
                da = _cmulc(_before(ct(lr), None, not reverse), _before(ct(li), None, not reverse), ct(yr), ct(yi))
            else:
                da = _cmulc(ct(lr), ct(li), _before(ct(yr), one(hr), reverse), _before(ct(yi), one(hi), reverse))
            da = back((da[0], -da[1]) if conj and da[1] is not None else da, ar)
        if need[4] or need[5]:
            at = -1 if reverse else 0
            first = lambda t: None if t is None else ct(t[..., at])   # noqa: E731
            dh = back((_cmul if conj else _cmulc)(first(lr), first(li), first(_over(ar, shape)), first(_over(ai, shape))), hr)
        pick = lambda t, k: t if need[k] else None        # noqa: E731
        return pick(da[0], 0), pick(da[1], 1), pick(lr, 2), pick(li, 3), pick(dh[0], 4), pick(dh[1], 5), None


def _over(t, shape):
    return None if t is None else t.expand(shape)


def recur(ar, ai, xr, xi, hr, hi, reverse=False, conj=False, lag=False, cx=None, shape=None):
    """The primitive on planes, differentiable to any order: x [*B, T] (views welcome) or None, a broadcastable to it
    (to `shape` when x is None), h0 broadcastable to [*B] or None -> (yr, yi), yi None when every operand is real."""
    if cx is None:
        cx = any(t is not None for t in (ai, xi, hi))
    shape = tuple(xr.shape if shape is None else shape)
    return _Scan.apply(ar, ai, xr, xi, hr, hi, (bool(reverse), bool(conj), bool(lag), bool(cx), shape))


def _recurrence(fn, a, x, h0, reverse):
    """the checks and the broadcast of the three public functions; x or h0 may be None"""
    ops = _operands(fn, (("a", a), ("x", x), ("h0", h0)), scalars=("h0",))
    (ar, ai), (xr, xi), (hr, hi) = ops["a"], ops["x"], ops["h0"]
    T = ar.shape[-1] if xr is None else xr.shape[-1]
    if ar.shape[-1] not in (1, T):
        raise ValueError(f"{fn}: the last dim of `a` must be 1 or {T}, that of `x`; got {ar.shape[-1]}")
    batch = tuple(torch.broadcast_shapes(*(t.shape[:-1] for t in (ar, xr) if t is not None)))  # RuntimeError, as torch raises it
    if hr is not None:
        try:
            fits = tuple(torch.broadcast_shapes(hr.shape, batch)) == batch
        except RuntimeError:
            fits = False
        if not fits:
            raise ValueError(f"{fn}: `h0` of shape {tuple(hr.shape)} does not broadcast to the batch shape {batch}")
    require_device(ar, ai, xr, xi, hr, hi)
    cx = any(t is not None for t in (ai, xi, hi))
    xr, xi = _over(xr, batch + (T,)), _over(xi, batch + (T,))
    if T == 0 or 0 in batch:                              # nothing to launch
        yr = torch.empty(batch + (T,), dtype=ar.dtype, device=ar.device)
        return _wrap(yr, torch.empty_like(yr) if cx else None)
    return _wrap(*recur(ar, ai, xr, xi, hr, hi, reverse, False, False, cx, batch + (T,)))


def linear_recurrence(a, x, h0=None, reverse=False):
    """cplx.linear_recurrence (which documents it)"""
    if x is None:
        raise CplxAmdError("linear_recurrence: `x` is a NoneType, not a Cplx or a real torch.Tensor")
    return _recurrence("linear_recurrence", a, x, h0, reverse)


def cumsum(x, reverse=False):
    """cplx.cumsum (which documents it): a = 1 through a stride-0 view of one element"""
    pr, _ = planes(x, "x", "cumsum")
    return _recurrence("cumsum", torch.ones(1, dtype=pr.dtype, device=pr.device), x, None, reverse)


def cumprod(a, reverse=False):
    """cplx.cumprod (which documents it): a null x and h0 = 1"""
    pr, _ = planes(a, "a", "cumprod")
    return _recurrence("cumprod", a, None, torch.ones((), dtype=pr.dtype, device=pr.device), reverse)
