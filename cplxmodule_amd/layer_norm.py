"""Layer normalisation of planar `Cplx` tensors on the fused per-row kernel (csrc/layer_norm.hip): the argument checks,
the layout fit, the launch glue and the autograd Function behind cplx.layer_norm.

A row is the last `len(normalized_shape)` dims, flattened to N complex features.  With m = mean x and c = x - m,

    whiten:   a = mean c_r^2 + eps, d = mean c_i^2 + eps, b = mean c_r c_i, s = sqrt(a d - b^2), t = s sqrt(a + d + 2 s),
              y_r = (d + s) / t c_r - b / t c_i,   y_i = -b / t c_r + (a + s) / t c_i
    modulus:  y = c / sqrt(mean |c|^2 + eps)

and out = W y + B per feature (`weight` [2, 2, *normalized_shape], `bias` [2, *normalized_shape], float32).  The forward
is ONE launch that reads and writes every plane value once and saves five (three) float32 per row; the backward is one
launch of persistent workgroups and one finishing launch, without atomics.  The normalised dims must be jointly dense
with last stride 1, else the operand costs one differentiable copy; the leading dims are fused into at most three runs
(_runs.py), so a transposed or sliced batch is read in place, and the result is dense in the input's memory order.
float64 planes take the composed route: parity mode.

Nothing reads a device value on the host: calls can be captured in a hipGraph.  The backward is not differentiable.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import MAX_RUNS, dense, dense_like, fill, runs, share
from .ops import once_differentiable

KINDS = _lib.LN_KINDS
FN = "layer_norm"
_CODES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def plan(rows, N, kind="whiten", dtype=torch.float32):
    """cplxamd_ln_plan as a dict (_lib.LN_PLAN_FIELDS; `plan` and `bwd_plan` as "wave", "block" or "stream") -- a pure
    host call.  The seams between the plans are `seam_wave`, `seam_block` and, for the backward, `bwd_seam_block`."""
    out = (ctypes.c_int64 * len(_lib.LN_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_ln_plan(int(rows), int(N), KINDS.index(kind), _CODES.get(dtype, -1), out)
    if rc != 0:
        raise CplxAmdError(f"{FN}: no plan for rows = {rows}, N = {N}, kind = {kind!r}, {dtype} (error {rc})")
    p = dict(zip(_lib.LN_PLAN_FIELDS, out))
    p["plan"], p["bwd_plan"] = _lib.LN_PLANS[p["plan"]], _lib.LN_PLANS[p["bwd_plan"]]
    return p


def _fit(xr, xi, nd):
    """planes with dense normalised dims -> (xr, xi, the result's strides, descriptor runs over [x, result, result])"""
    ns, nb = tuple(xr.shape[-nd:]), xr.dim() - nd
    for last in (False, True):
        if last:
            xr, xi = xr.contiguous(), xi.contiguous()
        ostr = dense_like(xr, xr.dim() - 1, xr.shape[-1])[1]
        if not last and any(s != w for n, s, w in zip(ns, ostr[-nd:], dense(ns)) if n > 1):
            continue                                     # (a leading dim inside the row, as an expanded one: copy)
        strides = [tuple(t[:nb]) + (1,) for t in (xr.stride(), ostr, ostr)]
        rr = runs(tuple(xr.shape[:nb]) + (1,), strides)
        if last or len(rr) <= MAX_RUNS:
            return xr, xi, ostr, rr


def _desc(rr, N, kind, eps):
    d = _lib.LnDesc(N=N, kind=kind, eps=eps)
    rows, _ = fill(d, rr, ["x_stride", "o_stride", "g_stride"])
    return d, rows


class _LayerNorm(torch.autograd.Function):
    """(out_r, out_i) of planes whose normalised dims are dense; `meta` = (number of normalised dims, eps, kind code)."""

    @staticmethod
    def forward(ctx, xr, xi, weight, bias, meta):
        nd, eps, kind = meta
        N = math.prod(xr.shape[-nd:])
        xr, xi, ostr, rr = _fit(xr, xi, nd)
        d, rows = _desc(rr, N, kind, eps)
        o_r = torch.empty_strided(xr.shape, ostr, dtype=xr.dtype, device=xr.device)
        o_i = torch.empty_like(o_r)
        stats = torch.empty(rows, 3 if kind else 5, dtype=torch.float32, device=xr.device)
        if rows:
            call("cplxamd_ln_fwd", ptr(xr), ptr(xi), ptr(weight), ptr(bias), ptr(o_r), ptr(o_i), ptr(stats),
                 ctypes.byref(d), _lib.dtype_code(xr), stream_ptr())
        ctx.save_for_backward(xr, xi, weight, stats)
        ctx.meta, ctx.fit, ctx.has_bias = meta, (ostr, rr, N, rows), bias is not None
        return o_r, o_i

    @staticmethod
    @once_differentiable
    def backward(ctx, gr, gi):
        xr, xi, weight, stats = ctx.saved_tensors
        (nd, eps, kind), (ostr, rr, N, rows) = ctx.meta, ctx.fit
        need_x = any(ctx.needs_input_grad[:2])
        need_p = weight is not None and any(ctx.needs_input_grad[2:4])
        if not (need_x or need_p):
            return (None,) * 5
        # the upstream gradient in the result's layout (dx has it too: one set of runs serves x, dx and g)
        same = lambda g: all(s == w for n, s, w in zip(g.shape, g.stride(), ostr) if n > 1)  # noqa: E731
        gr, gi = (g if same(g) else torch.empty_strided(xr.shape, ostr, dtype=xr.dtype, device=xr.device).copy_(g)
                  for g in (gr, gi))
        dx = [torch.empty_strided(xr.shape, ostr, dtype=xr.dtype, device=xr.device) if need_x else None for _ in range(2)]
        # (a gradient that is not asked for is not computed: dx is not written, the partials and their launch are skipped)
        dwb = torch.empty(6, N, dtype=torch.float32, device=xr.device) if need_p else None
        if rows:
            d, _ = _desc(rr, N, kind, eps)
            ws_bytes = plan(rows, N, KINDS[kind], xr.dtype)["ws_bytes"] if need_p else 0
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xr.device) if need_p else None
            call("cplxamd_ln_bwd", ptr(xr), ptr(xi), ptr(gr), ptr(gi), ptr(weight), ptr(stats), ptr(dx[0]), ptr(dx[1]),
                 ptr(dwb), None if dwb is None else ctypes.c_void_p(dwb.data_ptr() + 16 * N), ctypes.byref(d),
                 _lib.dtype_code(xr), ptr(ws), ws_bytes, stream_ptr())
        elif need_p:
            dwb.zero_()
        dw = dwb[:4].view(weight.shape) if need_p else None
        db = dwb[4:].view(weight.shape[1:]) if need_p and ctx.has_bias else None
        return dx[0], dx[1], dw, db, None


def _composed(xr, xi, nd, weight, bias, eps, kind):
    """the float64 route: the formulas of the module docstring in torch ops"""
    dims = tuple(range(-nd, 0))
    cr, ci = xr - xr.mean(dims, keepdim=True), xi - xi.mean(dims, keepdim=True)
    if kind == "modulus":
        rstd = torch.rsqrt((cr * cr + ci * ci).mean(dims, keepdim=True) + eps)
        yr, yi = cr * rstd, ci * rstd
    else:
        a, d = (cr * cr).mean(dims, keepdim=True) + eps, (ci * ci).mean(dims, keepdim=True) + eps
        b = (cr * ci).mean(dims, keepdim=True)
        s = torch.sqrt(a * d - b * b)
        t = s * torch.sqrt(a + d + 2 * s)
        yr, yi = ((d + s) * cr - b * ci) / t, ((a + s) * ci - b * cr) / t
    if weight is None:
        return yr, yi
    w = weight.to(xr.dtype)
    b0, b1 = (0, 0) if bias is None else bias.to(xr.dtype)
    return w[0, 0] * yr + w[0, 1] * yi + b0, w[1, 0] * yr + w[1, 1] * yi + b1


def layer_norm(input, normalized_shape, weight=None, bias=None, eps=1e-5, kind="whiten"):
    from .cplx import Cplx
    if kind not in KINDS:
        raise ValueError(f"{FN}: unknown kind {kind!r}; one of {KINDS}")
    if not isinstance(input, Cplx):
        what = "a torch tensor of complex dtype" if torch.is_tensor(input) and input.is_complex() else f"a {type(input).__name__}"
        raise CplxAmdError(f"{FN}: `input` is {what}, not a Cplx (wrap planes with Cplx(re, im))")
    xr, xi = input.real, input.imag
    if xr.dtype != xi.dtype or xr.device != xi.device:
        raise CplxAmdError(f"{FN}: the planes of `input` differ: {xr.dtype} on {xr.device} and {xi.dtype} on {xi.device}")
    ns = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    nd = len(ns)
    if nd < 1 or nd > xr.dim() or tuple(xr.shape[-nd:]) != ns:
        raise ValueError(f"{FN}: normalized_shape = {ns} does not match the trailing dims of an input of shape {tuple(xr.shape)}")
    if math.prod(ns) < 1:
        raise ValueError(f"{FN}: a row must hold at least one feature, got normalized_shape = {ns}")
    if bias is not None and weight is None:
        raise ValueError(f"{FN}: a bias needs a weight (pass both or neither)")
    if weight is not None and tuple(weight.shape) != (2, 2) + ns:
        raise ValueError(f"{FN}: weight has shape {tuple(weight.shape)}, expected {(2, 2) + ns}")
    if bias is not None and tuple(bias.shape) != (2,) + ns:
        raise ValueError(f"{FN}: bias has shape {tuple(bias.shape)}, expected {(2,) + ns}")
    if xr.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise CplxAmdError(f"{FN}: planes must be float32, bfloat16 or float64, got {xr.dtype}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0):
        raise ValueError(f"{FN}: eps must be finite and not negative, got {eps}")
    require_device(xr, xi, weight, bias)
    if xr.dtype == torch.float64:
        return Cplx(*_composed(xr, xi, nd, weight, bias, eps, kind))
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and t.dtype != torch.float32:
            raise CplxAmdError(f"{FN}: `{name}` must be float32 for every activation dtype, got {t.dtype}")
    xr, xi = share(xr, xi)
    if any(s != w for n, s, w in zip(ns, xr.stride()[-nd:], dense(ns)) if n > 1):
        xr, xi = xr.contiguous(), xi.contiguous()         # (one differentiable copy: the row must be dense)
    weight, bias = (None if t is None else t.contiguous() for t in (weight, bias))
    return Cplx(*_LayerNorm.apply(xr, xi, weight, bias, (nd, eps, KINDS.index(kind))))
