"""Structured compaction of the masked layers ("use the masks"; DESIGN.md "Masked layers on compacted
operands").

A mask whose rows (output features) or columns (input features) are entirely zero describes a SMALLER dense layer.  The
opt-in route of nn/masked.py (`compact_`) finds the live rows / columns on the device, gathers the activations and the
masked weight down to them, runs the existing dense Functions (mask=None) on the compacted operands and expands the
result:

    x' = gather(x, cols)          W' = (W * mask)[rows][:, cols]          y' = dense(x', W', b[rows])
    y  = expand(y', rows; dead features get the bias)

Gather and expand are linear and each other's adjoint, so the backward pass is the same composition mirrored, second
derivatives of the linear layers keep working, and every choice the dense Functions make (fp32_mode, split products,
Gauss 3M, channels-last) applies as it does to a dense layer of the smaller size.  Unstructured sparsity is NOT
attempted: see DESIGN.md.

Kernels: csrc/compact.hip (cplxamd_live_index, _gather_axis, _expand_axis, _compact_weight, _expand_weight).
"""
import math

import torch

from . import _lib, ops
from ._lib import CplxAmdError, call, dtype_code, ptr, require_device, stream_ptr

# The fast kernels decline odd shapes: the 3M / persistent GEMM entries want K % 32 == 0 and N % 4 == 0 (ops.gauss_ok),
# the channels-last convolutions Ci % 64 == 0 and Co % 64 == 0 (conv._cl_ok, conv._cl_wgrad_ok).  A non-empty live list is
# therefore padded to a multiple of 64 with dead indices (their weight rows / columns are zero: results are unchanged).
GRANULE = 64

# The compacted route is taken when the padded product O' I' is at most this fraction of O I (and strictly smaller).
# Measured (profiles/masked_compact_bench.txt, scripts/masked_compact_bench.py): the largest O' I' / (O I) on the grid at
# which the compacted step beats the dense one in both cases -- 0.5625 (0.75 live per side): 0.969 of the dense step for
# CplxLinearMasked 4096^2 at batch 8192, 0.932 for CplxConv2dMasked 256 -> 256 on 64 x 64 images, against a spread of the
# dense timings repeated in the same run of at most 1.1 %.  One run on one box: at this fraction the margin is small.
MAX_LIVE_FRACTION = 0.5625


def pad_live(live, total, granule=GRANULE):
    """The index list the plan keeps for a live set: `live` (any iterable of distinct indices < total) plus the
    lowest-numbered dead indices up to min(total, next multiple of `granule`), ascending.  Empty stays empty.  Pure host
    function; cplxamd_live_index computes the same list on the device."""
    live = sorted(set(int(i) for i in live))
    if not live:
        return []
    if live[0] < 0 or live[-1] >= total:
        raise ValueError("live index out of range")
    want = min(int(total), -(-len(live) // granule) * granule)
    have = set(live)
    out = list(live)
    i = 0
    while len(out) < want:
        if i not in have:
            out.append(i)
        i += 1
    return sorted(out)


# ------------------------------------------------------------------------------------------ #
#  raw kernels                                                                               #
# ------------------------------------------------------------------------------------------ #
def _mask3(mask):
    """float32 [O, C, T] view of a weight-shaped mask (T = 1 for a linear weight)."""
    if mask.dim() < 2:
        raise CplxAmdError("compaction needs a mask of at least two dimensions")
    mask = ops._f32(mask.contiguous())
    O, C = mask.shape[0], mask.shape[1]
    return mask.reshape(O, C, -1)


def live_index(mask, granule=1):
    """-> (rows[O], cols[C], inv_rows[O], inv_cols[C], counts[4]) int32 device tensors; counts = live rows, listed rows,
    live columns, listed columns (only the listed prefix of rows / cols is defined).  No host synchronisation."""
    require_device(mask)
    m = _mask3(mask)
    O, C, T = m.shape
    if min(O, C, T) < 1:
        raise CplxAmdError("compaction: empty mask")
    dev = m.device
    rows, inv_rows = torch.empty(O, dtype=torch.int32, device=dev), torch.empty(O, dtype=torch.int32, device=dev)
    cols, inv_cols = torch.empty(C, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.load().cplxamd_live_index_ws_bytes(O, C)), dtype=torch.uint8, device=dev)
    call("cplxamd_live_index", ptr(m), O, C, T, int(granule), ptr(rows), ptr(cols), ptr(inv_rows), ptr(inv_cols), ptr(counts),
         ptr(ws), ws.numel(), stream_ptr())
    return rows, cols, inv_rows, inv_cols, counts


def _axis_view(t, dim):
    """(tensor in a dense layout, channels-last?, (outer, axis, inner) of its storage) for an access along `dim`."""
    dim %= t.dim()
    if t.dim() == 4 and dim == 1 and ops._layout_of(t) is torch.channels_last:
        B, C, H, W = t.shape
        return t, True, (B * H * W, C, 1)
    t = t.contiguous()
    s = t.shape
    return t, False, (math.prod(s[:dim]), s[dim], math.prod(s[dim + 1:]))


def _alloc(like, dim, n, cl):
    shape = list(like.shape)
    shape[dim % like.dim()] = n
    return torch.empty(shape, dtype=like.dtype, device=like.device,
                       memory_format=torch.channels_last if cl else torch.contiguous_format)


def gather(tr, ti, idx, dim):
    """(tr, ti).index_select(dim, idx) in one launch (ti may be None); a channels-last tensor stays channels-last."""
    require_device(tr, ti, idx)
    tr, cl, (outer, axis, inner) = _axis_view(tr, dim)
    if ti is not None:
        ti = ops._cf(ti, torch.channels_last if cl else torch.contiguous_format)
    n = idx.numel()
    our = _alloc(tr, dim, n, cl)
    oui = None if ti is None else torch.empty_like(our)
    call("cplxamd_gather_axis", ptr(tr), ptr(ti), ptr(idx), ptr(our), ptr(oui), outer, axis, n, inner, dtype_code(tr),
         stream_ptr())
    return our, oui


def expand(tr, ti, inv, dim, fill=(None, None)):
    """The adjoint of `gather` as one pass over the full output: out[.., a, ..] = t[.., inv[a], ..] where inv[a] >= 0,
    else fill[a] (float32 [len(inv)] per plane; None: 0)."""
    require_device(tr, ti, inv, *fill)
    tr, cl, (outer, n, inner) = _axis_view(tr, dim)
    if ti is not None:
        ti = ops._cf(ti, torch.channels_last if cl else torch.contiguous_format)
    axis = inv.numel()
    fr, fi = (None if f is None else ops._f32(f.contiguous()) for f in fill)
    our = _alloc(tr, dim, axis, cl)
    oui = None if ti is None else torch.empty_like(our)
    call("cplxamd_expand_axis", ptr(tr), ptr(ti), ptr(inv), ptr(fr), ptr(fi), ptr(our), ptr(oui), outer, n, axis, inner,
         dtype_code(tr), stream_ptr())
    return our, oui


def compact_weight(wr, wi, mask, rows, cols, out_dtype=None):
    """((wr * mask)[rows][:, cols], same for wi) in one pass, converted to `out_dtype`: the compacted ops.mask_mul."""
    require_device(wr, wi, mask, rows, cols)
    wr, wi, m = ops._c(wr), ops._c(wi), _mask3(mask.expand_as(wr))
    O, C, T = m.shape
    R, Cn = rows.numel(), cols.numel()
    odt = out_dtype or wr.dtype
    our = torch.empty((R, Cn) + tuple(wr.shape[2:]), dtype=odt, device=wr.device)
    oui = None if wi is None else torch.empty_like(our)
    call("cplxamd_compact_weight", ptr(wr), ptr(wi), ptr(m), ptr(rows), ptr(cols), ptr(our), ptr(oui), O, C, T, R, Cn,
         dtype_code(wr), dtype_code(our), stream_ptr())
    return our, oui


def expand_weight(sr, si, mask, inv_rows, inv_cols, out_dtype=None):
    """The adjoint of `compact_weight`: a weight-shaped tensor with src * mask at the listed rows and columns and an exact
    zero everywhere else."""
    require_device(sr, si, mask, inv_rows, inv_cols)
    sr, si = ops._c(sr), ops._c(si)
    m = _mask3(mask)
    O, C, T = m.shape
    R, Cn = sr.shape[0], sr.shape[1]
    odt = out_dtype or sr.dtype
    our = torch.empty(mask.shape, dtype=odt, device=sr.device)
    oui = None if si is None else torch.empty_like(our)
    call("cplxamd_expand_weight", ptr(sr), ptr(si), ptr(m), ptr(inv_rows), ptr(inv_cols), ptr(our), ptr(oui), O, C, T, R, Cn,
         dtype_code(sr), dtype_code(our), stream_ptr())
    return our, oui


# ------------------------------------------------------------------------------------------ #
#  the plan                                                                                  #
# ------------------------------------------------------------------------------------------ #
class Plan:
    """Index lists of one mask.  rows / cols: ascending int32 lists of the kept output / input features (the live ones
    and the granule padding); inv_rows / inv_cols: position in the list or -1; n_rows / n_cols = (live, padded, total)."""

    __slots__ = ("key", "mask", "rows", "cols", "inv_rows", "inv_cols", "n_rows", "n_cols")

    @property
    def empty(self):
        return self.n_rows[1] == 0 or self.n_cols[1] == 0

    def fraction(self):
        return (self.n_rows[1] * self.n_cols[1]) / float(self.n_rows[2] * self.n_cols[2])

    def active(self, max_live=None):
        """The route is taken when the padded product is strictly smaller than the full one and within `max_live`."""
        frac = self.fraction()
        return frac < 1.0 and frac <= (MAX_LIVE_FRACTION if max_live is None else float(max_live))

    def report(self, active):
        return dict(rows=self.n_rows, cols=self.n_cols, active=bool(active))


def _key(mask):
    return (mask.data_ptr(), mask._version, tuple(mask.shape))


def build_plan(mask):
    """One launch group + ONE host synchronisation (the two list lengths).  A host-resident mask (a module inspected
    before it is moved to the GPU) gets the counts only."""
    p = Plan()
    p.key, p.mask = _key(mask), mask           # (the reference keeps the address from being reused while the plan lives)
    O, C = mask.shape[0], mask.shape[1]
    if not mask.is_cuda:
        live = mask.detach().reshape(O, C, -1).ne(0)
        lr, lc = int(live.any(2).any(1).sum()), int(live.any(2).any(0).sum())
        pr, pc = (min(t, -(-n // GRANULE) * GRANULE) if n else 0 for n, t in ((lr, O), (lc, C)))
        p.rows = p.cols = p.inv_rows = p.inv_cols = None
    else:
        rows, cols, p.inv_rows, p.inv_cols, counts = live_index(mask, GRANULE)
        lr, pr, lc, pc = counts.tolist()
        p.rows, p.cols = rows[:pr], cols[:pc]
    p.n_rows, p.n_cols = (lr, pr, O), (lc, pc, C)
    return p


def plan_of(layer):
    """The cached plan of a masked layer, rebuilt when the mask was replaced or edited in place."""
    mask = layer._require_mask()
    plan = layer.__dict__.get("_compact_plan")
    if plan is None or plan.key != _key(mask):
        if mask.is_cuda and torch.cuda.is_current_stream_capturing():
            raise CplxAmdError(f"`{type(layer).__name__}`: the compaction plan of this mask is stale and cannot be rebuilt "
                               "while the stream is capturing (it reads two counts back to the host): run the layer once "
                               "eagerly first (GraphedStep's warm-up does)")
        plan = build_plan(mask)
        object.__setattr__(layer, "_compact_plan", plan)
    return plan


def _planes(w):
    return (w,) if isinstance(w, torch.Tensor) else (w.real, w.imag)


def _dense_reason(layer):
    """Why a layer with a compact route runs dense anyway (None: nothing in the way)."""
    if getattr(layer, "groups", 1) != 1:
        return "groups"
    planes = _planes(layer.weight)
    if planes[0].dtype not in (torch.float32, torch.bfloat16) or layer.mask.dtype != torch.float32:
        return "dtype"
    if any(ops.hook_of(p) is not None for p in planes):
        return "data-parallel hook"
    return None


def route(layer, x):
    """The plan to run `layer` on compacted operands for the input plane `x`, or None for the dense route."""
    if not layer.compact or layer._compact_kind is None or not layer.is_sparse:
        return None
    if x.dtype not in (torch.float32, torch.bfloat16) or _dense_reason(layer) is not None:
        return None
    plan = plan_of(layer)
    return plan if plan.active(layer.compact_max_live) else None


def report(layer):
    """`compaction()` entry of one masked layer."""
    if layer._compact_kind is None or not layer.is_sparse:
        return None
    plan = plan_of(layer)
    return plan.report(layer.compact and _dense_reason(layer) is None and plan.active(layer.compact_max_live))


# ------------------------------------------------------------------------------------------ #
#  autograd                                                                                  #
# ------------------------------------------------------------------------------------------ #
def _pair_out(r, i, cplx):
    return (r, i) if cplx else r


class GatherFn(torch.autograd.Function):
    """gather along `dim`; backward = ExpandFn (zero fill).  Linear, differentiable to any order."""

    @staticmethod
    def forward(ctx, tr, ti, idx, inv, dim):
        ctx.idx, ctx.inv, ctx.dim, ctx.cplx = idx, inv, dim, ti is not None
        return _pair_out(*gather(tr, ti, idx, dim), ctx.cplx)

    @staticmethod
    def backward(ctx, gr, gi=None):
        out = ExpandFn.apply(gr, gi if ctx.cplx else None, ctx.inv, ctx.idx, ctx.dim, None, None)
        dr, di = out if ctx.cplx else (out, None)
        return dr, di, None, None, None


def _bias_sums(gr, gi, dim):
    """Per-feature sums of the output gradient over every other dimension -> float32: the kernels the dense routes use."""
    if torch.is_grad_enabled():                       # create_graph=True: differentiable torch ops, as ops.CplxLinearFn does
        dims = [d for d in range(gr.dim()) if d != dim % gr.dim()]
        return tuple(None if g is None else g.float().sum(dims) for g in (gr, gi))
    if gr.dim() == 4 and dim % 4 == 1:
        from . import conv
        if ops._layout_of(gr) is torch.channels_last:
            B, C, H, W = gr.shape
            rows = lambda t: t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(B * H * W, C)  # noqa: E731
            return ops.colsum(rows(gr)), (None if gi is None else ops.colsum(rows(gi)))
        gr = gr.contiguous()
        return conv.chansum2(gr, gi.contiguous()) if gi is not None else (conv.chansum(gr), None)
    O = gr.shape[-1]
    g2r = gr.reshape(-1, O).contiguous()
    if gi is None:
        return ops.colsum(g2r), None
    return ops.colsum2(g2r, gi.reshape(-1, O).contiguous())


class ExpandFn(torch.autograd.Function):
    """expand along `dim` (the adjoint of GatherFn); backward = GatherFn.  `br` / `bi`: the layer's bias, which the
    source ALREADY carries at its listed positions (the dense kernel added bias[rows]) and which is written as it is at
    every other position -- so y depends on every bias entry with weight one and its gradient is the plain sum of the
    output gradient over all other dimensions, dead features included: what the dense route gives."""

    @staticmethod
    def forward(ctx, tr, ti, inv, idx, dim, br, bi):
        ctx.idx, ctx.inv, ctx.dim, ctx.cplx = idx, inv, dim, ti is not None
        ctx.bias_dtypes = tuple(None if b is None else b.dtype for b in (br, bi))
        return _pair_out(*expand(tr, ti, inv, dim, (br, bi)), ctx.cplx)

    @staticmethod
    def backward(ctx, gr, gi=None):
        gi = gi if ctx.cplx else None
        out = GatherFn.apply(gr, gi, ctx.idx, ctx.inv, ctx.dim)
        dr, di = out if ctx.cplx else (out, None)
        dbr = dbi = None
        if ctx.needs_input_grad[5] or ctx.needs_input_grad[6]:
            dbr, dbi = _bias_sums(gr, gi, ctx.dim)
            dbr = None if dbr is None else dbr.to(ctx.bias_dtypes[0])
            dbi = None if dbi is None or ctx.bias_dtypes[1] is None else dbi.to(ctx.bias_dtypes[1])
        return dr, di, None, None, None, dbr, dbi


class CompactWeightFn(torch.autograd.Function):
    """W' = (W * mask)[rows][:, cols]; backward = ExpandWeightFn, so every masked entry of dW is an exact zero."""

    @staticmethod
    def forward(ctx, wr, wi, mask, plan, out_dtype):
        ctx.plan, ctx.cplx, ctx.wdtype = plan, wi is not None, wr.dtype
        ctx.save_for_backward(mask)
        return _pair_out(*compact_weight(wr, wi, mask, plan.rows, plan.cols, out_dtype), ctx.cplx)

    @staticmethod
    def backward(ctx, gr, gi=None):
        (mask,) = ctx.saved_tensors
        out = ExpandWeightFn.apply(gr, gi if ctx.cplx else None, mask, ctx.plan, ctx.wdtype)
        dr, di = out if ctx.cplx else (out, None)
        return dr, di, None, None, None


class ExpandWeightFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sr, si, mask, plan, out_dtype):
        ctx.plan, ctx.cplx, ctx.sdtype = plan, si is not None, sr.dtype
        ctx.save_for_backward(mask)
        return _pair_out(*expand_weight(sr, si, mask, plan.inv_rows, plan.inv_cols, out_dtype), ctx.cplx)

    @staticmethod
    def backward(ctx, gr, gi=None):
        (mask,) = ctx.saved_tensors
        out = CompactWeightFn.apply(gr, gi if ctx.cplx else None, mask, ctx.plan, ctx.sdtype)
        dr, di = out if ctx.cplx else (out, None)
        return dr, di, None, None, None


class _NoLiveFn(torch.autograd.Function):
    """The all-zero mask: the compacted layer has no features at all.  Stands in for the dense Function on the empty
    operands (no launch): empty outputs, and exact-zero (empty) gradients that keep x and W connected to the graph."""

    @staticmethod
    def forward(ctx, shape, n_out, *tensors):
        ctx.shapes = [(t.shape, t.dtype) for t in tensors]
        outs = tuple(tensors[0].new_empty(shape) for _ in range(n_out))
        return outs if n_out > 1 else outs[0]

    @staticmethod
    def backward(ctx, *grads):
        dev = grads[0].device
        return (None, None) + tuple(torch.zeros(s, dtype=d, device=dev) for s, d in ctx.shapes)


def _weight_dtype(w, x):
    """The compacted weight comes out in the activation dtype (one pass, like ops.mask_mul) -- unless its gradient is
    wanted: then it keeps the weight's dtype and the dense Function converts it, so that dW' arrives in float32 instead
    of being rounded to the activation dtype on its way back."""
    return w.dtype if (torch.is_grad_enabled() and w.requires_grad) else x.dtype


def _bias_planes(b):
    if b is None:
        return None, None
    return (b.real, b.imag) if not isinstance(b, torch.Tensor) else (b, None)


def _gathered_bias(br, bi, plan):
    """bias[rows] for the dense kernel's epilogue (float32, no history: ExpandFn owns the bias gradient)."""
    if br is None:
        return None, None
    with torch.no_grad():
        return gather(ops._f32(br.detach()), None if bi is None else ops._f32(bi.detach()), plan.rows, 0)


def linear(layer, input, plan):
    """{Cplx,}LinearMasked.forward on compacted operands."""
    from .cplx import Cplx
    w, mask = layer.weight, layer.mask
    cplx = not isinstance(w, torch.Tensor)
    xr, xi = (input.real, input.imag) if cplx else (input, None)
    wr, wi = (w.real, w.imag) if cplx else (w, None)
    br, bi = _bias_planes(layer.bias)
    x = GatherFn.apply(xr, xi, plan.cols, plan.inv_cols, -1)
    wc = CompactWeightFn.apply(wr, wi, mask, plan, _weight_dtype(wr, xr))
    if plan.empty:
        y = _NoLiveFn.apply(tuple(xr.shape[:-1]) + (0,), 2 if cplx else 1, *(x + wc if cplx else (x, wc)))
    else:
        bcr, bci = _gathered_bias(br, bi, plan)
        if cplx:
            y = ops.CplxLinearFn.apply(x[0], x[1], wc[0], wc[1], bcr, bci, 0, None)
        else:
            y = ops.RealLinearFn.apply(x, wc, bcr, None)
    yr, yi = y if cplx else (y, None)
    out = ExpandFn.apply(yr, yi, plan.inv_rows, plan.rows, -1, br, bi)
    return Cplx(*out) if cplx else out


def conv2d(layer, input, plan):
    """{Cplx,}Conv2dMasked.forward on compacted operands (groups == 1)."""
    from . import conv
    from .cplx import Cplx
    w, mask = layer.weight, layer.mask
    cplx = not isinstance(w, torch.Tensor)
    if not cplx and layer.padding_mode != "zeros":
        raise ValueError("Conv2dMasked supports `zeros` padding only")
    xr, xi = (input.real, input.imag) if cplx else (input, None)
    wr, wi = (w.real, w.imag) if cplx else (w, None)
    br, bi = _bias_planes(layer.bias)
    x = GatherFn.apply(xr, xi, plan.cols, plan.inv_cols, 1)
    wc = CompactWeightFn.apply(wr, wi, mask, plan, _weight_dtype(wr, xr))
    if plan.empty:
        shape, padding = list(xr.shape), conv.ntuple(layer.padding, 2)
        if layer.padding_mode == "circular":
            # cplx_conv2d pads, then convolves unpadded; conv._circular_pad hands `padding` to F.pad, which starts at the
            # LAST dimension: padding[0] widens W and padding[1] widens H (the reference's order)
            shape[2], shape[3], padding = shape[2] + padding[1], shape[3] + padding[0], 0
        oshape = conv._geom(shape, wr.shape, layer.stride, padding, layer.dilation, 1)[1]
        y = _NoLiveFn.apply((oshape[0], 0) + tuple(oshape[2:]), 2 if cplx else 1, *(x + wc if cplx else (x, wc)))
    else:
        bcr, bci = _gathered_bias(br, bi, plan)
        if cplx:
            yc = conv.cplx_conv2d(Cplx(*x), Cplx(*wc), None if bcr is None else Cplx(bcr, bci), layer.stride, layer.padding,
                                  layer.dilation, 1, layer.padding_mode)
            y = (yc.real, yc.imag)
        else:
            y = conv.RealConv2dFn.apply(x, wc, bcr, layer.stride, layer.padding, layer.dilation, 1)
    yr, yi = y if cplx else (y, None)
    out = ExpandFn.apply(yr, yi, plan.inv_rows, plan.rows, 1, br, bi)
    return Cplx(*out) if cplx else out
