"""Scaled dot-product attention of planar `Cplx` tensors on the fused flash kernel (csrc/attention.hip): the argument
checks, the layout fit, the launch glue and the autograd Function behind cplx.scaled_dot_product_attention.

With c = q k^H (the Hermitian product) per batch entry,

    s = scale Re c   (score="real")    or    s = scale |c|   (score="abs"),
    p = softmax over the keys of s  (real),       o = p v  (complex),

`scale` defaulting to 1 / sqrt(E).  The forward is ONE launch that never holds s or p in memory; it writes o and one
float32 log-sum-exp per (batch, query), from which the backward kernels recompute p.  The leading dims are batch: they
are fused, jointly for every tensor of the call, into at most three runs (_runs.py), so a `[B, L, H, E]` projection
viewed as `[B, H, L, E]` is read in place and the result, whose memory order follows the query's, is a free view of
`[B, L, H, Ev]`.  An operand whose last dim has a stride other than 1, or a call that needs more than three runs, costs
one differentiable copy.  float64 planes take the composed route (`@`, torch softmax): parity mode.

Nothing reads a device value on the host: calls can be captured in a hipGraph.  The backward is not differentiable.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import MAX_RUNS, dense_like, fill, runs, share
from .ops import once_differentiable

SCORES = ("real", "abs")
MAX_HEAD = 128
FN = "scaled_dot_product_attention"


def plan(L, S, E, Ev, batch=1, dtype=torch.float32):
    """cplxamd_attn_plan as a dict (q_tile, k_tile, head, q_tiles, grid, lds_bytes, ws_bytes) -- a pure host call."""
    out = (ctypes.c_int64 * len(_lib.ATTN_PLAN_FIELDS))()
    rc = _lib.load().cplxamd_attn_plan(int(L), int(S), int(E), int(Ev), int(batch),
                                       {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}.get(dtype, -1), out)
    if rc != 0:
        raise CplxAmdError(f"{FN}: no plan for L = {L}, S = {S}, E = {E}, Ev = {Ev}, batch = {batch} (error {rc})")
    return dict(zip(_lib.ATTN_PLAN_FIELDS, out))


def _desc(q, k, v, o, lse, grads, flags, scale):
    """the descriptor of a call on planes q, k, v, o (and dq, dk, dv), or None when the batch needs too many runs"""
    batch = tuple(q.shape[:-2])
    tensors = [q, k, v, o] + [lse] + list(grads)
    strides = [t.stride()[:len(batch)] + (1,) for t in tensors]
    rr = runs(batch + (1,), strides)
    if len(rr) > MAX_RUNS:
        return None, 0
    d = _lib.AttnDesc(L=q.shape[-2], S=k.shape[-2], E=q.shape[-1], Ev=v.shape[-1], flags=flags, scale=scale,
                      q_rs=q.stride(-2), k_rs=k.stride(-2), v_rs=v.stride(-2), o_rs=o.stride(-2))
    fields = ["q_stride", "k_stride", "v_stride", "o_stride", "lse_stride"]
    if grads:
        d.dq_rs, d.dk_rs, d.dv_rs = (t.stride(-2) for t in grads)
        fields += ["dq_stride", "dk_stride", "dv_stride"]
    rows, _ = fill(d, rr, fields)
    return d, rows


def _same_layout(a, b):
    """equal strides wherever a dim has more than one entry"""
    return all(x == y for n, x, y in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _row_stride_ok(t):
    return t.stride(-1) == 1 or t.shape[-1] == 1


class _Attention(torch.autograd.Function):
    """(o_r, o_i) of planes whose last dims have stride 1; `meta` = (flags, scale)."""

    @staticmethod
    def forward(ctx, qr, qi, kr, ki, vr, vi, meta):
        flags, scale = meta
        shape, ostr = dense_like(qr, qr.dim() - 1, vr.shape[-1])
        o_r = torch.empty_strided(shape, ostr, dtype=qr.dtype, device=qr.device)
        o_i = torch.empty_like(o_r)
        lse = torch.empty(shape[:-1], dtype=torch.float32, device=qr.device)
        d, rows = _desc(qr, kr, vr, o_r, lse, (), flags, scale)
        if d is None:                                     # (more than three runs: dense operands always fit)
            qr, qi, kr, ki, vr, vi = (t.contiguous() for t in (qr, qi, kr, ki, vr, vi))
            o_r = torch.empty(shape, dtype=qr.dtype, device=qr.device)
            o_i = torch.empty_like(o_r)
            d, rows = _desc(qr, kr, vr, o_r, lse, (), flags, scale)
        if rows:
            call("cplxamd_attn_fwd", ptr(qr), ptr(qi), ptr(kr), ptr(ki), ptr(vr), ptr(vi), ptr(o_r), ptr(o_i), ptr(lse),
                 ctypes.byref(d), _lib.dtype_code(qr), stream_ptr())
        ctx.save_for_backward(qr, qi, kr, ki, vr, vi, o_r, o_i, lse)
        ctx.meta = meta
        return o_r, o_i

    @staticmethod
    @once_differentiable
    def backward(ctx, gr, gi):
        qr, qi, kr, ki, vr, vi, o_r, o_i, lse = ctx.saved_tensors
        flags, scale = ctx.meta
        need_q, need_kv = any(ctx.needs_input_grad[:2]), any(ctx.needs_input_grad[2:6])
        if not (need_q or need_kv):
            return (None,) * 7
        # the upstream gradient in o's layout (one layout per tensor: the planes share strides)
        gr, gi = (g if _same_layout(g, o_r) else torch.empty_like(o_r).copy_(g) for g in (gr, gi))
        dense = lambda t, need: [torch.empty_like(t, memory_format=torch.contiguous_format) if need else None  # noqa: E731
                                 for _ in range(2)]
        dq, dk, dv = dense(qr, need_q), dense(kr, need_kv), dense(vr, need_kv)
        # (a gradient that is not asked for is not computed: its kernel is not launched; its strides repeat the operand's)
        grads = (dq[0] if need_q else qr, dk[0] if need_kv else kr, dv[0] if need_kv else vr)
        d, rows = _desc(qr, kr, vr, o_r, lse, grads, flags, scale)
        if d is None:                                     # dense copies: one run
            qr, qi, kr, ki, vr, vi, o_r, o_i, gr, gi = (t.contiguous() for t in (qr, qi, kr, ki, vr, vi, o_r, o_i, gr, gi))
            grads = (dq[0] if need_q else qr, dk[0] if need_kv else kr, dv[0] if need_kv else vr)
            d, rows = _desc(qr, kr, vr, o_r, lse, grads, flags, scale)
        if rows:
            ws_bytes = 4 * rows * qr.shape[-2]
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qr.device)
            call("cplxamd_attn_bwd", ptr(qr), ptr(qi), ptr(kr), ptr(ki), ptr(vr), ptr(vi), ptr(o_r), ptr(o_i), ptr(gr),
                 ptr(gi), ptr(lse), ptr(dq[0]), ptr(dq[1]), ptr(dk[0]), ptr(dk[1]), ptr(dv[0]), ptr(dv[1]),
                 ctypes.byref(d), _lib.dtype_code(qr), ptr(ws), ws_bytes, stream_ptr())
        return dq[0], dq[1], dk[0], dk[1], dv[0], dv[1], None


def _composed(q, k, v, causal, scale, score):
    """the float64 route: `@` on the float64 contraction path and torch's softmax"""
    from .cplx import Cplx
    c = q @ Cplx(k.real.transpose(-1, -2), -k.imag.transpose(-1, -2))
    s = (c.real if score == "real" else abs(c)) * scale
    if causal:
        L, S = s.shape[-2:]
        s = s.masked_fill(torch.ones(L, S, dtype=torch.bool, device=s.device).triu(1), -math.inf)
    p = torch.softmax(s, -1)
    return Cplx(p @ v.real, p @ v.imag)


def _checked(x, name):
    from .cplx import Cplx
    if not isinstance(x, Cplx):
        kind = "a torch tensor of complex dtype" if torch.is_tensor(x) and x.is_complex() else f"a {type(x).__name__}"
        raise CplxAmdError(f"{FN}: `{name}` is {kind}, not a Cplx (wrap planes with Cplx(re, im))")
    re, im = x.real, x.imag
    if re.dtype != im.dtype or re.device != im.device:
        raise CplxAmdError(f"{FN}: the planes of `{name}` differ: {re.dtype} on {re.device} and {im.dtype} on {im.device}")
    if re.dim() < 2:
        raise ValueError(f"{FN}: `{name}` has {re.dim()} dims; attention needs [..., rows, features]")
    return re, im


def scaled_dot_product_attention(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, score="real"):
    from .cplx import Cplx
    if score not in SCORES:
        raise ValueError(f"{FN}: unknown score {score!r}; one of {SCORES}")
    if attn_mask is not None:
        raise CplxAmdError(f"{FN}: `attn_mask` is not offered yet (only `is_causal`); pass attn_mask=None")
    if dropout_p != 0:
        raise CplxAmdError(f"{FN}: dropout inside the kernel is not offered; pass dropout_p=0 and apply CplxDropout outside")
    (qr, qi), (kr, ki), (vr, vi) = _checked(query, "query"), _checked(key, "key"), _checked(value, "value")
    if qr.shape[-1] != kr.shape[-1]:
        raise ValueError(f"{FN}: query has E = {qr.shape[-1]}, key has E = {kr.shape[-1]}")
    if kr.shape[-2] != vr.shape[-2]:
        raise ValueError(f"{FN}: key has S = {kr.shape[-2]}, value has S = {vr.shape[-2]}")
    if not (qr.shape[:-2] == kr.shape[:-2] == vr.shape[:-2]):
        raise CplxAmdError(f"{FN}: the leading dims differ: {tuple(qr.shape[:-2])}, {tuple(kr.shape[:-2])}, "
                           f"{tuple(vr.shape[:-2])} (no broadcasting, no grouped heads)")
    if not (qr.dtype == kr.dtype == vr.dtype):
        raise CplxAmdError(f"{FN}: query, key and value have different dtypes: {qr.dtype}, {kr.dtype}, {vr.dtype}")
    if qr.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise CplxAmdError(f"{FN}: planes must be float32, bfloat16 or float64, got {qr.dtype}")
    L, E, S, Ev = qr.shape[-2], qr.shape[-1], kr.shape[-2], vr.shape[-1]
    if min(L, S, E, Ev) < 1:
        raise ValueError(f"{FN}: L, S, E and Ev must be at least 1, got {L}, {S}, {E}, {Ev}")
    if max(E, Ev) > MAX_HEAD:
        raise CplxAmdError(f"{FN}: head sizes above {MAX_HEAD} are not offered, got E = {E}, Ev = {Ev}")
    require_device(qr, qi, kr, ki, vr, vi)
    scale = 1.0 / math.sqrt(E) if scale is None else float(scale)
    if qr.dtype == torch.float64:
        return _composed(query, key, value, bool(is_causal), scale, score)
    planes = []
    for re, im in ((qr, qi), (kr, ki), (vr, vi)):
        re, im = share(re, im)
        if not _row_stride_ok(re):
            re, im = re.contiguous(), im.contiguous()
        planes += [re, im]
    flags = (_lib.ATTN_CAUSAL if is_causal else 0) | (_lib.ATTN_ABS if score == "abs" else 0)
    return Cplx(*_Attention.apply(*planes, (flags, scale)))
