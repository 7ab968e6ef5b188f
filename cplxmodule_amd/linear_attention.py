"""Linear attention with a per-step complex decay -- retention, gated linear attention, the matrix-state recurrence -- on
the chunked MFMA kernel of csrc/linattn.hip: the argument checks, the plan, the launch glue and the autograd Function
behind cplx.linear_attention, and the composed route (`composed`: the quadratic masked form in torch products) that
float64 takes and scripts/bench_linear_attention.py compares against.

One primitive (cplxamd_linattn).  In processing order p = 0 .. T - 1 (step p is row p, or T - 1 - p in reverse), with S
an E x Ev complex matrix per batch entry:

    S[p] = exp(lambda[p]) S[p - 1] + k[p]^H (x) v[p],   o[p] = scale q[p] S[p],   S[-1] = state (or zero)

Four flags: `reverse`; `conj` conjugates lambda; `lag` takes the lambda of step p - 1, and the state enters step 0
unscaled; `scale_in` moves `scale` from the output to the update.  With autograd's convention (dL/dre + i dL/dim), g
the gradient of o and gS that of the returned state, every data gradient is the same kernel with the roles swapped:

    dq = run(g, v, k, S0^H; conj)                                     head dims (Ev, E)
    dk = run(v, g, q, gS^H; reverse flipped, lag, scale_in)           head dims (Ev, E)
    dv = run(k, q, g, gS;   reverse flipped, lag, conj, scale_in)
    dS0 = conj(exp lambda[first]) (the final state of the dv call)
    dlambda[r] = sum_{t >= r} U[t] - sum_{s >= r} conj(W[s]) + <S_T, gS>,   U = sum_e conj(q) dq,  W = sum_e conj(k) dk

(`decay_gradient`: two row sums, one running sum and an E x Ev product, in torch: not the hot path).  A gradient that is
not asked for is not launched.  The backward is not differentiable: higher derivatives are `composed`'s.

The leading dims of q, k, v are equal and are read where they lie under _runs.py's rule of three batch runs (a
[B, T, H, E] projection viewed as [B, H, T, E] costs no copy; the result follows the query's memory order); a last dim
with a stride other than 1, or a call that needs more runs, costs one copy.  lambda travels as dense float32 planes
[*B, T], the states as float32 planes whatever the dtype.  Nothing reads a device value on the host.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import MAX_RUNS, dense_like, fill, planes, runs, share
from .attention import MAX_HEAD
from .ops import once_differentiable

FN = "linear_attention"


def plan(T, E, Ev, batch=1, dtype=torch.float32):
    """cplxamd_linattn_plan as a dict of _lib.LINATTN_PLAN_FIELDS (chunk, head_e, head_v, slice, slices, chunks, grid,
    lds_bytes, threads) -- a pure host call, no GPU needed."""
    out = (ctypes.c_int64 * len(_lib.LINATTN_PLAN_FIELDS))()
    kind = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}.get(dtype, -1)
    rc = _lib.load().cplxamd_linattn_plan(int(T), int(E), int(Ev), int(batch), kind, out)
    if rc != 0:
        raise CplxAmdError(f"{FN}: no plan for T = {T}, E = {E}, Ev = {Ev} (1 .. {MAX_HEAD}), batch = {batch} in {dtype} "
                           f"(float32 or bfloat16; error {rc})")
    return dict(zip(_lib.LINATTN_PLAN_FIELDS, out))


def _rows(p):
    """a plane pair whose last dim the kernel can step along (stride 1), in one layout"""
    pr, pi = share(*p)
    if pr.stride(-1) != 1:
        pr, pi = pr.contiguous(), pi.contiguous()
    return pr, pi


def run(q, k, v, lam, state, scale, reverse=False, conj=False, lag=False, scale_in=False, want_state=True):
    """The module-level primitive, without autograd, on plane pairs: q, k [*B, T, E], v [*B, T, Ev] (float32 or bfloat16;
    views welcome), lam = (re, im or None) float32 [*B, T] or None, state = (re, im) float32 [*B, E, Ev] or None
    -> (o_r, o_i, f_r, f_i): o [*B, T, Ev] in the operands' dtype and the query's memory order, and the final state
    [*B, E, Ev] in float32, not rounded (None without `want_state`)."""
    (qr, qi), (kr, ki), (vr, vi) = _rows(q), _rows(k), _rows(v)
    batch, T, E, Ev, dev = tuple(qr.shape[:-2]), qr.shape[-2], qr.shape[-1], vr.shape[-1], qr.device
    lr = li = sr = si = None
    if lam is not None:
        lr, li = (None if t is None else t.expand(batch + (T,)) for t in lam)
        if li is not None and li.stride() != lr.stride():
            lr, li = lr.contiguous(), li.contiguous()
        if lr.stride(-1) != 1 and T != 1:
            lr, li = lr.contiguous(), None if li is None else li.contiguous()
    if state is not None:
        sr, si = (t if t.stride(-1) == 1 or Ev == 1 else t.contiguous() for t in share(*state))
    for dense in (False, True):
        if dense:                                         # (more than three runs: dense operands always fit)
            qr, qi, kr, ki, vr, vi = (t.contiguous() for t in (qr, qi, kr, ki, vr, vi))
            if lam is not None:
                lr, li = lr.contiguous(), None if li is None else li.contiguous()
            if state is not None:
                sr, si = sr.contiguous(), si.contiguous()
        shape, ostr = dense_like(qr, qr.dim() - 1, Ev)
        o_r = torch.empty_strided(shape, ostr, dtype=qr.dtype, device=dev)
        f_r = torch.empty(batch + (E, Ev), dtype=torch.float32, device=dev) if want_state else None
        named = [("q", qr), ("k", kr), ("v", vr), ("o", o_r)] + [("l", lr)] * (lam is not None)
        named += [("s", sr)] * (state is not None) + [("f", f_r)] * want_state
        rr = runs(batch + (1,), [t.stride()[:len(batch)] + (1,) for _, t in named])
        if len(rr) <= MAX_RUNS:
            break
    flags = ((_lib.LINATTN_REVERSE if reverse else 0) | (_lib.LINATTN_CONJ if conj else 0) | (_lib.LINATTN_LAG if lag else 0)
             | (_lib.LINATTN_SCALE_IN if scale_in else 0))
    d = _lib.LinAttnDesc(T=T, E=E, Ev=Ev, q_rs=qr.stride(-2), k_rs=kr.stride(-2), v_rs=vr.stride(-2), o_rs=o_r.stride(-2),
                         s_rs=sr.stride(-2) if state is not None else 0, f_rs=Ev, flags=flags, scale=float(scale))
    rows, _ = fill(d, rr, [name + "_stride" for name, _ in named])
    o_i = torch.empty_like(o_r)
    f_i = torch.empty_like(f_r) if want_state else None
    if rows and T:
        call("cplxamd_linattn", ptr(qr), ptr(qi), ptr(kr), ptr(ki), ptr(vr), ptr(vi), ptr(lr), ptr(li), ptr(sr), ptr(si),
             ptr(o_r), ptr(o_i), ptr(f_r), ptr(f_i), ctypes.byref(d), _lib.dtype_code(qr), stream_ptr())
    return o_r, o_i, f_r, f_i


def decay_gradient(q, dq, k, dk, final, gf, reverse):
    """dL/dlambda of the module docstring on plane pairs: q, dq, k, dk [*B, T, E], `final` the state after the last step
    and `gf` its gradient [*B, E, Ev] (or None) -> planes [*B, T] in float32 (float64 for float64 operands)."""
    ct = torch.float64 if q[0].dtype == torch.float64 else torch.float32
    (qr, qi), (ar, ai), (kr, ki), (br, bi) = ((t.to(ct) for t in p) for p in (q, dq, k, dk))
    # U - conj(W) per step, then its running sum from the last processed step back
    er = (qr * ar + qi * ai).sum(-1) - (kr * br + ki * bi).sum(-1)
    ei = (qr * ai - qi * ar).sum(-1) + (kr * bi - ki * br).sum(-1)
    if reverse:
        er, ei = er.cumsum(-1), ei.cumsum(-1)
    else:
        er, ei = er.flip(-1).cumsum(-1).flip(-1), ei.flip(-1).cumsum(-1).flip(-1)
    if gf is not None:                                    # the returned state: one more query row after the last step
        (fr, fi), (gr, gi) = ((t.to(ct) for t in p) for p in (final, gf))
        er = er + (fr * gr + fi * gi).sum((-1, -2)).unsqueeze(-1)
        ei = ei + (fr * gi - fi * gr).sum((-1, -2)).unsqueeze(-1)
    return er, ei


def _herm(p):
    """the conjugate transpose of a state"""
    return None if p is None else (p[0].transpose(-1, -2), -p[1].transpose(-1, -2))


def gradients(prim, q, k, v, lam, state, final, g, gf, scale, reverse, want):
    """The backward of the module docstring on plane pairs, with `prim` the primitive (`run`, or anything of its
    signature: tests/test_linear_attention_host.py passes the float64 loop).  lam, state, final (the state after the last
    step), gf (its gradient) in the compute type, lam's leading dims aligned to the batch; None where absent.
    `want` = (q, k, v, lam, state) -> (dq, dk, dv, dlam, dstate): plane pairs, dlam at the batch shape [*B, T], None
    where not wanted: a gradient that is not asked for is not launched."""
    want_q, want_k, want_v, want_l, want_s = want
    want_l, want_s = want_l and lam is not None, want_s and state is not None
    dq = dk = dv = dl = ds = None
    if want_q or want_l:
        dq = prim(g, v, k, lam, _herm(state), scale, reverse, conj=True, want_state=False)[:2]
    if want_k or want_l:
        dk = prim(v, g, q, lam, _herm(gf), scale, not reverse, lag=True, scale_in=True, want_state=False)[:2]
    if want_v or want_s:
        dvr, dvi, zr, zi = prim(k, q, g, lam, gf, scale, not reverse, conj=True, lag=True, scale_in=True, want_state=want_s)
        dv = (dvr, dvi)
        if want_s and lam is not None:                    # conj(exp lambda[first]) times what enters the first step
            at = q[0].shape[-2] - 1 if reverse else 0
            e = torch.exp(lam[0][..., at]).unsqueeze(-1).unsqueeze(-1)
            if lam[1] is None:
                zr, zi = e * zr, e * zi
            else:
                ang = lam[1][..., at].unsqueeze(-1).unsqueeze(-1)
                ar, ai = e * torch.cos(ang), -e * torch.sin(ang)
                zr, zi = ar * zr - ai * zi, ar * zi + ai * zr
        ds = (zr, zi) if want_s else None
    if want_l:
        dl = decay_gradient(q, dq, k, dk, final, gf, reverse)
    return dq, dk, dv, dl, ds


class _LinAttn(torch.autograd.Function):
    """(o_r, o_i, f_r, f_i) of the module docstring.  lr, li: the log-decay planes with their leading dims aligned to the
    batch (size 1 where they broadcast), li None for a real decay, both None without one; sr, si: the entering state or
    None.  meta = (scale, reverse)."""

    @staticmethod
    def forward(ctx, qr, qi, kr, ki, vr, vi, lr, li, sr, si, meta):
        scale, reverse = meta
        lam = None if lr is None else (lr.float(), None if li is None else li.float())
        state = None if sr is None else (sr.float(), si.float())
        o_r, o_i, f_r, f_i = run((qr, qi), (kr, ki), (vr, vi), lam, state, scale, reverse)
        ctx.meta = meta
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(qr, qi, kr, ki, vr, vi, lr, li, sr, si, f_r, f_i)
        return o_r, o_i, f_r.to(qr.dtype), f_i.to(qr.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gr, gi, gfr, gfi):
        qr, qi, kr, ki, vr, vi, lr, li, sr, si, f_r, f_i = ctx.saved_tensors
        scale, reverse = ctx.meta
        need = ctx.needs_input_grad
        zero = lambda t, like, shape: like.new_zeros(shape) if t is None else t      # noqa: E731
        shape_o = qr.shape[:-1] + vr.shape[-1:]
        g = (zero(gr, qr, shape_o), zero(gi, qr, shape_o))
        gf = None
        if gfr is not None or gfi is not None:
            gf = (zero(gfr, f_r, f_r.shape).float(), zero(gfi, f_r, f_r.shape).float())
        lam = None if lr is None else (lr.float(), None if li is None else li.float())
        state = None if sr is None else (sr.float(), si.float())
        want = tuple(need[i] or need[i + 1] for i in (0, 2, 4, 6, 8))
        dq, dk, dv, dl, ds = gradients(run, (qr, qi), (kr, ki), (vr, vi), lam, state, (f_r, f_i), g, gf, scale, reverse, want)
        grads = [None] * 10
        for i, (p, on) in enumerate(((dq, want[0]), (dk, want[1]), (dv, want[2]))):
            if on:
                grads[2 * i], grads[2 * i + 1] = p
        if dl is not None:                                # (a broadcast decay: summed over the rows that share it)
            grads[6] = dl[0].sum_to_size(lr.shape).to(lr.dtype)
            grads[7] = None if li is None else dl[1].sum_to_size(li.shape).to(li.dtype)
        if ds is not None:
            grads[8], grads[9] = ds[0].to(sr.dtype), ds[1].to(si.dtype)
        return tuple(t if need[i] else None for i, t in enumerate(grads)) + (None,)


def _mm(ar, ai, br, bi):
    return ar @ br - ai @ bi, ar @ bi + ai @ br


def _composed(q, k, v, lam, state, scale, reverse):
    """the quadratic masked form in torch products on plane pairs -> (o_r, o_i, f_r, f_i); lam and state as the
    Function's.  The weights are formed in float32 (float64 for float64 decays) and cast to the operands' dtype."""
    (qr, qi), (kr, ki), (vr, vi) = q, k, v
    dt, T = qr.dtype, qr.shape[-2]
    if reverse:
        qr, qi, kr, ki, vr, vi = (t.flip(-2) for t in (qr, qi, kr, ki, vr, vi))
    kh = (kr.transpose(-1, -2), -ki.transpose(-1, -2))
    pr, pi = _mm(qr, qi, *kh)
    mask = torch.ones(T, T, dtype=torch.bool, device=qr.device).tril()
    cexp = lambda re, im: (torch.exp(re).to(dt), None) if im is None else ((torch.exp(re) * torch.cos(im)).to(dt),    # noqa: E731
                                                                           (torch.exp(re) * torch.sin(im)).to(dt))
    cmul = lambda ar, ai, br, bi: (ar * br, ai * br) if bi is None else (ar * br - ai * bi, ar * bi + ai * br)         # noqa: E731
    if lam is not None:
        wide = lambda t: None if t is None else (t if t.dtype == torch.float64 else t.float())                         # noqa: E731
        lr, li = (None if t is None else (wide(t).flip(-1) if reverse else wide(t)).cumsum(-1) for t in lam)
        pair = lambda t: None if t is None else t.unsqueeze(-1) - t.unsqueeze(-2)                                      # noqa: E731
        pr, pi = cmul(pr, pi, *cexp(pair(lr).masked_fill(~mask, -math.inf), pair(li)))
    else:
        pr, pi = pr * mask, pi * mask
    o_r, o_i = _mm(pr, pi, vr, vi)
    wr, wi = vr, vi
    if lam is not None:                                   # what is left of step s's update after the last step
        left = lambda t: None if t is None else (t[..., -1:] - t).unsqueeze(-1)                                        # noqa: E731
        wr, wi = cmul(vr, vi, *cexp(left(lr), left(li)))
    f_r, f_i = _mm(kh[0], kh[1], wr, wi)
    if state is not None:
        sr, si = (t.to(dt) for t in state)
        cr, ci = _mm(qr, qi, sr, si)
        if lam is not None:
            one = lambda t: None if t is None else t.unsqueeze(-1)                                                     # noqa: E731
            cr, ci = cmul(cr, ci, *cexp(one(lr), one(li)))
            sr, si = cmul(sr, si, *cexp(one(one(lr[..., -1])), None if li is None else one(one(li[..., -1]))))
        o_r, o_i, f_r, f_i = o_r + cr, o_i + ci, f_r + sr, f_i + si
    o_r, o_i = o_r * scale, o_i * scale
    if reverse:
        o_r, o_i = o_r.flip(-2), o_i.flip(-2)
    return o_r, o_i, f_r, f_i


def _checked(fn, x, name, dims):
    from .cplx import Cplx
    if not isinstance(x, Cplx):
        kind = "a torch tensor of complex dtype" if torch.is_tensor(x) and x.is_complex() else f"a {type(x).__name__}"
        raise CplxAmdError(f"{fn}: `{name}` is {kind}, not a Cplx (wrap planes with Cplx(re, im))")
    re, im = x.real, x.imag
    if re.dtype != im.dtype or re.device != im.device:
        raise CplxAmdError(f"{fn}: the planes of `{name}` differ: {re.dtype} on {re.device} and {im.dtype} on {im.device}")
    if re.dim() < dims:
        raise ValueError(f"{fn}: `{name}` has {re.dim()} dims; it needs at least {dims}")
    return re, im


def _prepare(fn, query, key, value, log_decay, state, scale):
    """the checks shared by linear_attention and composed -> (q, k, v, lam, state as plane pairs or None, scale)"""
    (qr, qi), (kr, ki), (vr, vi) = (_checked(fn, x, n, 2) for x, n in ((query, "query"), (key, "key"), (value, "value")))
    if qr.shape[-1] != kr.shape[-1]:
        raise ValueError(f"{fn}: query has E = {qr.shape[-1]}, key has E = {kr.shape[-1]}")
    if not (qr.shape[-2] == kr.shape[-2] == vr.shape[-2]):
        raise ValueError(f"{fn}: query, key and value have T = {qr.shape[-2]}, {kr.shape[-2]}, {vr.shape[-2]}")
    if not (qr.shape[:-2] == kr.shape[:-2] == vr.shape[:-2]):
        raise ValueError(f"{fn}: the leading dims differ: {tuple(qr.shape[:-2])}, {tuple(kr.shape[:-2])}, "
                         f"{tuple(vr.shape[:-2])} (no broadcasting, no grouped heads)")
    if not (qr.dtype == kr.dtype == vr.dtype):
        raise CplxAmdError(f"{fn}: query, key and value have different dtypes: {qr.dtype}, {kr.dtype}, {vr.dtype}")
    if qr.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise CplxAmdError(f"{fn}: planes must be float32, bfloat16 or float64, got {qr.dtype}")
    batch, T, E, Ev = tuple(qr.shape[:-2]), qr.shape[-2], qr.shape[-1], vr.shape[-1]
    if min(E, Ev) < 1:
        raise ValueError(f"{fn}: E and Ev must be at least 1, got {E}, {Ev}")
    if max(E, Ev) > MAX_HEAD:
        raise CplxAmdError(f"{fn}: head sizes above {MAX_HEAD} are not offered, got E = {E}, Ev = {Ev}")
    lam = None
    if log_decay is not None:
        lr, li = planes(log_decay, "log_decay", fn)
        if not lr.is_floating_point():
            raise CplxAmdError(f"{fn}: `log_decay` must be of a floating dtype, got {lr.dtype}")
        ok = lr.dim() >= 1 and lr.dim() <= len(batch) + 1 and lr.shape[-1] == T
        ok = ok and all(a in (1, b) for a, b in zip(lr.shape[-2::-1], batch[::-1]))
        if not ok:
            raise ValueError(f"{fn}: `log_decay` must be broadcastable to {batch + (T,)}, got {tuple(lr.shape)}")
        lead = (None,) * (len(batch) + 1 - lr.dim())
        lam = (lr[lead], None if li is None else li[lead])
    if state is not None:
        sr, si = _checked(fn, state, "state", 2)
        if tuple(sr.shape) != batch + (E, Ev):
            raise ValueError(f"{fn}: `state` must be {batch + (E, Ev)}, got {tuple(sr.shape)}")
        if sr.dtype != qr.dtype:
            raise CplxAmdError(f"{fn}: `state` is {sr.dtype}, query is {qr.dtype}")
        state = (sr, si)
    return (qr, qi), (kr, ki), (vr, vi), lam, state, 1.0 / math.sqrt(E) if scale is None else float(scale)


def _finish(o_r, o_i, f_r, f_i, return_state):
    from .cplx import Cplx
    return (Cplx(o_r, o_i), Cplx(f_r, f_i)) if return_state else Cplx(o_r, o_i)


def _empty(q, v, state, return_state):
    """T = 0 or an empty batch: no launch; the state passes through"""
    (qr, _), (vr, _) = q, v
    o = [qr.new_empty(qr.shape[:-1] + vr.shape[-1:]) for _ in range(2)]
    f = state if state is not None else [qr.new_zeros(qr.shape[:-2] + (qr.shape[-1], vr.shape[-1])) for _ in range(2)]
    return _finish(*o, *f, return_state)


def composed(query, key, value, log_decay=None, state=None, return_state=False, scale=None, reverse=False):
    """cplx.linear_attention in its quadratic masked form, spelled with torch products on the planes: a [T, T] score
    matrix per batch entry.  Every dtype, on any device, differentiable to any order.  The route of float64 operands (the
    parity route) and the baseline of scripts/bench_linear_attention.py."""
    q, k, v, lam, state, scale = _prepare("linear_attention.composed", query, key, value, log_decay, state, scale)
    if q[0].shape[-2] == 0 or 0 in q[0].shape[:-2]:
        return _empty(q, v, state, return_state)
    return _finish(*_composed(q, k, v, lam, state, scale, bool(reverse)), return_state)


def linear_attention(query, key, value, log_decay=None, state=None, return_state=False, scale=None, reverse=False):
    """cplx.linear_attention (which documents it)"""
    q, k, v, lam, state, scale = _prepare(FN, query, key, value, log_decay, state, scale)
    if q[0].shape[-2] == 0 or 0 in q[0].shape[:-2]:
        return _empty(q, v, state, return_state)
    if q[0].dtype == torch.float64:
        return _finish(*_composed(q, k, v, lam, state, scale, bool(reverse)), return_state)
    require_device(*q, *k, *v, *(lam or ()), *(state or ()))
    none = (None, None)
    return _finish(*_LinAttn.apply(*q, *k, *v, *(lam or none), *(state or none), (scale, bool(reverse))), return_state)
