"""Recursive (IIR) filtering along the last dim on the chunk-parallel kernel of csrc/iir.hip: the argument handling, the
plan, the launch glue, the split path and the autograd Function behind cplx.lfilter and cplx.sosfilt.

One primitive (cplxamd_iir): for every row, a cascade of S direct-form-II-transposed sections of D states each runs over
the row from an entering state (zi, or zero), optionally in reverse time and with conjugated coefficients.  The
coefficients travel as ONE operand c [*Bc, S, 2 (D + 1)], section s holding b0 .. bD, a0 .. aD, already normalised (a0 is
not read; it receives no gradient: cplx.lfilter divides by a0 with torch, which is where a0's gradient comes from).

Write R(c; v) for the same filter run in reverse time with conjugated coefficients from zero state, and c|1 for c with
its numerator replaced by 1.  With autograd's convention (dL/dre + i dL/dim), incoming gradient g and gt = R(c|1; g):
    dx = R(c; g),   dzi = gt[..., :D],   db[k] = sum_n conj(x[n - k]) gt[n],   da[k] = -sum_n conj(y[n - k]) gt[n]  (k >= 1)
The two correlations are upfirdn.wgrad (a kernel that sums over the rows that share a filter, in fixed order), R is
the primitive with both flags flipped, so the backward of the Function is made of differentiable Functions and
derivatives of every order stay on these kernels.  For a cascade only dx is offered by the Function (one fused launch,
reversed, conjugated, sections in reverse order); cplx.sosfilt composes per-section Functions when `sos` or `zi` needs a
gradient.  The final state zf is returned by the kernel; where a gradient may flow it is instead formed from the last D
samples:  zf[i] = sum_{k > i} b_k x[N + i - k] - a_k y[N + i - k]  (+ zi[i + N] when N < D), with torch on D-sized slices.

A real operand is a null imaginary plane (never read, no zero plane allocated); all-real operands run the real kernels.
Leading dims broadcast by torch's rules and are read where they lie, under _runs.py's rule of three batch runs,
otherwise one differentiable copy.  State planes are kept in the compute type (float32 for bfloat16 operands) and rounded
once.  Workspaces come from torch's allocator and nothing reads a device value on the host: calls can be captured in a
hipGraph.

Long rows with few rows take the SPLIT path (the plan decides; `_FORCE_SEGMENTS` forces it): each row is cut into
segments, and four launches of the primitive and of a tiny scan kernel replace the one launch -- segment-final states
from zero entering state; the segment transition matrix from unit entering states on null input; a sequential scan of
the segments of each row; the run from the true entering states (`split`, which filtfilt.py runs with its own launcher).
No workgroup waits for another inside a launch.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense, fill, fit, planes, share

PATHS = ("row", "split")                                   # cplxamd_iir_plan's return codes
MAX_ORDER = 8                                              # states of one direct-form section
MAX_SECTIONS = 16                                          # sections of one launch; longer cascades are chained
_FORCE_SEGMENTS = 0                                        # private: > 0 cuts every row into that many segments (tests, bench)


def plan(n, order, sections=1, rows=1, filters=1, dtype=torch.float32, cplx=True, force_segments=None):
    """The plan for rows of `n` samples through `sections` sections of `order` states -- a pure host call, no GPU needed
    -> dict: path ("row" / "split") and the fields of _lib.IIR_PLAN_FIELDS (chunk, lanes, tile, tiles per segment,
    segments, seg_len, compiled states, LDS bytes, threads, grid, workspace bytes of the split path)."""
    out = (ctypes.c_int64 * len(_lib.IIR_PLAN_FIELDS))()
    force = _FORCE_SEGMENTS if force_segments is None else force_segments
    rc = _lib.load().cplxamd_iir_plan(int(n), int(order), int(sections), int(rows), int(filters), code(dtype),
                                      int(bool(cplx)), int(force), out)
    if rc == -3:
        raise CplxAmdError(f"iir: rows of {n} samples in {rows} rows exceed what the kernel indexes (2^40 samples, "
                           "2^31 - 1 workgroups)")
    if rc < 0:
        raise CplxAmdError(f"iir: no plan for order {order} with {sections} section(s) (one section of 1 .. {MAX_ORDER} "
                           f"states, or up to {MAX_SECTIONS} sections of 1 .. 2 states; n >= 1)")
    p = dict(zip(_lib.IIR_PLAN_FIELDS, out))
    p["path"] = PATHS[rc]
    return p


def _ct(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def _call(xr, xi, cr, ci, zr, zi, yr, yi, fr, fi, runs, n, x_es, order, sections, segs, seg_len, flags, cx, dtype):
    d = _lib.IirDesc(n=n, order=order, sections=sections, segments=segs, seg_len=seg_len, x_es=x_es, flags=flags)
    fill(d, runs, ("x_stride", "c_stride", "y_stride"))
    call("cplxamd_iir", ptr(xr), ptr(xi), ptr(cr), ptr(ci), ptr(zr), ptr(zi), ptr(yr), ptr(yi), ptr(fr), ptr(fi),
         ctypes.byref(d), int(cx), code(dtype), stream_ptr())


def split(launch, scan, plan_of, enter, x, y, runs, n, S, D, cx, ct, want_zf):
    """The split path of one pass, for iir.py and filtfilt.py.  `runs`: the pass's batch runs, the coefficients' strides
    in column 2; `plan_of(rows, filters)`: the caller's plan; `launch(x, z, y, f, runs, n, segs, seg_len)`: one launch of
    the caller's primitive on plane pairs -- x of n samples a row ((None, None): null input), the entering states z, y
    and the final states f; `scan`: the caller's module-level `call`; `enter()`: the row's entering state, planes of
    [rows, S D] entries in the compute type `ct`, asked for when the scan needs it.
    -> None, and nothing launched, where the rows stay whole: the plan says so, or the rows that share a filter are not
    consecutive, or the filters do not fit two batch runs; else the four launches, and the final state planes
    [rows, segs, S, D] of every segment ((None, None) unless `want_zf`)."""
    kept = [r for r in runs if r[2] != 0]
    rows, filters, w = math.prod(r[0] for r in runs), math.prod(r[0] for r in kept), S * D
    p = plan_of(rows, filters)
    segs, seg_len = p["segments"], p["seg_len"]
    shared_inner = all(r[2] == 0 for r in runs[len(kept):]) and all(r[2] != 0 for r in runs[:len(kept)])
    if segs == 1 or not (shared_inner and len(kept) <= 2):
        return None
    dev, none = x[0].device, (None, None)
    new = lambda *s: (torch.empty(s, dtype=ct, device=dev), torch.empty(s, dtype=ct, device=dev) if cx else None)  # noqa: E731
    # 1. segment-final states from zero entering state (in reverse time, segment 0 is the END of the row)
    z = new(rows, segs, S, D)
    launch(x, none, none, z, runs, n, segs, seg_len)
    # 2. the transition of a full segment: unit entering states on null input, one row per (filter, unit state)
    eye = torch.eye(w, dtype=ct, device=dev).reshape(1, w, 1, S, D).expand(filters, w, 1, S, D).contiguous()
    m = new(filters * w, 1, S, D)
    mruns = [[r[0], 0, r[2]] for r in kept] + [[w]]      # (the strides a run leaves out are zero)
    launch(none, (eye, None), none, m, mruns, seg_len, 1, seg_len)
    # 3. the entering state of every segment: a sequential scan per row
    s = enter()
    e = new(rows, segs, S, D)
    scan("cplxamd_iir_scan", ptr(z[0]), ptr(z[1]), ptr(m[0]), ptr(m[1]), ptr(s[0]), ptr(s[1]), ptr(e[0]), ptr(e[1]), rows,
         rows // max(filters, 1), segs, w, int(cx), code(ct), stream_ptr())
    # 4. every segment from its true entering state; the last segment's final state is the row's
    f = new(rows, segs, S, D) if want_zf else none
    launch(x, e, y, f, runs, n, segs, seg_len)
    return f


def run(xr, xi, cr, ci, zr, zi, reverse=False, conj=False, cx=None, want_zf=False, force_segments=None):
    """The module-level primitive, without autograd: x [*B, N] planes (views welcome), c [*Bc, S, 2 (D + 1)] planes with
    Bc broadcastable to B, as many dims, and dense last two dims, zi [*B, S, D] planes or None -> (yr, yi, fr, fi): y
    [*B, N] and, if `want_zf`, the final state [*B, S, D] (else None), in the operands' dtype.  xi, ci, zi's imaginary
    plane may be None; yi / fi are None when every operand is real (`cx` False)."""
    batch, n = tuple(xr.shape[:-1]), xr.shape[-1]
    S, W = cr.shape[-2], cr.shape[-1]
    D = W // 2 - 1
    dtype, ct, dev = xr.dtype, _ct(xr.dtype), xr.device
    if cx is None:
        cx = xi is not None or ci is not None or (zr is not None and zi is not None)
    shape = batch + (n,)
    yr = torch.empty(shape, dtype=dtype, device=dev)
    yi = torch.empty_like(yr) if cx else None
    rows = math.prod(batch)

    def state(t):                                         # [rows, 1, S, D] in the compute type, dense
        return None if t is None else t.expand(batch + (S, D)).to(ct).reshape(rows, 1, S, D).contiguous()

    ((xr, xi), (cr, ci)), runs = fit(shape, [(xr, xi), (cr, ci)], dense(shape), [(0,), (1,)])
    flags = (_lib.IIR_REVERSE if reverse else 0) | (_lib.IIR_CONJ if conj else 0)
    zr, zi = state(zr), state(zi) if cx else None

    def launch(x, z, y, f, runs, n, segs, seg_len):
        _call(*x, cr, ci, *z, *y, *f, runs, n, 0 if x[0] is None else xr.stride(-1), D, S, segs, seg_len, flags, cx, dtype)

    f = split(launch, call, lambda r, k: plan(n, D, S, r, k, dtype, cx, force_segments), lambda: (zr, zi), (xr, xi), (yr, yi),
              runs, n, S, D, cx, ct, True)
    if f is None:
        f = (torch.empty(rows, 1, S, D, dtype=ct, device=dev) if want_zf else None,
             torch.empty(rows, 1, S, D, dtype=ct, device=dev) if want_zf and cx else None)
        launch((xr, xi), (zr, zi), (yr, yi), f, runs, n, 1, n)
    if not want_zf:
        return yr, yi, None, None
    back = lambda t: None if t is None else t[:, -1].reshape(batch + (S, D)).to(dtype)  # noqa: E731
    return yr, yi, back(f[0]), back(f[1])


def _conj_planes(pr, pi, flip):
    return pr, (None if pi is None else -pi) if flip else pi


class _Iir(torch.autograd.Function):
    """(yr, yi) = the cascade c [*Bc, S, 2 (D + 1)] over x [*B, N] from the state z [*B, S, D] (or None), in forward or
    reverse time, with the coefficients as they are or conjugated; xi, ci, zi may be None; yi is None unless `cx`."""

    @staticmethod
    def forward(ctx, xr, xi, cr, ci, zr, zi, meta):
        reverse, conj, cx = meta
        yr, yi, _, _ = run(xr, xi, cr, ci, zr, zi, reverse, conj, cx)
        ctx.meta = meta
        ctx.save_for_backward(xr, xi, cr, ci, zr, zi, yr, yi)
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        from . import upfirdn
        xr, xi, cr, ci, zr, zi, yr, yi = ctx.saved_tensors
        reverse, conj, cx = ctx.meta
        gi = gi if cx else None
        need = ctx.needs_input_grad
        S, D = cr.shape[-2], cr.shape[-1] // 2 - 1
        n = xr.shape[-1]
        dx = dc = dz = (None, None)
        if need[0] or need[1]:
            back = (cr.flip(-2), None if ci is None else ci.flip(-2)) if S > 1 else (cr, ci)
            dx = filt(gr, gi, *back, None, None, not reverse, not conj, cx)
        if any(need[2:6]):
            if S != 1:
                raise CplxAmdError("iir: the fused cascade has a gradient for the signal only; cplx.sosfilt composes "
                                   "per-section filters when `sos` or `zi` requires one")
            one = torch.zeros(D + 1, dtype=cr.dtype, device=cr.device)
            one[0] = 1
            ap_r = torch.cat([one.expand(cr.shape[:-1] + (D + 1,)), cr[..., D + 1:]], -1)
            ap_i = None if ci is None else torch.cat([torch.zeros_like(ci[..., :D + 1]), ci[..., D + 1:]], -1)
            tr, ti = filt(gr, gi, ap_r, ap_i, None, None, not reverse, not conj, cx)     # gt = R(c|1; g)
            if need[2] or need[3]:
                fshape = tuple(cr.shape[:-2])
                out_imag = ci is not None

                def corr(ur, ui):                         # sum_n conj(u_p[t - k]) gt_p[t] in process order
                    if not reverse:
                        return upfirdn.wgrad(ur, ui, tr, ti, 1, 1, 0, D + 1, fshape, out_imag)
                    return _conj_planes(*upfirdn.wgrad(tr, ti, ur, ui, 1, 1, 0, D + 1, fshape, out_imag), True)

                br_, bi_ = corr(xr, xi)
                ar_, ai_ = corr(yr, yi)
                keep = torch.ones(D + 1, dtype=cr.dtype, device=cr.device)
                keep[0] = 0                               # a0 is not an operand of the kernel
                dcr = torch.cat([br_, -ar_ * keep], -1).unsqueeze(-2)
                dci = None if bi_ is None else torch.cat([bi_, -ai_ * keep], -1).unsqueeze(-2)
                dc = _conj_planes(dcr, dci, conj)
            if need[4] or need[5]:
                def head(t):
                    if t is None:
                        return None
                    h = t[..., :D] if not reverse else t[..., max(n - D, 0):].flip(-1)
                    if n < D:
                        h = torch.nn.functional.pad(h, (0, D - n))
                    return h.unsqueeze(-2)
                dz = (head(tr), head(ti))
        pick = lambda t, k: t if need[k] else None        # noqa: E731
        return pick(dx[0], 0), pick(dx[1], 1), pick(dc[0], 2), pick(dc[1], 3), pick(dz[0], 4), pick(dz[1], 5), None


def filt(xr, xi, cr, ci, zr, zi, reverse=False, conj=False, cx=None):
    """The primitive on planes, differentiable to any order: x [*B, N] (views welcome), c [*Bc, S, 2 (D + 1)] with Bc
    broadcastable to B and as many dims, z [*B, S, D] or None -> (yr, yi), yi None when every operand is real."""
    xr, xi = share(xr, xi)
    cr, ci = share(cr, ci)
    if zr is not None:
        zr, zi = share(zr, zi)
    if cr.stride()[-2:] != (cr.shape[-1], 1) and cr.numel():
        cr, ci = cr.contiguous(), None if ci is None else ci.contiguous()
    if cx is None:
        cx = xi is not None or ci is not None or (zr is not None and zi is not None)
    shape = tuple(xr.shape)
    ((xr, xi), (cr, ci)), _ = fit(shape, [(xr, xi), (cr, ci)], dense(shape), [(0,), (1,)])   # copies: x, then c expanded
    return _Iir.apply(xr, xi, cr, ci, zr, zi, (bool(reverse), bool(conj), bool(cx)))


# ---- complex arithmetic on (re, im | None) planes: coefficient- and state-sized tensors only ----------------------------
def _cmul(ar, ai, br, bi):
    if ai is None and bi is None:
        return ar * br, None
    if ai is None:
        return ar * br, ar * bi
    if bi is None:
        return ar * br, ai * br
    return ar * br - ai * bi, ar * bi + ai * br


def _cdiv(ar, ai, br, bi):
    if bi is None:
        return ar / br, None if ai is None else ai / br
    den = br * br + bi * bi
    if ai is None:
        return ar * br / den, -(ar * bi) / den
    return (ar * br + ai * bi) / den, (ai * br - ar * bi) / den


def _cadd(ar, ai, br, bi):
    if ai is None and bi is None:
        return ar + br, None
    if ai is None:
        return ar + br, bi + torch.zeros_like(ar)
    if bi is None:
        return ar + br, ai + torch.zeros_like(br)
    return ar + br, ai + bi


def _final_state(xr, xi, yr, yi, br, bi, ar, ai, zr, zi, D):
    """zf [*B, D] of one section from the last D samples of x and y (and zi where the row is shorter than D): torch on
    D-sized slices, differentiable.  b, a [*Bc, D + 1] normalised; z [*B, D] or None."""
    n = xr.shape[-1]
    m = min(n, D)
    pad = torch.nn.functional.pad
    tail = lambda t: None if t is None else pad(t[..., n - m:], (D - m, 0))  # noqa: E731
    xr, xi, yr, yi = tail(xr), tail(xi), tail(yr), tail(yi)
    fr = fi = None
    for k in range(1, D + 1):
        sl = lambda t: None if t is None else t[..., D - k:]                  # noqa: E731
        co = lambda t: None if t is None else t[..., k:k + 1]                 # noqa: E731
        pr, pi = _cmul(co(br), co(bi), sl(xr), sl(xi))
        qr, qi = _cmul(co(ar), co(ai), sl(yr), sl(yi))
        tr, ti = _cadd(pr, pi, -qr, None if qi is None else -qi)
        tr, ti = pad(tr, (0, D - k)), None if ti is None else pad(ti, (0, D - k))
        fr, fi = (tr, ti) if fr is None else _cadd(fr, fi, tr, ti)
    if zr is not None and n < D:
        sh = lambda t: None if t is None else pad(t[..., n:], (0, n))         # noqa: E731
        fr, fi = _cadd(fr, fi, sh(zr), sh(zi))
    return fr, fi


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _section(xr, xi, cr, ci, zr, zi, D, cx):
    """one direct-form section c [*Bc, 1, 2 (D + 1)] over x [*B, N] with z [*B, D] or None -> (yr, yi, fr, fi); the
    final state only when z is given"""
    z3 = lambda t: None if t is None else t.unsqueeze(-2)                     # noqa: E731
    if zr is None:
        return filt(xr, xi, cr, ci, None, None, False, False, cx) + (None, None)
    if not _needs_grad(xr, xi, cr, ci, zr, zi):
        yr, yi, fr, fi = run(xr, xi, cr.contiguous(), None if ci is None else ci.contiguous(), z3(zr), z3(zi), False, False,
                             cx, True)
        return yr, yi, fr.squeeze(-2), None if fi is None else fi.squeeze(-2)
    yr, yi = filt(xr, xi, cr, ci, z3(zr), z3(zi), False, False, cx)
    c1 = lambda t, lo: None if t is None else t[..., 0, lo:lo + D + 1]        # noqa: E731
    fr, fi = _final_state(xr, xi, yr, yi, c1(cr, 0), c1(ci, 0), c1(cr, D + 1), c1(ci, D + 1), zr, zi, D)
    if cx and fi is None:
        fi = torch.zeros_like(fr)
    return yr, yi, fr, fi


def _operands(fn, named):
    """planes of every operand, with the checks the two functions share -> {name: (re, im)}"""
    out, first = {}, None
    for name, v in named:
        if v is None:
            out[name] = (None, None)
            continue
        pr, pi = planes(v, name, fn)
        if pr.dim() == 0:
            raise ValueError(f"{fn}: `{name}` is 0-d: there is no dim to filter along")
        if first is None:
            first = (name, pr.dtype)
        elif pr.dtype != first[1]:
            raise CplxAmdError(f"{fn}: the operands have different dtypes: `{first[0]}` is {first[1]}, `{name}` is {pr.dtype}")
        out[name] = (pr, pi)
    code(first[1])
    return out


def _wrap(pr, pi):
    from .cplx import Cplx
    return pr if pi is None else Cplx(pr, pi)


def _lead(t, nd, tail):
    """t [*b, *tail dims] with leading singleton dims added up to nd batch dims"""
    return None if t is None else t[(None,) * (nd - (t.dim() - tail))]


def lfilter(b, a, x, zi=None):
    """cplx.lfilter (which documents it)"""
    from . import upfirdn
    fn = "lfilter"
    ops = _operands(fn, (("b", b), ("a", a), ("x", x), ("zi", zi)))
    (br, bi), (ar, ai), (xr, xi), (zr, zi_) = ops["b"], ops["a"], ops["x"], ops["zi"]
    nb, na, n = br.shape[-1], ar.shape[-1], xr.shape[-1]
    if nb == 0 or na == 0:
        raise ValueError(f"{fn}: the last dim of `{'b' if nb == 0 else 'a'}` is empty")
    D = max(na, nb) - 1
    if zr is not None and zr.shape[-1] != D:
        raise ValueError(f"{fn}: `zi` must have max(len(a), len(b)) - 1 = {D} entries along its last dim, got {zr.shape[-1]}")
    if na - 1 > MAX_ORDER:
        raise CplxAmdError(f"{fn}: a denominator of order {na - 1} exceeds the direct form's {MAX_ORDER}: direct forms of that "
                           "order are not sound in float32 -- factor the filter into second-order sections and use "
                           "cplx.sosfilt")
    lead = [t.shape[:-1] for t in (xr, br, ar) + ((zr,) if zr is not None else ())]
    batch = tuple(torch.broadcast_shapes(*lead))          # RuntimeError, as torch raises it
    require_device(xr, xi, br, bi, ar, ai, zr, zi_)
    nd = len(batch)
    cx = any(t is not None for t in (xi, bi, ai, zi_))
    expand = lambda t, last: None if t is None else t.expand(batch + (last,))     # noqa: E731
    xr, xi, zr, zi_ = expand(xr, n), expand(xi, n), expand(zr, D), expand(zi_, D)
    if n == 0 or 0 in batch:                              # nothing to launch
        yr = torch.empty(batch + (n,), dtype=xr.dtype, device=xr.device)
        yi = torch.empty_like(yr) if cx else None
        if zr is None:
            return _wrap(yr, yi)
        return _wrap(yr, yi), _wrap(zr.clone(), (torch.zeros_like(zr) if zi_ is None else zi_.clone()) if cx else None)
    # a0 normalises both, by differentiable division
    a0r, a0i = ar[..., :1], None if ai is None else ai[..., :1]
    br, bi = _cdiv(br, bi, a0r, a0i)
    ar, ai = _cdiv(ar, ai, a0r, a0i)
    pad = torch.nn.functional.pad
    if D == 0:                                            # a scale: one tap of the polyphase kernel
        yr, yi = upfirdn.conv(xr, xi, _lead(br, nd, 1), _lead(bi, nd, 1), 1, 1, 0, n, False, cx)
        return _wrap(yr, yi) if zr is None else (_wrap(yr, yi), _wrap(zr.clone(), None if not cx else torch.zeros_like(zr)))
    cb = tuple(torch.broadcast_shapes(br.shape[:-1], ar.shape[:-1]))
    if nb - 1 > MAX_ORDER:
        # COMPOSED: the numerator as one polyphase launch (first N entries), zi as an added sequence, then the all-pole kernel
        vr, vi = upfirdn.conv(xr, xi, _lead(br, nd, 1), _lead(bi, nd, 1), 1, 1, 0, n, False, xi is not None or bi is not None)
        if zr is not None:
            seq = lambda t: None if t is None else (t[..., :n] if n <= D else pad(t, (0, n - D)))     # noqa: E731
            vr, vi = _cadd(vr, vi, seq(zr), seq(zi_))
        Da = max(na - 1, 1)
        one = torch.zeros(Da + 1, dtype=xr.dtype, device=xr.device)
        one[0] = 1
        apr = pad(ar, (0, Da + 1 - na))
        cr = torch.cat([one.expand(apr.shape), apr], -1)
        ci = None if ai is None else torch.cat([torch.zeros_like(apr), pad(ai, (0, Da + 1 - na))], -1)
        yr, yi = filt(vr, vi, _lead(cr, nd, 1).unsqueeze(-2), None if ci is None else _lead(ci, nd, 1).unsqueeze(-2), None, None,
                      False, False, cx)
        if zr is None:
            return _wrap(yr, yi)
        full = lambda t, k: None if t is None else pad(t, (0, D + 1 - k)).expand(cb + (D + 1,))       # noqa: E731
        fr, fi = _final_state(xr, xi, yr, yi, _lead(full(br, nb), nd, 1), _lead(full(bi, nb), nd, 1), _lead(full(ar, na), nd, 1),
                              _lead(full(ai, na), nd, 1), zr, zi_, D)
        return _wrap(yr, yi), _wrap(fr, torch.zeros_like(fr) if cx and fi is None else fi)
    full = lambda t, k: pad(t, (0, D + 1 - k)).expand(cb + (D + 1,))              # noqa: E731
    cr = torch.cat([full(br, nb), full(ar, na)], -1)
    ci = None
    if bi is not None or ai is not None:
        zero = lambda: torch.zeros(cb + (D + 1,), dtype=xr.dtype, device=xr.device)                   # noqa: E731
        ci = torch.cat([zero() if bi is None else full(bi, nb), zero() if ai is None else full(ai, na)], -1)
    yr, yi, fr, fi = _section(xr, xi, _lead(cr, nd, 1).unsqueeze(-2), None if ci is None else _lead(ci, nd, 1).unsqueeze(-2),
                              zr, zi_, D, cx)
    return _wrap(yr, yi) if zr is None else (_wrap(yr, yi), _wrap(fr, fi))


def sosfilt(sos, x, zi=None):
    """cplx.sosfilt (which documents it)"""
    fn = "sosfilt"
    ops = _operands(fn, (("sos", sos), ("x", x), ("zi", zi)))
    (sr, si), (xr, xi), (zr, zi_) = ops["sos"], ops["x"], ops["zi"]
    if sr.dim() < 2 or sr.shape[-1] != 6:
        raise ValueError(f"{fn}: `sos` must be [..., n_sections, 6], got {tuple(sr.shape)}")
    S, n = sr.shape[-2], xr.shape[-1]
    if S == 0:
        raise ValueError(f"{fn}: `sos` has no sections")
    if zr is not None and (zr.dim() < 2 or tuple(zr.shape[-2:]) != (S, 2)):
        raise ValueError(f"{fn}: `zi` must be [..., n_sections, 2] = [..., {S}, 2], got {tuple(zr.shape)}")
    lead = [xr.shape[:-1], sr.shape[:-2]] + ([zr.shape[:-2]] if zr is not None else [])
    batch = tuple(torch.broadcast_shapes(*lead))
    require_device(xr, xi, sr, si, zr, zi_)
    nd = len(batch)
    cx = any(t is not None for t in (xi, si, zi_))
    xr, xi = xr.expand(batch + (n,)), None if xi is None else xi.expand(batch + (n,))
    if zr is not None:
        zr, zi_ = zr.expand(batch + (S, 2)), None if zi_ is None else zi_.expand(batch + (S, 2))
    if n == 0 or 0 in batch:
        yr = torch.empty(batch + (n,), dtype=xr.dtype, device=xr.device)
        yi = torch.empty_like(yr) if cx else None
        if zr is None:
            return _wrap(yr, yi)
        return _wrap(yr, yi), _wrap(zr.clone(), (torch.zeros_like(zr) if zi_ is None else zi_.clone()) if cx else None)
    # every section is normalised by its a0
    a0r, a0i = sr[..., 3:4], None if si is None else si[..., 3:4]
    cr, ci = _cdiv(sr, si, a0r, a0i)
    cr, ci = _lead(cr, nd, 2), _lead(ci, nd, 2)
    yr, yi = xr, xi
    if _needs_grad(sr, si, zr, zi_) or (zr is not None and _needs_grad(xr, xi)):
        # COMPOSED (not the hot path): one differentiable direct-form launch per section
        frs, fis = [], []
        for s in range(S):
            sec = lambda t: None if t is None else t[..., s:s + 1, :]         # noqa: E731
            st = lambda t: None if t is None else t[..., s, :]                # noqa: E731
            yr, yi, fr, fi = _section(yr, yi, sec(cr), sec(ci), st(zr), st(zi_), 2, cx)
            frs.append(fr)
            fis.append(fi)
        if zr is None:
            return _wrap(yr, yi)
        return _wrap(yr, yi), _wrap(torch.stack(frs, -2), torch.stack(fis, -2) if cx else None)
    frs, fis = [], []
    for s0 in range(0, S, MAX_SECTIONS):                  # launches of up to MAX_SECTIONS sections, chained
        part = lambda t: None if t is None else t[..., s0:s0 + MAX_SECTIONS, :]   # noqa: E731
        if zr is None:
            yr, yi = filt(yr, yi, part(cr), part(ci), None, None, False, False, cx)
            continue
        pc = lambda t: None if t is None else part(t).contiguous()            # noqa: E731
        yr, yi, fr, fi = run(yr, yi, pc(cr), pc(ci), part(zr), part(zi_), False, False, cx, True)
        frs.append(fr)
        fis.append(fi)
    if zr is None:
        return _wrap(yr, yi)
    return _wrap(yr, yi), _wrap(torch.cat(frs, -2), torch.cat(fis, -2) if cx else None)
