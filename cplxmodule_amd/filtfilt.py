"""Zero-phase filtering along the last dim on the extended pass of the recurrence kernel (csrc/filtfilt.hip, DESIGN section
23): the steady-state initial conditions (lfilter_zi, sosfilt_zi), the argument handling, the plan, the two passes with
their split path and the composed routes behind cplx.filtfilt and cplx.sosfiltfilt.

scipy's filtfilt(method="pad"): extend x by e samples on each side (odd: 2 x[0] - x[e - m]; even: x[e - m]; constant:
x[0]; the right side mirrored), run the filter forward over the extension from the state zi_unit * ext[0], run it again
over the reversed result from zi_unit * (its first sample), reverse, drop the e samples at each end.  Here that is two
launches of cplxamd_filtfilt_pass:
    pass 1   x, read where it lies through the kernel's index map  ->  a workspace of n + 2 e samples in the COMPUTE type
    pass 2   the workspace in reverse time                         ->  y, the logical samples [e, e + n), operands' dtype
Both take the unit state [*Bc, S, D] (compute type) and scale it in the kernel by the first sample they process.  No padded
copy, no flip, no slice; for bfloat16 operands the intermediate is never rounded.  Rows that the plan cuts into segments
take iir.py's split path per pass (four launches each); the scaled state then enters the scan, formed with state-sized
torch ops.  Everything else here is coefficient- and state-sized torch arithmetic; nothing reads a device value on the
host, so a call can be captured in a hipGraph.

When an operand requires grad, or the filter is beyond the fused kernel (D = 0, nb - 1 > 8, more than 16 sections), the
result is COMPOSED from the differentiable pieces: a torch extension, cplx.lfilter / cplx.sosfilt with zi, flips.  That
is not the hot path.
"""
import ctypes

import torch

from . import _lib
from . import iir as _iir
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code, dense, fill, fit
from .iir import MAX_ORDER, MAX_SECTIONS, PATHS, _cdiv, _cmul, _ct, _lead, _needs_grad, _operands, _wrap

PADTYPES = ("odd", "even", "constant", None)


# ---- the index map and the plan: pure host calls ---------------------------------------------------------------------------
def src_index(m, n, edge, padtype):
    """(j, k) of logical sample m of a row of n samples extended by `edge` on each side -- the kernel's own index map:
    the sample is x[j] (k == -1), x[k] (j == -1) or 2 x[k] - x[j].  `padtype` is a name, None (edge 0) or a mode code."""
    out = (ctypes.c_int64 * 2)()
    mode = padtype if isinstance(padtype, int) else _lib.FILTFILT_MODES["odd" if padtype is None else padtype]
    if _lib.load().cplxamd_filtfilt_src(int(m), int(n), int(edge), mode, out) != 0:
        raise CplxAmdError(f"filtfilt: no logical sample {m} in a row of {n} samples extended by {edge}")
    return out[0], out[1]


def plan(n, edge, order, sections=1, rows=1, filters=1, dtype=torch.float32, cplx=True, force_segments=None):
    """The plan of one pass over rows of `n` samples extended by `edge` on each side -- a pure host call -> dict: path
    ("row" / "split") and the fields of _lib.FILTFILT_PLAN_FIELDS: iir.plan's for the extended row (LDS bytes with the two
    anchors per plane), ext_len = n + 2 edge, signal_bytes = the intermediate workspace between the two passes."""
    out = (ctypes.c_int64 * len(_lib.FILTFILT_PLAN_FIELDS))()
    force = _iir._FORCE_SEGMENTS if force_segments is None else force_segments
    rc = _lib.load().cplxamd_filtfilt_plan(int(n), int(edge), int(order), int(sections), int(rows), int(filters),
                                           code(dtype), int(bool(cplx)), int(force), out)
    if rc == -3:
        raise CplxAmdError(f"filtfilt: rows of {n} + 2 * {edge} samples in {rows} rows exceed what the kernel indexes (2^40 "
                           "samples, 2^31 - 1 workgroups)")
    if rc < 0:
        raise CplxAmdError(f"filtfilt: no plan for order {order} with {sections} section(s) and an edge of {edge} on {n} "
                           f"samples (one section of 1 .. {MAX_ORDER} states, or up to {MAX_SECTIONS} sections of 1 .. 2 "
                           "states; 0 <= edge < n)")
    p = dict(zip(_lib.FILTFILT_PLAN_FIELDS, out))
    p["path"] = PATHS[rc]
    return p


# ---- the steady state of the unit step: coefficient-sized torch arithmetic, any device, differentiable ---------------------
def _joined(pr, pi):
    """planes -> one tensor: real, or complex when there is an imaginary plane (coefficient-sized only)"""
    return pr if pi is None else torch.complex(pr, pi)


def _split(t):
    return (t.real.contiguous(), t.imag.contiguous()) if t.is_complex() else (t, None)


def _zi_direct(b, a):
    """b, a [..., D + 1], normalised (a[..., 0] = 1) -> the direct-form-II-transposed state of the unit-step steady state,
    [..., D], in closed form: zi[0] = sum_{k >= 1} (b_k - a_k b_0) / sum_k a_k,
    zi[k] = (1 + a_1 + .. + a_k) zi[0] - sum_{j = 1 .. k} (b_j - a_j b_0)"""
    d = b.shape[-1] - 1
    if d == 0:
        return b[..., :0]
    c = (b[..., 1:] - a[..., 1:] * b[..., :1]).cumsum(-1)
    z0 = c[..., -1:] / a.sum(-1, keepdim=True)
    return a[..., :d].cumsum(-1) * z0 - torch.cat([torch.zeros_like(c[..., :1]), c[..., :-1]], -1)


def _zi_sos(sos):
    """sos [..., S, 6], every section normalised -> [..., S, 2]: each biquad's steady state times the DC gain of the
    sections before it"""
    b, a = sos[..., :3], sos[..., 3:]
    gain = (b.sum(-1) / a.sum(-1)).cumprod(-1)
    before = torch.cat([torch.ones_like(gain[..., :1]), gain[..., :-1]], -1)
    return _zi_direct(b, a) * before.unsqueeze(-1)


def _work(t):
    """bfloat16 coefficients are worked on in float32"""
    return None if t is None else (t.float() if t.dtype == torch.bfloat16 else t)


def _padded_ba(br, bi, ar, ai):
    """planes of b [..., nb], a [..., na] -> (b, a) [*cb, D + 1] joined tensors, normalised by a[..., 0], zero-padded"""
    nb, na = br.shape[-1], ar.shape[-1]
    d = max(na, nb) - 1
    a0r, a0i = ar[..., :1], None if ai is None else ai[..., :1]
    b = _joined(*_cdiv(br, bi, a0r, a0i))
    a = _joined(*_cdiv(ar, ai, a0r, a0i))
    if b.is_complex() != a.is_complex():
        b, a = (b, a + 0j) if b.is_complex() else (b + 0j, a)
    cb = tuple(torch.broadcast_shapes(b.shape[:-1], a.shape[:-1]))
    pad = torch.nn.functional.pad
    full = lambda t, k: (pad(t, (0, d + 1 - k)) if d + 1 > k else t).expand(cb + (d + 1,))   # noqa: E731
    return full(b, nb), full(a, na)


def _normalised_sos(sr, si):
    return _joined(*_cdiv(sr, si, sr[..., 3:4], None if si is None else si[..., 3:4]))


def lfilter_zi(b, a):
    """cplx.lfilter_zi (which documents it)"""
    fn = "lfilter_zi"
    ops = _operands(fn, (("b", b), ("a", a)))
    (br, bi), (ar, ai) = ops["b"], ops["a"]
    if br.shape[-1] == 0 or ar.shape[-1] == 0:
        raise ValueError(f"{fn}: the last dim of `{'b' if br.shape[-1] == 0 else 'a'}` is empty")
    zr, zi = _split(_zi_direct(*_padded_ba(_work(br), _work(bi), _work(ar), _work(ai))))
    back = lambda t: None if t is None else t.to(br.dtype)                    # noqa: E731
    return _wrap(back(zr), back(zi))


def _check_sos(fn, sr):
    if sr.dim() < 2 or sr.shape[-1] != 6:
        raise ValueError(f"{fn}: `sos` must be [..., n_sections, 6], got {tuple(sr.shape)}")
    if sr.shape[-2] == 0:
        raise ValueError(f"{fn}: `sos` has no sections")


def sosfilt_zi(sos):
    """cplx.sosfilt_zi (which documents it)"""
    fn = "sosfilt_zi"
    (sr, si), = _operands(fn, (("sos", sos),)).values()
    _check_sos(fn, sr)
    zr, zi = _split(_zi_sos(_normalised_sos(_work(sr), _work(si))))
    back = lambda t: None if t is None else t.to(sr.dtype)                    # noqa: E731
    return _wrap(back(zr), back(zi))


# ---- one pass ------------------------------------------------------------------------------------------------------------------
def _call(xr, xi, cr, ci, zr, zi, yr, yi, fr, fi, runs, n, edge, mode, y_lo, y_n, x_es, order, sections, segs, seg_len, flags,
          cx, in_dtype, out_dtype):
    d = _lib.FiltFiltDesc(n=n, edge=edge, y_lo=y_lo, y_n=y_n, order=order, sections=sections, segments=segs, seg_len=seg_len,
                          x_es=x_es, flags=flags, mode=mode, reserved=0)
    fill(d, runs, ("x_stride", "c_stride", "z_stride", "y_stride"))
    call("cplxamd_filtfilt_pass", ptr(xr), ptr(xi), ptr(cr), ptr(ci), ptr(zr), ptr(zi), ptr(yr), ptr(yi), ptr(fr), ptr(fi),
         ctypes.byref(d), int(cx), code(in_dtype), code(out_dtype), stream_ptr())


def _first(xr, xi, n, edge, mode, reverse, ct):
    """the first logical sample in processing order, [*B] planes in the compute type: state-sized torch, the kernel's map"""
    j, k = src_index(n + 2 * edge - 1 if reverse else 0, n, edge, mode)

    def one(p):
        if p is None:
            return None
        at = lambda i: p[..., i].to(ct)                   # noqa: E731
        return at(j) if k < 0 else (at(k) if j < 0 else 2 * at(k) - at(j))
    return one(xr), one(xi)


def run_pass(xr, xi, cr, ci, ur, ui, edge, mode, y_lo, y_n, reverse, cx, out_dtype, force_segments=None):
    """One extended pass, without autograd: x [*B, N] planes (views welcome; xi may be None), the cascade c
    [*Bc, S, 2 (D + 1)] and its unit state u [*Bc, S, D] in the compute type, dense, with as many dims as x and Bc
    broadcastable to B -> (yr, yi): the logical samples [y_lo, y_lo + y_n) of the recurrence over the row extended by
    `edge` (in reverse time if `reverse`), from the state u * (first sample processed), as dense planes of `out_dtype`."""
    batch, n = tuple(xr.shape[:-1]), xr.shape[-1]
    S, W = cr.shape[-2], cr.shape[-1]
    D = W // 2 - 1
    ct, dev, in_dtype = cr.dtype, xr.device, xr.dtype
    yr = torch.empty(batch + (y_n,), dtype=out_dtype, device=dev)
    yi = torch.empty_like(yr) if cx else None
    # copies: x, then c and u expanded
    ((xr, xi), (cr, ci), (ur, ui)), runs = fit(batch + (n,), [(xr, xi), (cr, ci), (ur, ui)], dense(batch + (y_n,)),
                                               [(0,), (1, 2)])
    rev = _lib.FILTFILT_REVERSE if reverse else 0
    es = xr.stride(-1)

    def launch(x, z, y, f, runs, n, segs, seg_len):
        # the transition (null input) runs on the bare segment in the compute type; without y the window is a placeholder
        bare = x[0] is None
        lo, cnt = (0, 1) if y[0] is None else (y_lo, y_n)
        _call(*x, cr, ci, *z, *y, *f, runs, n, 0 if bare else edge, mode, lo, cnt, 0 if bare else es, D, S, segs, seg_len, rev,
              cx, ct if bare else in_dtype, ct if bare else out_dtype)

    def enter():                                          # the scaled state enters the scan as the row's initial state
        fr, fi = _first(xr, xi, n, edge, mode, reverse, ct)
        full = lambda t: None if t is None else t.expand(batch + (S, D))          # noqa: E731
        grow = lambda t: None if t is None else t[..., None, None]                # noqa: E731
        s_r, s_i = _cmul(full(ur), full(ui), grow(fr), grow(fi))
        flat = lambda t: None if t is None else t.expand(batch + (S, D)).reshape(-1, S * D).contiguous()   # noqa: E731
        return flat(s_r), flat(s_i) if cx else None

    if _iir.split(launch, call, lambda r, k: plan(n, edge, D, S, r, k, in_dtype, cx, force_segments), enter, (xr, xi), (yr, yi),
                  runs, n, S, D, cx, ct, False) is None:
        _call(xr, xi, cr, ci, ur, ui, yr, yi, None, None, runs, n, edge, mode, y_lo, y_n, es, D, S, 1, n + 2 * edge,
              rev | _lib.FILTFILT_SCALE, cx, in_dtype, out_dtype)
    return yr, yi


def _two_pass(xr, xi, cr, ci, ur, ui, edge, mode, cx):
    """zero-phase filtering of x [*B, N] planes by the cascade c / unit state u (compute type): two passes, one workspace"""
    n = xr.shape[-1]
    ct = cr.dtype
    wr, wi = run_pass(xr, xi, cr, ci, ur, ui, edge, mode, 0, n + 2 * edge, False, cx, ct)
    return run_pass(wr, wi, cr, ci, ur, ui, 0, mode, edge, n, True, cx, xr.dtype)


# ---- the composed routes (not the hot path) ----------------------------------------------------------------------------------
def _extend(p, e, padtype):
    """a plane [*B, N] extended by e samples on each side, with torch: differentiable"""
    if p is None or e == 0:
        return p
    n = p.shape[-1]
    if padtype == "constant":
        left, right = p[..., :1].expand(p.shape[:-1] + (e,)), p[..., n - 1:].expand(p.shape[:-1] + (e,))
    else:
        left, right = p[..., 1:e + 1].flip(-1), p[..., n - 1 - e:n - 1].flip(-1)
        if padtype == "odd":
            left, right = 2 * p[..., :1] - left, 2 * p[..., n - 1:] - right
    return torch.cat([left, p, right], -1)


def _times_first(zi, pr, pi, state_dims):
    """zi_unit [*Bc, *state] times x[..., 0] of the planes [*B, N] -> planes [*B', *state]"""
    from .cplx import Cplx
    zr, zim = (zi.real, zi.imag) if isinstance(zi, Cplx) else (zi, None)
    pick = lambda p: None if p is None else p[..., :1][(...,) + (None,) * (state_dims - 1)]   # noqa: E731
    return _cmul(zr, zim, pick(pr), pick(pi))


def _composed(step, zi_unit, xr, xi, edge, padtype, state_dims):
    """extension -> step(signal, zi) -> flip -> step -> flip -> trim, on differentiable pieces; `step` is cplx.lfilter or
    cplx.sosfilt with the filter bound, zi_unit None for a filter without state"""
    n = xr.shape[-1]
    er, ei = _extend(xr, edge, padtype), _extend(xi, edge, padtype)

    def once(pr, pi):
        from .cplx import Cplx
        if zi_unit is None:
            y = step(_wrap(pr, pi), None)
        else:
            y, _ = step(_wrap(pr, pi), _wrap(*_times_first(zi_unit, pr, pi, state_dims)))
        return (y.real, y.imag) if isinstance(y, Cplx) else (y, None)

    yr, yi = once(er, ei)
    yr, yi = once(yr.flip(-1), None if yi is None else yi.flip(-1))
    cut = lambda p: None if p is None else p.flip(-1)[..., edge:edge + n]     # noqa: E731
    return _wrap(cut(yr), cut(yi))


# ---- the public functions -----------------------------------------------------------------------------------------------------
def _edge(fn, padtype, padlen, default, n):
    if padtype not in PADTYPES:
        raise ValueError(f"{fn}: unknown padtype {padtype!r}: padtype must be 'even', 'odd', 'constant', or None")
    if padlen is not None and (int(padlen) != padlen or padlen < 0):
        raise ValueError(f"{fn}: padlen must be a non-negative integer, got {padlen}")
    edge = 0 if padtype is None else (default if padlen is None else int(padlen))
    if 0 < n <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    return edge


def _empty(batch, n, xr, cx):
    yr = torch.empty(batch + (n,), dtype=xr.dtype, device=xr.device)
    return _wrap(yr, torch.empty_like(yr) if cx else None)


def filtfilt(b, a, x, padtype="odd", padlen=None):
    """cplx.filtfilt (which documents it)"""
    from . import cplx as _cplx
    fn = "filtfilt"
    ops = _operands(fn, (("b", b), ("a", a), ("x", x)))
    (br, bi), (ar, ai), (xr, xi) = ops["b"], ops["a"], ops["x"]
    nb, na, n = br.shape[-1], ar.shape[-1], xr.shape[-1]
    if nb == 0 or na == 0:
        raise ValueError(f"{fn}: the last dim of `{'b' if nb == 0 else 'a'}` is empty")
    edge = _edge(fn, padtype, padlen, 3 * max(na, nb), n)
    D = max(na, nb) - 1
    if na - 1 > MAX_ORDER:
        raise CplxAmdError(f"{fn}: a denominator of order {na - 1} exceeds the direct form's {MAX_ORDER}: direct forms of that "
                           "order are not sound in float32 -- factor the filter into second-order sections and use "
                           "cplx.sosfiltfilt")
    batch = tuple(torch.broadcast_shapes(xr.shape[:-1], br.shape[:-1], ar.shape[:-1]))
    require_device(xr, xi, br, bi, ar, ai)
    cx = any(t is not None for t in (xi, bi, ai))
    if n == 0 or 0 in batch:
        return _empty(batch, n, xr, cx)
    if _needs_grad(xr, xi, br, bi, ar, ai) or D == 0 or nb - 1 > MAX_ORDER:
        step = lambda s, z: _cplx.lfilter(b, a, s) if z is None else _cplx.lfilter(b, a, s, z)   # noqa: E731
        return _composed(step, None if D == 0 else lfilter_zi(b, a), xr, xi, edge, padtype, 1)
    nd = len(batch)
    ct = _ct(xr.dtype)
    to = lambda t: None if t is None else t.to(ct)        # noqa: E731
    bb, aa = _padded_ba(to(br), to(bi), to(ar), to(ai))
    ur, ui = _split(_zi_direct(bb, aa))
    cr, ci = _split(torch.cat([bb, aa], -1))
    three = lambda t: None if t is None else _lead(t, nd, 1).unsqueeze(-2).contiguous()   # noqa: E731
    xr, xi = xr.expand(batch + (n,)), None if xi is None else xi.expand(batch + (n,))
    mode = _lib.FILTFILT_MODES["odd" if padtype is None else padtype]
    return _wrap(*_two_pass(xr, xi, three(cr), three(ci), three(ur), three(ui), edge, mode, cx))


def sosfiltfilt(sos, x, padtype="odd", padlen=None):
    """cplx.sosfiltfilt (which documents it)"""
    from . import cplx as _cplx
    fn = "sosfiltfilt"
    ops = _operands(fn, (("sos", sos), ("x", x)))
    (sr, si), (xr, xi) = ops["sos"], ops["x"]
    _check_sos(fn, sr)
    S, n = sr.shape[-2], xr.shape[-1]
    edge = _edge(fn, padtype, padlen, 3 * (2 * S + 1), n)
    batch = tuple(torch.broadcast_shapes(xr.shape[:-1], sr.shape[:-2]))
    require_device(xr, xi, sr, si)
    cx = any(t is not None for t in (xi, si))
    if n == 0 or 0 in batch:
        return _empty(batch, n, xr, cx)
    if _needs_grad(xr, xi, sr, si) or S > MAX_SECTIONS:
        step = lambda s, z: _cplx.sosfilt(sos, s) if z is None else _cplx.sosfilt(sos, s, z)     # noqa: E731
        return _composed(step, sosfilt_zi(sos), xr, xi, edge, padtype, 2)
    nd = len(batch)
    ct = _ct(xr.dtype)
    to = lambda t: None if t is None else t.to(ct)        # noqa: E731
    c = _normalised_sos(to(sr), to(si))
    ur, ui = _split(_zi_sos(c))
    cr, ci = _split(c)
    lead = lambda t: None if t is None else _lead(t, nd, 2).contiguous()      # noqa: E731
    xr, xi = xr.expand(batch + (n,)), None if xi is None else xi.expand(batch + (n,))
    mode = _lib.FILTFILT_MODES["odd" if padtype is None else padtype]
    return _wrap(*_two_pass(xr, xi, lead(cr), lead(ci), lead(ur), lead(ui), edge, mode, cx))
