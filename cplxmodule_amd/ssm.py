"""The diagonal state-space scan with N states per channel, along the last dim, on the fused kernels of csrc/ssm.hip and
csrc/ssm_grad.hip: the argument handling, the plans, the launch glue and the autograd Function behind cplx.ssm_scan, and
the composed route (`composed`: torch products and cplx.linear_recurrence) that float64 takes and scripts/bench_ssm.py
compares against.

One primitive (cplxamd_ssm_scan).  In processing order p = 0 .. T - 1 (step p is sample p, or T - 1 - p in reverse)

    h[n, p] = A[n, p] h[n, p - 1] + b[n, p] X[p],   y[p] = sum_n c[n, p] h[n, p],   h[n, -1] = h0[n] (or zero)

with A = a (one value per state, or one per step) and X = x, or A[n, p] = exp(dt[p] a[n]) and X = dt x, formed in
registers.  Four flags: `reverse`; `conj` conjugates a, b and c; `lag` takes the coefficient (and its dt) of step p - 1,
and h0 enters step 0 unscaled; `dt_out` moves the factor dt from x to y.  With autograd's convention (dL/dre + i dL/dim),
incoming gradients g of y and gf of the final state:

    lambda[n, t] = conj(c[n, t]) g[t] + conj(A[n, t + 1]) lambda[n, t + 1],   lambda[n, T] "=" gf[n] unscaled
    dx[t] = dt[t] sum_n conj(b[n, t]) lambda[n, t]      -- the primitive on (a, c, b, g, dt, gf), all four flags flipped
    dh0[n] = conj(A[n, 0]) lambda[n, 0]                 -- lambda[., 0] is that call's final state

so dx and dh0 cost one launch of the same kernel and nothing of size N T.  When a, b, c or dt require grad the backward is
instead ONE launch of the parameter-gradient kernel (csrc/ssm_grad.hip: `run_grad`, `grad_plan`), which recomputes h and
lambda in registers and writes dx, lambda[., 0] and

    dc = g conj(h),  db = lambda conj(X),  dA = lambda conj(h[p - 1]);   with dt:  da[n] = sum_t dA conj(dt A),
    ddt[t] = Re sum_n dA conj(a A) + Re(conj(x[t]) dX[t])

per row of the batch in float32: [*B, N, T] where the operand varies along time, [*B, N, 1] (summed on chip) where it has
one value per state.  The rows that share an operand are summed with sum_to_size and rounded once.  `parameter_gradients`
states the same formulas with torch products on [*B, N, T] tensors; tests/test_ssm_host.py checks it against autograd and
nothing else calls it.  The backward is not differentiable: second derivatives are `composed`'s.

Leading dims broadcast by torch's rules and are read where they lie (stride 0 included) under _runs.py's rule of three
batch runs, otherwise one copy.  Time must have stride 1 (or 0 in a, b, c): an operand whose time dim is strided is
copied once; there is no column plan.  Nothing reads a device value on the host: calls can be captured in a hipGraph.
"""
import ctypes

import torch

from . import _lib, scan
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import MAX_RUNS, code, dense, fill, fit
from .iir import _cmul, _ct, _operands, _wrap
from .ops import once_differentiable

FN = "ssm_scan"
N_MAX = 256


def plan(T, N, rows=1, dtype=torch.float32, cplx=True, time_varying=True):
    """The plan for `rows` rows of `T` steps and `N` states -- a pure host call, no GPU needed.  `time_varying`: the
    coefficient varies along time (`a` [..., N, T], or the `dt` form).  -> dict of _lib.SSM_PLAN_FIELDS: chunk (the L
    steps a thread keeps in registers), tile, tiles, group (the states per barrier), LDS bytes, threads, grid, window
    (the consecutive coefficients whose product the kernel forms)."""
    out = (ctypes.c_int64 * len(_lib.SSM_PLAN_FIELDS))()
    kind = code(dtype)
    rc = _lib.load().cplxamd_ssm_plan(int(T), int(N), int(rows), kind, int(bool(cplx)), int(bool(time_varying)), out)
    if rc == -3:
        raise CplxAmdError(f"{FN}: {rows} rows of {T} steps exceed what the kernel indexes (2^40 steps, 2^31 - 1 rows)")
    if rc < 0:
        raise CplxAmdError(f"{FN}: no plan for N = {N} states (1 .. {N_MAX}) in {dtype} (float32 or bfloat16)")
    return dict(zip(_lib.SSM_PLAN_FIELDS, out))


def _timed(p):
    """planes [..., N, T or 1] whose time dim the kernel can step along: stride 1, or one value"""
    if p[0] is None or p[0].shape[-1] == 1 or p[0].stride(-1) in (0, 1):
        return p
    return tuple(None if t is None else t.contiguous() for t in p)


def run(a, b, c, x, dt, h0, reverse=False, conj=False, lag=False, dt_out=False, cx=None, want_state=True):
    """The module-level primitive, without autograd, on plane pairs (re, im or None): a, b, c [*B, N, T or 1], x [*B, T],
    dt [*B, T] or None, h0 [*B, N] or (None, None); views welcome, stride 0 along any leading dim
    -> (yr, yi, fr, fi): y [*B, T] in the operands' dtype and the final state [*B, N] (None without `want_state`) in
    float32, not rounded: the backward multiplies it; both dense; the imaginary planes are None when every operand is
    real (`cx` False)."""
    xr = x[0]
    batch, T, N, dtype, dev = tuple(xr.shape[:-1]), xr.shape[-1], a[0].shape[-2], xr.dtype, xr.device
    if cx is None:
        cx = any(p[1] is not None for p in (a, b, c, x, h0))
    dense1 = lambda t: t if t is None or T == 1 or t.stride(-1) == 1 else t.contiguous()      # noqa: E731
    x, dt = (dense1(x[0]), dense1(x[1])), dense1(dt)
    h0 = tuple(None if t is None else t.float() for t in h0)                  # the state planes are float32 for the kernel
    yr = torch.empty(batch + (T,), dtype=dtype, device=dev)
    fr = torch.empty(batch + (N,), dtype=torch.float32, device=dev) if want_state else None
    named = [("a", _timed(a)), ("b", _timed(b)), ("c", _timed(c)), ("x", x)] + [("dt", (dt, None))] * (dt is not None)
    named += [("h", h0)] * (h0[0] is not None) + [("f", (fr, None))] * want_state
    free = [(k,) for k, (name, _) in enumerate(named) if name != "f"]
    ops, rr = fit(batch + (T,), [p for _, p in named], dense(batch + (T,)), sorted(free, key=lambda k: named[k[0]][0] != "x"))
    if len(rr) > MAX_RUNS:
        raise CplxAmdError(f"{FN}: the batch dims do not fit {MAX_RUNS} runs")       # (every operand was copied: not reached)
    got = {name: p for (name, _), p in zip(named, ops)}
    (ar, ai), (br, bi), (cr, ci), (xr, xi) = got["a"], got["b"], got["c"], got["x"]
    dt, (hr, hi) = got.get("dt", (None, None))[0], got.get("h", (None, None))
    es = lambda t: 0 if t.shape[-1] == 1 else t.stride(-1)    # noqa: E731
    flags = ((_lib.SSM_REVERSE if reverse else 0) | (_lib.SSM_CONJ if conj else 0) | (_lib.SSM_LAG if lag else 0)
             | (_lib.SSM_DT_OUT if dt_out else 0))
    d = _lib.SsmDesc(n=T, states=N, a_es=es(ar), b_es=es(br), c_es=es(cr), a_ns=ar.stride(-2), b_ns=br.stride(-2),
                     c_ns=cr.stride(-2), h_ns=0 if hr is None else hr.stride(-1), f_ns=1, flags=flags)
    fill(d, rr, [name + "_stride" for name, _ in named] + ["y_stride"])
    yi = torch.empty_like(yr) if cx else None
    fi = torch.empty_like(fr) if cx and want_state else None
    keep = lambda t: ptr(t) if cx else None                   # noqa: E731
    call("cplxamd_ssm_scan", ptr(ar), keep(ai), ptr(br), keep(bi), ptr(cr), keep(ci), ptr(xr), keep(xi), ptr(dt), ptr(hr),
         keep(hi), ptr(yr), ptr(yi), ptr(fr), ptr(fi), ctypes.byref(d), int(cx), code(dtype), stream_ptr())
    return yr, yi, fr, fi


def grad_plan(T, N, rows=1, dtype=torch.float32, cplx=True, time_varying=True):
    """The plan of the parameter-gradient kernel (csrc/ssm_grad.hip) for `rows` rows of `T` steps and `N` states -- a pure
    host call like `plan`.  -> dict of _lib.SSM_PGRAD_PLAN_FIELDS: chunk, tile, tiles, group (the states per barrier), LDS
    bytes, ws_bytes (the float32 states of h that enter the tiles, [rows, tiles, N], x 2 when complex; 0 for one tile),
    threads, grid."""
    out = (ctypes.c_int64 * len(_lib.SSM_PGRAD_PLAN_FIELDS))()
    if dtype not in (torch.float32, torch.bfloat16):
        raise CplxAmdError(f"{FN}: no gradient plan in {dtype} (float32 or bfloat16; float64 takes ssm.composed)")
    rc = _lib.load().cplxamd_ssm_pgrad_plan(int(T), int(N), int(rows), code(dtype), int(bool(cplx)), int(bool(time_varying)), out)
    if rc == -3:
        raise CplxAmdError(f"{FN}: {rows} rows of {T} steps exceed what the kernel indexes (2^40 steps, 2^31 - 1 rows)")
    if rc < 0:
        raise CplxAmdError(f"{FN}: no gradient plan for N = {N} states (1 .. {N_MAX})")
    return dict(zip(_lib.SSM_PGRAD_PLAN_FIELDS, out))


def run_grad(a, b, c, x, dt, h0, g, gf, reverse=False, cx=None, need=(True, True, True, True, True)):
    """The gradients of the scan in ONE launch (cplxamd_ssm_pgrad), without autograd, on plane pairs laid out as `run`'s,
    with g [*B, T] the gradient of y and gf [*B, N] (or (None, None)) that of the final state; `need` = (a, b, c, dt, x).
    -> ((dxr, dxi), da, db, dc, ddt, (lr, li)): dx in the operands' dtype, everything else float32 and PER ROW of the
    batch: da, db, dc plane pairs [*B, N, T] where the operand varies along time and [*B, N, 1] where it has one value per
    state (summed over time on chip), ddt [*B, T], lambda[., 0] [*B, N]; None where `need` is off (the caller sums over
    the rows that share an operand and rounds).  Nothing of size N T is allocated but a gradient of that shape."""
    xr = x[0]
    batch, T, N, dtype, dev = tuple(xr.shape[:-1]), xr.shape[-1], a[0].shape[-2], xr.dtype, xr.device
    if cx is None:
        cx = any(p[1] is not None for p in (a, b, c, x, h0, g, gf))
    dense1 = lambda t: t if t is None or T == 1 or t.stride(-1) == 1 else t.contiguous()      # noqa: E731
    # (an operand expanded along TIME has a gradient per step: it is copied, the kernel sums what has one value)
    timed = lambda p: tuple(t if t is None or t.shape[-1] == 1 else dense1(t) for t in p)     # noqa: E731
    f32 = lambda p: tuple(None if t is None else t.float() for t in p)                        # noqa: E731
    named = [("a", timed(a)), ("b", timed(b)), ("c", timed(c)), ("x", tuple(dense1(t) for t in x)),
             ("g", tuple(dense1(t) for t in g))] + [("dt", (dense1(dt), None))] * (dt is not None)
    named += [("h", f32(h0))] * (h0[0] is not None) + [("f", f32(gf))] * (gf[0] is not None)
    ops, rr = fit(batch + (T,), [p for _, p in named], dense(batch + (T,)),
                  sorted(((k,) for k in range(len(named))), key=lambda k: named[k[0]][0] != "x"))
    if len(rr) > MAX_RUNS:
        raise CplxAmdError(f"{FN}: the batch dims do not fit {MAX_RUNS} runs")       # (every operand was copied: not reached)
    got = {name: p for (name, _), p in zip(named, ops)}
    none = (None, None)
    (ar, ai), (br, bi), (cr, ci), (xr, xi), (gr, gi) = (got[k] for k in "abcxg")
    dt, (hr, hi), (fr, fi) = got.get("dt", none)[0], got.get("h", none), got.get("f", none)
    es = lambda t: 0 if t.shape[-1] == 1 else t.stride(-1)    # noqa: E731
    wa, wb, wc, wd, wx = (bool(v) for v in need)
    wd = wd and dt is not None
    bits = ((_lib.SSM_NEED_A if wa else 0) | (_lib.SSM_NEED_B if wb else 0) | (_lib.SSM_NEED_C if wc else 0)
            | (_lib.SSM_NEED_DT if wd else 0) | (_lib.SSM_NEED_X if wx else 0))
    d = _lib.SsmGradDesc(n=T, states=N, a_es=es(ar), b_es=es(br), c_es=es(cr), a_ns=ar.stride(-2), b_ns=br.stride(-2),
                         c_ns=cr.stride(-2), h_ns=0 if hr is None else hr.stride(-1), f_ns=0 if fr is None else fr.stride(-1),
                         flags=_lib.SSM_REVERSE if reverse else 0, need=bits)
    rows, _ = fill(d, rr, [name + "_stride" for name, _ in named])
    new = lambda on, tail, kind=torch.float32: (tuple(torch.empty(batch + tail, dtype=kind, device=dev)       # noqa: E731
                                                      if k == 0 or cx else None for k in range(2)) if on else none)
    wide = lambda t: (N, T if es(t) == 1 else 1)              # noqa: E731
    dx, da, db, dc = new(wx, (T,), dtype), new(wa, wide(ar)), new(wb, wide(br)), new(wc, wide(cr))
    ddt, lam = new(wd, (T,))[0], new(True, (N,))
    p = grad_plan(T, N, rows, dtype, cx, dt is not None or es(ar) == 1)
    ws = torch.empty(p["ws_bytes"] // 4, dtype=torch.float32, device=dev) if p["ws_bytes"] else None
    keep = lambda t: t if cx else None                        # noqa: E731
    planes = lambda ts, count: (ctypes.c_void_p * count)(*(None if t is None else ptr(t).value for t in ts))   # noqa: E731
    call("cplxamd_ssm_pgrad",
         planes((ar, keep(ai), br, keep(bi), cr, keep(ci), xr, keep(xi), dt, hr, keep(hi), gr, keep(gi), fr, keep(fi)),
                _lib.SSM_PGRAD_IN),
         planes((*dx, *da, *db, *dc, ddt, *lam, ws), _lib.SSM_PGRAD_OUT), ctypes.byref(d), int(cx), code(dtype), stream_ptr())
    return dx, da, db, dc, ddt, lam


def _over(p, shape):
    return tuple(None if t is None else t.expand(shape) for t in p)


def _z(p, ct, cx):
    """a plane pair in the compute type: one real tensor when nothing of the call is complex, else a complex one"""
    pr, pi = (None if t is None else t.to(ct) for t in p)
    return pr if not cx else torch.complex(pr, torch.zeros_like(pr) if pi is None else pi)


def _recur(a, u, h0, reverse, conj=False, lag=False):
    """scan.run on compute-type tensors: u [*B, N, T], a broadcastable to it, h0 [*B, N] or None"""
    cx = u.is_complex()
    parts = lambda t: (None, None) if t is None else ((t.real, t.imag) if cx else (t, None))      # noqa: E731
    (ar, ai), (ur, ui), (hr, hi) = parts(a.expand(u.shape)), parts(u), parts(h0)
    yr, yi = scan.run(ar, ai, ur, ui, hr, hi, reverse, conj, lag, cx)
    return torch.complex(yr, yi) if cx else yr


def parameter_gradients(a, b, c, x, dt, h0, g, gf, reverse, need, recur=_recur):
    """The gradients of a, b, c and dt (module docstring) on compute-type tensors (all complex, or all real): a, b, c
    [*B, N, T or 1], x, dt, g [*B, T], h0, gf [*B, N] or None; `need` = (a, b, c, dt) -> (da, db, dc, ddt) at the
    broadcast shape [*B, N, T] (dt: [*B, T]) or None; the caller reduces them.  `recur`: the scan primitive."""
    one = lambda t: t.unsqueeze(-2)                           # noqa: E731
    A = a if dt is None else torch.exp(one(dt) * a)
    X = x if dt is None else dt * x
    full = torch.broadcast_shapes(A.shape, b.shape, c.shape, one(X).shape)
    last, T = (0, x.shape[-1]) if reverse else (x.shape[-1] - 1, x.shape[-1])
    v = (c.conj() * one(g)).expand(full).clone()
    if gf is not None:
        v[..., last] += gf
    lam = recur(A, v, None, not reverse, True, True)
    da = db = dc = ddt = None
    if need[0] or need[2] or (need[3] and dt is not None):
        h = recur(A, (b * one(X)).expand(full).contiguous(), h0, reverse)
        if need[2]:
            dc = one(g) * h.conj()
        if need[0] or need[3]:
            first = torch.zeros_like(h[..., :1]) if h0 is None else h0.unsqueeze(-1).expand(full[:-1] + (1,))
            before = torch.cat([h[..., 1:], first], -1) if reverse else torch.cat([first, h[..., :T - 1]], -1)
            dA = lam * before.conj()
            da = dA if dt is None else dA * (one(dt) * A).conj()
            if need[3] and dt is not None:
                ddt = (dA * (a * A).conj()).real.sum(-2)
    if need[1]:
        db = lam * one(X).conj()
    if need[3] and dt is not None:
        ddt = ddt + (x.conj() * (b.conj() * lam).sum(-2)).real
    return da, db, dc, ddt


class _Ssm(torch.autograd.Function):
    """(yr, yi, fr, fi) = the scan of the module docstring.  Every operand arrives with its leading dims aligned to
    `batch` (size 1 where it broadcasts); imaginary planes, dt and h0 may be None.  meta = (reverse, cx, batch, T, N)."""

    @staticmethod
    def forward(ctx, ar, ai, br, bi, cr, ci, xr, xi, dt, hr, hi, meta):
        reverse, cx, batch, T, N = meta
        abc = lambda pr, pi: _over((pr, pi), batch + (N, pr.shape[-1]))                          # noqa: E731
        yr, yi, fr, fi = run(abc(ar, ai), abc(br, bi), abc(cr, ci), _over((xr, xi), batch + (T,)),
                             None if dt is None else dt.expand(batch + (T,)), _over((hr, hi), batch + (N,)), reverse, cx=cx)
        ctx.meta = meta
        ctx.save_for_backward(ar, ai, br, bi, cr, ci, xr, xi, dt, hr, hi)
        return yr, yi, fr.to(xr.dtype), None if fi is None else fi.to(xr.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gr, gi, gfr, gfi):
        ar, ai, br, bi, cr, ci, xr, xi, dt, hr, hi = ctx.saved_tensors
        reverse, cx, batch, T, N = ctx.meta
        need = ctx.needs_input_grad
        abc = lambda pr, pi: _over((pr, pi), batch + (N, pr.shape[-1]))                          # noqa: E731
        dte = None if dt is None else dt.expand(batch + (T,))
        a, b, c = abc(ar, ai), abc(br, bi), abc(cr, ci)
        g, gf = (gr, gi if cx else None), (gfr, gfi if cx else None)
        back = lambda t, like: None if t is None or like is None else t.sum_to_size(like.shape).to(like.dtype)   # noqa: E731
        grads = [None] * 11
        wants = (need[0] or need[1], need[2] or need[3], need[4] or need[5], need[8] and dt is not None)
        if any(wants):
            # every gradient from ONE launch of the parameter-gradient kernel, per row: the rows that share an operand
            # are summed here, in float32, and rounded once
            (dxr, dxi), da, db, dc, ddt, (lr, li) = run_grad(a, b, c, _over((xr, xi), batch + (T,)), dte,
                                                             _over((hr, hi), batch + (N,)), g, gf, reverse, cx,
                                                             wants + (need[6] or need[7],))
            for k, (t, w) in enumerate(((da, wants[0]), (db, wants[1]), (dc, wants[2]))):
                if w:
                    grads[2 * k], grads[2 * k + 1] = back(t[0], ctx.saved_tensors[2 * k]), back(t[1], ctx.saved_tensors[2 * k + 1])
            del da, db, dc
            grads[8] = back(ddt, dt)
        else:
            # dx and lambda[., 0] alone: the scan kernel, b and c swapped, every flag flipped
            dxr, dxi, lr, li = run(a, c, b, g, dte, gf, not reverse, True, True, True, cx)
        grads[6], grads[7] = back(dxr, xr), back(dxi, xi)
        if need[9] or need[10]:
            ct, at = _ct(xr.dtype), T - 1 if reverse else 0
            a0 = _z(tuple(None if t is None else t[..., at if t.shape[-1] > 1 else 0] for t in a), ct, cx)
            lam0 = _z((lr, li), ct, cx)
            if dt is not None:
                a0 = torch.exp(dte[..., at].to(ct).unsqueeze(-1) * a0)
            dh = a0.conj() * lam0
            grads[9], grads[10] = back(dh.real, hr), back(dh.imag if cx else None, hi)
        return tuple(v if need[k] else None for k, v in enumerate(grads)) + (None,)


def _prepare(fn, a, b, c, x, dt, h0):
    """the checks and the broadcast shared by ssm_scan and composed -> (planes with their leading dims aligned to the
    batch shape, dt, batch, T, N, cx)"""
    for name, v in (("a", a), ("b", b), ("c", c), ("x", x)):
        if v is None:
            raise CplxAmdError(f"{fn}: `{name}` is a NoneType, not a Cplx or a real torch.Tensor")
    ops = _operands(fn, (("x", x), ("a", a), ("b", b), ("c", c), ("dt", dt), ("h0", h0)))
    if ops["dt"][1] is not None:
        raise CplxAmdError(f"{fn}: `dt` must be a real tensor, not a Cplx")
    T = ops["x"][0].shape[-1]
    if ops["a"][0].dim() < 2:
        raise ValueError(f"{fn}: `a` must be [..., N, T] or [..., N, 1], got {tuple(ops['a'][0].shape)}")
    N = ops["a"][0].shape[-2]
    if not 1 <= N <= N_MAX:
        raise CplxAmdError(f"{fn}: N = {N} states; the kernel takes 1 .. {N_MAX}")
    for name in ("a", "b", "c"):
        s = tuple(ops[name][0].shape)
        if len(s) < 2 or s[-2] != N or s[-1] not in (1, T):
            raise ValueError(f"{fn}: `{name}` must be [..., {N}, {T}] or [..., {N}, 1], got {s}")
    if dt is not None and ops["a"][0].shape[-1] != 1 and T != 1:
        raise ValueError(f"{fn}: with `dt`, `a` holds the continuous poles and must be [..., {N}, 1]")
    if dt is not None and ops["dt"][0].shape[-1] != T:
        raise ValueError(f"{fn}: `dt` must be [..., {T}], got {tuple(ops['dt'][0].shape)}")
    if h0 is not None and ops["h0"][0].shape[-1] != N:
        raise ValueError(f"{fn}: `h0` must be [..., {N}], got {tuple(ops['h0'][0].shape)}")
    tails = {"x": 1, "dt": 1, "h0": 1, "a": 2, "b": 2, "c": 2}
    batch = tuple(torch.broadcast_shapes(*(p[0].shape[:-tails[k]] for k, p in ops.items() if p[0] is not None)))
    require_device(*(t for p in ops.values() for t in p))
    lead = lambda t, k: None if t is None else t[(None,) * (len(batch) + tails[k] - t.dim())]   # noqa: E731
    ops = {k: (lead(p[0], k), lead(p[1], k)) for k, p in ops.items()}
    cx = any(p[1] is not None for p in ops.values())
    return ops, batch, T, N, cx


def _composed(ops, batch, T, N, cx, reverse):
    (ar, ai), (br, bi), (cr, ci), (xr, xi), dt, (hr, hi) = ops["a"], ops["b"], ops["c"], ops["x"], ops["dt"][0], ops["h0"]
    one = lambda t: None if t is None else t.unsqueeze(-2)    # noqa: E731
    if dt is not None:
        e = torch.exp(one(dt) * ar)
        ar, ai = (e, None) if ai is None else (e * torch.cos(one(dt) * ai), e * torch.sin(one(dt) * ai))
        xr, xi = dt * xr, None if xi is None else dt * xi
    full = batch + (N, T)
    ur, ui = _over(_cmul(br, bi, one(xr), one(xi)), full)
    h = scan.recur(ar, ai, ur, ui, hr, hi, reverse, False, False, cx, full)
    yr, yi = _cmul(cr, ci, *h)
    at = 0 if reverse else T - 1
    return yr.sum(-2), None if yi is None else yi.sum(-2), h[0][..., at], None if h[1] is None else h[1][..., at]


def _empty(ops, batch, T, N, cx, return_state):
    def new(k):
        pr = torch.empty(batch + (k,), dtype=ops["x"][0].dtype, device=ops["x"][0].device)
        return _wrap(pr, torch.empty_like(pr) if cx else None)
    return (new(T), new(N)) if return_state else new(T)


def composed(a, b, c, x, dt=None, h0=None, return_state=False, reverse=False):
    """cplx.ssm_scan spelled with the package's other operations: torch products, `cplx.linear_recurrence`'s Function on
    the [*B, N, T] state, a sum over the states.  Every dtype, differentiable to any order; about ten passes over a
    tensor N times the size of x.  The route of float64 operands, and the baseline of scripts/bench_ssm.py."""
    ops, batch, T, N, cx = _prepare("ssm.composed", a, b, c, x, dt, h0)
    if T == 0 or 0 in batch:
        return _empty(ops, batch, T, N, cx, return_state)
    yr, yi, fr, fi = _composed(ops, batch, T, N, cx, reverse)
    return (_wrap(yr, yi), _wrap(fr, fi)) if return_state else _wrap(yr, yi)


def ssm_scan(a, b, c, x, dt=None, h0=None, return_state=False, reverse=False):
    """cplx.ssm_scan (which documents it)"""
    ops, batch, T, N, cx = _prepare(FN, a, b, c, x, dt, h0)
    if T == 0 or 0 in batch:
        return _empty(ops, batch, T, N, cx, return_state)
    if ops["x"][0].dtype == torch.float64:
        yr, yi, fr, fi = _composed(ops, batch, T, N, cx, reverse)
    else:
        yr, yi, fr, fi = _Ssm.apply(*ops["a"], *ops["b"], *ops["c"], *ops["x"], ops["dt"][0], *ops["h0"],
                                    (bool(reverse), cx, batch, T, N))
    return (_wrap(yr, yi), _wrap(fr, fi)) if return_state else _wrap(yr, yi)
