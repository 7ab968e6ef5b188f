"""cplx.ssm_scan on the GPU (csrc/ssm.hip) against the plain float64 loop of tests/ssm_cases.py on the CPU, computed from
the planes as the kernel received them (torch autograd through the loop for the gradients).  L, the tile and the group
are read from ssm.plan.  Rows are [2, 3]; `shared`: b and c are [2, 1, N, T], expanded over the 3 by stride 0.  The
errors this file prints: profiles/ssm_parity.txt.

Bounds, the scan's own (tests/test_gpu_scan.py): float32 |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|; bf16 y, hT, dx and dh0
|got - ref| <= 2^-8 max|ref| (one rounding at 2^-9, doubled); bf16 da, db, dc, ddt 2^-7 max|ref| (products with operands
that are rounded already: two roundings, doubled).  The kernel holds them, so none was widened: measured, the `dt`
form's float32 y is at 0.12 to 0.97 of its bound where the float32 loop on the CPU (reference against reference, printed
beside it) is at 0.06 to 0.14."""
import functools
import math

import pytest
import torch

from gpu_util import DEV
from scan_cases import z
from ssm_cases import loop

from cplxmodule_amd import Cplx, cplx, ssm

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
L, TILE = (ssm.plan(5003, 16)[k] for k in ("chunk", "tile"))
SIZES = [1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
NMAX = 17


def states(cx, vary):
    G = ssm.plan(5003, 16, cplx=cx, time_varying=vary)["group"]
    return sorted({1, G - 1, G, G + 1, NMAX})


def dev(t, dtype, cx=True, over=None):
    """planes [2, ...] on the CPU -> a Cplx (or the real plane alone) on the device, expanded to `over` by stride 0"""
    if t is None:
        return None
    pr, pi = (p.to(dtype).to(DEV) if over is None else p.to(dtype).to(DEV).expand(over) for p in t[:2])
    return Cplx(pr, pi) if cx else pr


def zz(t, cx=True):
    return None if t is None else z(t[0], t[1] if cx else None)


def first(t, n):
    """the first n states of planes [2, ..., N, T]"""
    return None if t is None else t[..., :n, :]


@functools.lru_cache(maxsize=8)
def exact_case(T, cx, vary, shared, with_h0, reverse):
    """integer planes for NMAX states: a in {1, -1, i, -i} (real: {1, -1}) with about one zero in 50, the rest Gaussian
    integers -> (a, b, c, x, h0, the loop's h [2, 3, NMAX, T]).  Every order of summation stays below 2^24."""
    g = torch.Generator().manual_seed(T)
    ta, rows = (T if vary else 1), ((2, 1) if shared else (2, 3))
    k = torch.randint(0, 4 if cx else 2, (2, 3, NMAX, ta), generator=g)
    a = torch.stack([torch.tensor([1., -1, 0, 0])[k], torch.tensor([0., 0, 1, -1])[k]]) * (torch.rand(k.shape, generator=g) >= 0.02)
    small = lambda *s: torch.randint(-2, 3, (2, *s), generator=g).float()        # noqa: E731
    b, c, x = small(*rows, NMAX, ta), small(*rows, NMAX, ta), small(2, 3, T)
    h0 = small(2, 3, NMAX) if with_h0 else None
    h = loop(zz(a, cx), zz(b, cx), zz(c, cx), zz(x, cx), None, zz(h0, cx), reverse)[2]
    assert (zz(c, cx).abs() * h.abs()).sum(-2).max() < 2 ** 24
    return a, b, c, x, h0, h


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("vary", [True, False])
@pytest.mark.parametrize("cx", [True, False])
def test_exact(cx, vary, shared, reverse, with_h0):
    for T, N, dtype in ((T, N, dt) for T in SIZES for N in states(cx, vary) for dt in (F32, BF16)):
        a, b, c, x, h0, h = exact_case(T, cx, vary, shared, with_h0, reverse)
        ref = ((zz(c, cx) * h)[..., :N, :].sum(-2), h[..., :N, 0 if reverse else -1])
        bc = lambda t: dev(first(t, N), dtype, cx, (2, 3, N, t.shape[-1]))       # noqa: E731
        got = cplx.ssm_scan(dev(first(a, N), dtype, cx), bc(b), bc(c), dev(x, dtype, cx),
                            h0=None if h0 is None else dev(h0[..., :N], dtype, cx), return_state=True, reverse=reverse)
        for o, w in zip(got, ref):
            for p, q in zip((o.real, o.imag) if cx else (o,), (w.real, w.imag) if cx else (w,)):
                # (bf16: the reference's one round-to-nearest-even)
                assert p.dtype == dtype and torch.equal(p.cpu(), q.float().to(dtype)), (T, N, dtype)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cx", [True, False])
def test_a_block_continues_from_the_state_of_the_block_before(cx, reverse):
    T, T1, N = 2 * TILE + 5, TILE + 7, 5
    a, b, c, x, h0, _ = exact_case(T, cx, True, True, True, reverse)
    cut = lambda t, lo, hi: dev(first(t, N)[..., lo:hi], F32, cx)                # noqa: E731
    run = lambda lo, hi, h: cplx.ssm_scan(cut(a, lo, hi), cut(b, lo, hi), cut(c, lo, hi), dev(x[..., lo:hi], F32, cx),  # noqa: E731
                                          h0=h, return_state=True, reverse=reverse)
    whole, state = run(0, T, dev(h0[..., :N], F32, cx))
    (lo1, hi1), (lo2, hi2) = ((T1, T), (0, T1)) if reverse else ((0, T1), (T1, T))
    y1, mid = run(lo1, hi1, dev(h0[..., :N], F32, cx))
    y2, end = run(lo2, hi2, mid)
    parts = lambda o: (o.real, o.imag) if cx else (o,)                           # noqa: E731
    for p, q1, q2, s, e in zip(parts(whole), parts(y1), parts(y2), parts(state), parts(end)):
        assert torch.equal(p, torch.cat([q2, q1] if reverse else [q1, q2], -1)) and torch.equal(s, e)


def close(got, ref, what, dtype, loose=False):
    top = ref.abs().max()
    bound = 1e-5 * ref.abs() + 1e-5 * top if dtype == F32 else 2.0 ** (-7 if loose else -8) * top
    err = ((got.detach().double().cpu() - ref).abs() / bound).max().item()
    print(what, str(dtype)[6:], "error / bound", err)
    assert got.shape == ref.shape and err <= 1.0, (what, err)


@functools.lru_cache(maxsize=None)
def smooth_case(T, N, dtype, shared, with_dt):
    """planes rounded to dtype: a = poles with Re in [-1, -0.01], Im in [-pi, pi] and dt in [1e-3, 1e-1], or without
    `dt` a[n, t] = r e^{i theta}, r in [0.8, 1); b, c, x, h0 normal -> the leaves, the upstream (g, gf), the float64 (y, hT)
    and the gradients of Re <g, y> + Re <gf, hT> by autograd through the loop"""
    g = torch.Generator().manual_seed(T + N)
    rows = (2, 1) if shared else (2, 3)
    if with_dt:
        a = torch.stack([-0.01 - 0.99 * torch.rand(3, N, 1, generator=g), math.pi * (2 * torch.rand(3, N, 1, generator=g) - 1)])
        dt = 1e-3 + (1e-1 - 1e-3) * torch.rand(2, 3, T, generator=g)
    else:
        r, th = 0.8 + 0.2 * torch.rand(2, 3, N, T, generator=g), 2 * math.pi * torch.rand(2, 3, N, T, generator=g)
        a, dt = torch.stack([r * th.cos(), r * th.sin()]), None
    n = lambda *s: torch.randn(2, *s, generator=g)                               # noqa: E731
    pl = [t.to(dtype) for t in (a, n(*rows, N, T), n(*rows, N, T), n(2, 3, T), n(2, 3, N))] + ([dt.to(dtype)] if with_dt else [])
    up = [n(2, 3, T).to(dtype), n(2, 3, N).to(dtype)]
    leaves = [t.double().requires_grad_() for t in pl]
    cz = [torch.complex(t[0], t[1]) for t in leaves[:5]]
    y, hT, _ = loop(*cz[:4], leaves[5] if with_dt else None, cz[4])
    loss = sum((o.real * u[0].double()).sum() + (o.imag * u[1].double()).sum() for o, u in zip((y, hT), up))
    return pl, up, y.detach(), hT.detach(), torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("T,N", [(TILE + 1, 5), (TILE + 1, 16), (2 * TILE + 5, 5), (2 * TILE + 5, 16)])
def test_close_dt_form(T, N, dtype):
    pl, _, y, hT, _ = smooth_case(T, N, dtype, True, True)
    a, x, h0 = (dev(pl[k], dtype) for k in (0, 3, 4))
    got, state = cplx.ssm_scan(a, dev(pl[1], dtype, over=(2, 3, N, T)), dev(pl[2], dtype, over=(2, 3, N, T)), x,
                               dt=pl[5].to(DEV), h0=h0, return_state=True)
    # reference against reference: the same loop in float32 on the CPU
    f32 = loop(*(torch.complex(t[0].float(), t[1].float()) for t in pl[:4]), pl[5].float(), torch.complex(*pl[4].float()))[0]
    print(f"T={T} N={N} float32 loop against float64 loop, error / float32 bound",
          ((f32.to(y.dtype) - y).abs() / (1e-5 * y.abs() + 1e-5 * y.abs().max())).max().item())
    for name, o, ref in (("y", got, y), ("hT", state, hT)):
        close(o.real, ref.real, f"dt form T={T} N={N} {name}_r", dtype)
        close(o.imag, ref.imag, f"dt form T={T} N={N} {name}_i", dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("with_dt", [False, True])
@pytest.mark.parametrize("shared", [True, False])
def test_gradients(shared, with_dt, dtype):
    T, N = TILE + 1, 5
    pl, up, y, hT, grads = smooth_case(T, N, dtype, shared, with_dt)
    lv = [t.to(DEV).requires_grad_() for t in pl]
    over = lambda t: Cplx(t[0].expand(2, 3, N, T), t[1].expand(2, 3, N, T))      # noqa: E731
    a, x, h0 = (Cplx(lv[k][0], lv[k][1]) for k in (0, 3, 4))
    got, state = cplx.ssm_scan(a, over(lv[1]), over(lv[2]), x, dt=lv[5] if with_dt else None, h0=h0, return_state=True)
    close(got.real, y.real, "y_r", dtype)
    outs = torch.autograd.grad([got.real, got.imag, state.real, state.imag], lv, [u.to(DEV) for u in (*up[0], *up[1])])
    for name, o, ref in zip(("da", "db", "dc", "dx", "dh0", "ddt"), outs, grads):
        close(o, ref, f"shared={shared} dt={with_dt} {name}", dtype, loose=name not in ("dx", "dh0"))


def test_layouts_and_the_memory_of_the_forward():
    """(integer operands: a view and its dense twin agree bit for bit only where every order of composition is exact)"""
    T, N = TILE + 1, 5
    a, b, c, x, h0, _ = exact_case(2 * TILE + 5, True, True, False, True, False)
    a, b, c, x = *(dev(first(t, N), F32) for t in (a, b, c)), dev(x, F32)
    dense = lambda t: Cplx(t.real.contiguous(), t.imag.contiguous())             # noqa: E731
    tr = lambda t: Cplx(t.real.transpose(0, 1), t.imag.transpose(0, 1))          # noqa: E731
    sl = lambda t, s: Cplx(t.real[s], t.imag[s])                                 # noqa: E731
    keep, step = (Ellipsis, slice(0, T)), (Ellipsis, slice(0, 2 * T, 2))
    wide = sl(a, (slice(0, 1),) + keep)
    views = {"step-sliced x": (sl(a, keep), sl(b, keep), sl(c, keep), sl(x, step)),
             "expanded a": (Cplx(wide.real.expand(2, 3, N, T), wide.imag.expand(2, 3, N, T)), sl(b, keep), sl(c, keep), sl(x, keep)),
             "transposed leading pair": tuple(tr(sl(t, keep)) for t in (a, b, c, x))}
    for name, ops in views.items():
        got = cplx.ssm_scan(*ops, return_state=True)
        twin = cplx.ssm_scan(*(dense(t) for t in ops), return_state=True)
        for o, w in zip(got, twin):
            assert torch.equal(o.real, w.real) and torch.equal(o.imag, w.imag) and o.real.is_contiguous(), name
    # b and c shared by the 8 channels of a batch entry: the forward allocates y and hT, never an [2, 8, N, T] tensor
    B, D, N = 2, 8, 16
    big = [torch.randn(s, device=DEV) for s in ((D, N, 1), (B, 1, N, T), (B, 1, N, T), (B, D, T), (B, D, T))]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ex = lambda t: t.expand(B, D, N, T)                                          # noqa: E731
    dt = 0.01 * big[4].abs()
    before = torch.cuda.max_memory_allocated()
    cplx.ssm_scan(Cplx(-big[0].abs(), big[0]), Cplx(ex(big[1]), ex(big[2])), Cplx(ex(big[2]), ex(big[1])), big[3], dt=dt)
    assert torch.cuda.max_memory_allocated() - before < B * D * N * T * 4
