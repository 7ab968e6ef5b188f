"""cplx.linear_recurrence, cumsum and cumprod on the GPU (csrc/scan.hip) against the plain float64 loop of
tests/scan_cases.py on the CPU, computed from the planes as the kernel received them (torch autograd through the loop for
the gradients).  L, the tiles and the seams are read from scan.plan.  The errors this file prints:
profiles/scan_parity.txt.

Bounds: float32 |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|; bf16 h and dx |got - ref| <= 2^-8 max|ref| (one rounding at
2^-9, doubled), bf16 da and dh0 2^-7 max|ref| (a product with the saved, already rounded h: two roundings, doubled).
Data is laid out once as [2, D, T]; the row layout reads it densely, the column layout as a [2, T, D] tensor transposed."""
import functools
import math

import pytest
import torch

from gpu_util import DEV
from scan_cases import reference, z

from cplxmodule_amd import Cplx, cplx, scan

pytestmark = pytest.mark.gpu

ROW, COL = scan.plan(5003, 300), scan.plan(5003, 100, 130)
F32, BF16 = torch.float32, torch.bfloat16


def sizes(p):
    L, tile = p["chunk"], p["tile"]
    return sorted({1, 2, L - 1, L, L + 1, tile - 1, tile, tile + 1, 3 * tile + 5, 5003})


def lay(t, lanes, D=None):
    """[2, Dmax, T] on the CPU -> the device tensor of the first D channels in the layout under test"""
    t = t if D is None else t[:, :D]
    return t.to(DEV) if lanes == "row" else t.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)


def pair(t, cx):
    return Cplx(t[0], t[1]) if cx else t[0]


def integers(T, cx, g, lead=(2, 130)):
    """planes [2, *lead, T]: a in {1, -1, i, -i} (real: {1, -1}) with about one reset (a = 0) in 50; x Gaussian integers"""
    k = torch.randint(0, 4 if cx else 2, (*lead, T), generator=g)
    a = torch.stack([torch.tensor([1., -1, 0, 0])[k], torch.tensor([0., 0, 1, -1])[k]])
    return a * (torch.rand(*lead, T, generator=g) >= 0.02), torch.randint(-3, 4, (2, *lead, T), generator=g).float()


@functools.lru_cache(maxsize=16)
def exact_case(T, cx, reverse, with_h0):
    """-> (a, x, h0 planes [2 planes, 2, 130, ...], the loop's h: integers below 2^24, kept as float32)"""
    g = torch.Generator().manual_seed(T)
    a, x = integers(T, cx, g)
    h0 = torch.randint(-3, 4, (2, 2, 130), generator=g).float() if with_h0 else None
    zz = lambda t: None if t is None else z(t[0], t[1] if cx else None)      # noqa: E731
    h = reference(zz(a), zz(x), zz(h0), reverse)
    return a, x, h0, h.to(torch.complex64 if cx else torch.float32)


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cx", [True, False])
@pytest.mark.parametrize("lanes", ["row", "column"])
def test_exact(lanes, cx, reverse, with_h0, monkeypatch):
    cases = [(T, 0) for T in sizes(ROW if lanes == "row" else COL)] + [(5003, f) for f in (2, 3, 7)]
    for (T, force), D, dtype in ((c, D, dt) for c in cases for D in ((130,) if lanes == "row" else (1, 63, 64, 65, 130))
                                 for dt in (F32, BF16)):
        a, x, h0, ref = exact_case(T, cx, reverse, with_h0)
        monkeypatch.setattr(scan, "_FORCE_SEGMENTS", force)
        dev = lambda t: lay(t.to(dtype), lanes, D)                           # noqa: E731
        got = cplx.linear_recurrence(pair([dev(a[0]), dev(a[1])], cx), pair([dev(x[0]), dev(x[1])], cx),
                                     None if h0 is None else pair([h0[0, :, :D].to(dtype).to(DEV), h0[1, :, :D].to(dtype).to(DEV)], cx),
                                     reverse=reverse)
        for g, w in zip((got.real, got.imag) if cx else (got,), (ref.real, ref.imag) if cx else (ref,)):
            # (bf16: the reference's one round-to-nearest-even)
            assert g.dtype == dtype and torch.equal(g.cpu(), w[:, :D].to(dtype)), (T, force, D, dtype)


def close(got, ref, what, dtype, loose=False):
    top = ref.abs().max()
    bound = 1e-5 * ref.abs() + 1e-5 * top if dtype == F32 else 2.0 ** (-7 if loose else -8) * top
    err = ((got.detach().double().cpu() - ref).abs() / bound).max().item()
    print(what, str(dtype)[6:], "error / bound", err)
    assert got.shape == ref.shape and err <= 1.0, (what, err)


@functools.lru_cache(maxsize=None)
def smooth_case(T, unit, dtype, shared):
    """6 rows as [2, 3, T]: a = r e^{i theta}, r in [0.8, 1) or 1 (`shared`: one coefficient row for all), x and h0 normal
    -> the planes (rounded to dtype) and the float64 h and gradients of sum Re(conj(up) h) by autograd through the loop"""
    g = torch.Generator().manual_seed(T + unit)
    r = torch.ones(2, 3, T) if unit else 0.8 + 0.2 * torch.rand(2, 3, T, generator=g)
    th = 2 * math.pi * torch.rand(2, 3, T, generator=g)
    a = torch.stack([r * th.cos(), r * th.sin()])[:, :1, :1] if shared else torch.stack([r * th.cos(), r * th.sin()])
    pl = [t.to(dtype) for t in (a[0], a[1], *torch.randn(2, 2, 3, T, generator=g), *torch.randn(2, 2, 3, generator=g))]
    up = torch.randn(2, 2, 3, T, generator=g).to(dtype)
    leaves = [t.double().requires_grad_() for t in pl]
    h = reference(*(torch.complex(leaves[k], leaves[k + 1]) for k in (0, 2, 4)))
    grads = torch.autograd.grad((h.real * up[0].double()).sum() + (h.imag * up[1].double()).sum(), leaves)
    return pl, up, h.detach(), grads


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("lanes,force,shared", [("row", 0, False), ("column", 0, False), ("row", 3, False), ("column", 3, False),
                                                ("row", 0, True)])
def test_toleranced(lanes, force, shared, unit, dtype, monkeypatch):
    monkeypatch.setattr(scan, "_FORCE_SEGMENTS", force)
    for T in (5003, (ROW if lanes == "row" else COL)["tile"] + 1):
        pl, up, h, grads = smooth_case(T, unit, dtype, shared)
        dev = [(lay(t, lanes) if t.dim() == 3 else t.to(DEV)).requires_grad_() for t in pl]
        out = cplx.linear_recurrence(Cplx(dev[0], dev[1]), Cplx(dev[2], dev[3]), Cplx(dev[4], dev[5]))
        got = torch.autograd.grad([out.real, out.imag], dev, [lay(up[0], lanes), lay(up[1], lanes)])
        what = f"{lanes} force={force} shared={shared} r={'1' if unit else '[0.8,1)'} T={T}"
        close(out.real, h.real, what + " h_r", dtype)
        close(out.imag, h.imag, what + " h_i", dtype)
        for name, g, ref in zip(("da_r", "da_i", "dx_r", "dx_i", "dh0_r", "dh0_i"), got, grads):
            close(g, ref, f"{what} {name}", dtype, loose=name[1] != "x")


@pytest.mark.parametrize("lanes", ["row", "column"])
def test_growth_inside_the_window(lanes):
    g = torch.Generator().manual_seed(7)
    r, th = 1 + 0.05 * torch.rand(2, 3, 600, generator=g), 2 * math.pi * torch.rand(2, 3, 600, generator=g)
    a, x = torch.stack([r * th.cos(), r * th.sin()]), torch.randn(2, 2, 3, 600, generator=g)
    out = cplx.linear_recurrence(Cplx(lay(a[0], lanes), lay(a[1], lanes)), Cplx(lay(x[0], lanes), lay(x[1], lanes)))
    ref = reference(z(a[0], a[1]), z(x[0], x[1]))
    close(out.real, ref.real, f"growth {lanes} max|h| {ref.abs().max():.3g} h_r", F32)
    close(out.imag, ref.imag, f"growth {lanes} h_i", F32)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("lanes,T,fast", [("row", 37, False), ("column", scan.plan(37, 100, 130, torch.float64)["tile"] + 1, False),
                                          ("row", scan.plan(37, 300, None, torch.float64)["tile"] + 1, True)])
def test_gradcheck(lanes, T, fast, reverse):
    """float64 on the kernel; the row tile + 1 has 8196 inputs, so it is checked along random directions (fast_mode)"""
    g = torch.Generator().manual_seed(3)
    shape = (1, 1, T) if fast else (2, 2, T)
    th = 2 * math.pi * torch.rand(shape, dtype=torch.float64, generator=g)
    args = [lay(t, lanes).requires_grad_() for t in (0.9 * th.cos(), 0.9 * th.sin(), *torch.randn(2, *shape, dtype=torch.float64, generator=g))]
    args += [t.to(DEV).requires_grad_() for t in torch.randn(2, *shape[:2], dtype=torch.float64, generator=g)]

    def fn(ar, ai, xr, xi, hr, hi):
        o = cplx.linear_recurrence(Cplx(ar, ai), Cplx(xr, xi), Cplx(hr, hi), reverse=reverse)
        return o.real, o.imag
    assert torch.autograd.gradcheck(fn, args, fast_mode=fast)
    assert torch.autograd.gradgradcheck(fn, args, fast_mode=fast)


def test_layouts_reruns_capture_and_empties():
    """(the layouts run on integer operands: a transposed view and its dense twin take different plans, which agree bit
    for bit only where every order of composition is exact)"""
    g = torch.Generator().manual_seed(5)
    T = ROW["tile"] + 1
    a, x = integers(6, True, g, (4, T + 3))
    base = [t.to(DEV) for t in (a[0], a[1], x[0], x[1])]
    views = {"sliced rows": lambda t: t.transpose(-1, -2)[::2, 1:5, 3:].contiguous()[:, ::2],
             "expanded a": lambda t: t.transpose(-1, -2).contiguous(),
             "transposed": lambda t: t.transpose(-1, -2),
             "last-dim-1 a": lambda t: t.transpose(-1, -2).contiguous()}
    for name, view in views.items():
        ar, ai, xr, xi = (view(t) for t in base)
        if name == "expanded a":
            ar, ai = ar[:1].expand(xr.shape), ai[:1].expand(xr.shape)
        if name == "last-dim-1 a":
            ar, ai = ar[..., :1], ai[..., :1]
        got = cplx.linear_recurrence(Cplx(ar, ai), Cplx(xr, xi))
        twin = cplx.linear_recurrence(Cplx(ar.expand(xr.shape).contiguous(), ai.expand(xr.shape).contiguous()),
                                      Cplx(xr.contiguous(), xi.contiguous()))
        assert torch.equal(got.real, twin.real) and torch.equal(got.imag, twin.imag), name
        assert got.real.stride() == torch.empty_like(xr).stride() and got.imag.stride() == got.real.stride(), name
    # two runs give equal bits, forward and backward; one capture, three replays against the eager result
    lv = [(0.9 * torch.randn(4, 6, T, generator=g)).to(DEV).requires_grad_() for _ in range(4)]
    lv.append(torch.randn(4, 6, generator=g).to(DEV).requires_grad_())
    def step():
        o = cplx.linear_recurrence(Cplx(lv[0], lv[1]), Cplx(lv[2], lv[3]), lv[4])
        return [o.real, o.imag] + list(torch.autograd.grad([o.real, o.imag], lv, [lv[2].detach(), lv[3].detach()]))
    for u, v in zip(step(), step()):
        assert torch.equal(u, v)
    sig = [lv[2].detach().transpose(-1, -2).contiguous().transpose(-1, -2), lv[3].detach()]
    eager = cplx.cumsum(Cplx(sig[0], sig[1]))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            held = cplx.cumsum(Cplx(sig[0], sig[1]))
        for _ in range(3):
            held.real.zero_()
            graph.replay()
            assert torch.equal(held.real, eager.real) and torch.equal(held.imag, eager.imag)
    torch.cuda.synchronize()
    e = torch.zeros(0, 5, device=DEV)
    assert cplx.linear_recurrence(e, Cplx(e, e)).real.shape == (0, 5) and cplx.cumsum(e.t()).shape == (5, 0)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wrappers(dtype):
    g = torch.Generator().manual_seed(9)
    T = ROW["tile"] + 1
    th = 2 * math.pi * torch.rand(3, T, generator=g)
    for name, fn, ref_fn, pr, pi in (("cumsum", cplx.cumsum, torch.cumsum, *torch.randn(2, 3, T, generator=g).to(dtype)),
                                     ("cumprod", cplx.cumprod, torch.cumprod, th.cos().to(dtype), th.sin().to(dtype))):
        got, ref = fn(Cplx(pr.to(DEV), pi.to(DEV))), ref_fn(z(pr, pi), -1)
        close(got.real, ref.real, name + " Cplx re", dtype)
        close(got.imag, ref.imag, name + " Cplx im", dtype)
        real = pr.sign() if name == "cumprod" else pr                        # |a| = 1 for the real product too
        close(fn(real.to(DEV)), ref_fn(real.double(), -1), name + " real", dtype)
