"""cplx.czt / zoom_fft on the GPU (csrc/czt.hip through cplxmodule_amd/czt.py): parity on every path, contour, dtype and
vector count for `Cplx` and real input, strided inputs read in place, the single rounding of bf16 planes, derivatives of
first and second order, gradient parity per path, bit-identical reruns, hipGraph replay, the FFT special case and empty
batches.  Cases, reference (the direct sum in complex128 on the CPU) and bounds: czt_cases.py."""
import math

import pytest
import torch

import czt_cases as cc
from fft_cases import F64_TOL
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import czt as hostczt
from cplxmodule_amd._runs import dense_like, runs

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
PARITY = [pytest.param(n, m, dt, name, id=f"{n}x{m}-{tag}-{name}")
          for n, m in cc.SHAPES for tag, dt in DTYPES.items() for name in cc.CONTOURS
          if (dt == torch.float32 or (n, m) not in cc.F32_ONLY) and cc.contour_params(name, n, m) is not None]


def same_bits(a, b):
    return torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)


def check(got, ref, dtype, what):
    assert got.real.dtype == dtype and got.imag.dtype == dtype and got.real.shape == ref.shape, what
    if dtype == torch.bfloat16:
        bad, worst = cc.bf16_plane_violations(got, ref)
        print(what, "bf16 worst ratio", worst)
        assert bad == 0, (what, bad, worst)
    else:
        err = cc.normwise(got, ref)
        print(what, "norm-wise error", err)
        assert err <= (cc.f64_tol() if dtype == torch.float64 else cc.F32_TOL), (what, err)


# ---- 1. parity: every shape x dtype x contour, 1 and V + 1 (or 3) vectors, Cplx and real input -------------------------
@pytest.mark.parametrize("n,m,dtype,name", PARITY)
def test_parity(n, m, dtype, name):
    re, im, ref, ref_real = cc.case(n, m, dtype, name)
    assert hostczt.plan(n, m, 1, dtype)[1] == cc.vectors_per_workgroup(n, m)
    for vectors in cc.vector_counts(n, m):
        dre, dim = re[:vectors].to(DEV), im[:vectors].to(DEV)
        check(cc.apply(name, Cplx(dre, dim), m), ref[:vectors], dtype, f"cplx x{vectors}")
        check(cc.apply(name, dre, m), ref_real[:vectors], dtype, f"real x{vectors}")


# ---- 2. strided inputs are read in place: the same bits as from a dense copy -----------------------------------------------
def _views(t):
    """name -> a view of the values of t [2, 3, 4, n] behind another layout"""
    out = {}
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    buf[..., ::2] = t
    out["step-sliced"] = buf[..., ::2]
    out["transposed"] = t.transpose(0, 2).contiguous().transpose(0, 2)
    out["last dim not innermost"] = t.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    big = torch.zeros(2, 3, 9, t.shape[-1], dtype=t.dtype, device=t.device)
    big[:, :, :8:2] = t
    out["two runs"] = big[:, :, :8:2]
    big = torch.zeros(2, 7, 8, t.shape[-1], dtype=t.dtype, device=t.device)
    big[:, :6:2, ::2] = t
    out["three runs"] = big[:, :6:2, ::2]
    big = torch.zeros(2, 2, 6, 8, t.shape[-1], dtype=t.dtype, device=t.device)
    big[:, 0, ::2, ::2] = t
    out["three runs, sliced"] = big[:, 0, ::2, ::2]
    for v in out.values():
        assert torch.equal(v, t) and v.stride() != t.stride()
    count = lambda v: len(runs(v.shape, (v.stride(), dense_like(v, 3, 5)[1]), 3))  # noqa: E731
    assert [count(out[k]) for k in ("step-sliced", "two runs", "three runs", "three runs, sliced")] == [1, 2, 3, 3]
    return out


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("n,m", [(100, 37), (513, 513)])
def test_strided_inputs(n, m, tag):
    dtype = DTYPES[tag]
    re, im = cc.gaussian((2, 3, 4, n), dtype, seed=7)
    re, im = re.to(DEV), im.to(DEV)
    want = cc.apply("spiral_in", Cplx(re, im), m)
    want_real = cc.apply("zoom", re, m)
    check(want, cc.direct(cc.c128(re, im), m, *cc.contour_params("spiral_in", n, m)), dtype, "dense")
    vr, vi = _views(re), _views(im)
    for layout in vr:
        got = cc.apply("spiral_in", Cplx(vr[layout], vi[layout]), m)
        assert same_bits(got, want), layout
        assert same_bits(cc.apply("zoom", vr[layout], m), want_real), layout
    # planes of different layouts: one of them is copied
    assert same_bits(cc.apply("spiral_in", Cplx(vr["transposed"], vi["two runs"]), m), want)
    # the result has the input's memory order
    got = cc.apply("spiral_in", Cplx(vr["transposed"], vi["transposed"]), m)
    assert got.real.stride() == torch.empty(4, 3, 2, m).transpose(0, 2).stride()
    # `expand`ed rows: stride 0, every row the same vector
    row = Cplx(re[:1, :1, :1].expand(2, 3, 4, n), im[:1, :1, :1].expand(2, 3, 4, n))
    assert row.real.stride()[:3] == (0, 0, 0)
    got = cc.apply("spiral_in", row, m)
    assert same_bits(got, Cplx(want.real[:1, :1, :1].expand(2, 3, 4, m), want.imag[:1, :1, :1].expand(2, 3, 4, m)))
    # more leading dims than three runs hold: one copy, the same bits
    re5 = torch.zeros(2, 3, 6, 8, 2 * n, dtype=dtype, device=DEV)
    im5 = torch.zeros_like(re5)
    re5[:, 0, ::2, ::2, ::2], im5[:, 0, ::2, ::2, ::2] = re, im
    v5 = re5[:, ::2, ::2, ::2, ::2]
    assert len(runs(v5.shape, (v5.stride(), dense_like(v5, 4, m)[1]), 4)) == 4
    got = cc.apply("spiral_in", Cplx(v5, im5[:, ::2, ::2, ::2, ::2]), m)
    assert same_bits(Cplx(got.real[:, 0], got.imag[:, 0]), want)


# ---- 3. bf16 planes: float32 arithmetic, one rounding -------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 37), (513, 513), (5000, 3194)])
def test_bf16_rounds_once(n, m):
    re, im = cc.gaussian((3, n), torch.bfloat16, seed=3)
    re, im = re.to(DEV), im.to(DEV)
    for name in ("zoom", "spiral_out"):
        wide = cc.apply(name, Cplx(re.float(), im.float()), m)
        got = cc.apply(name, Cplx(re, im), m)
        assert got.real.dtype == torch.bfloat16
        assert same_bits(got, Cplx(wide.real.bfloat16(), wide.imag.bfloat16())), name
        wide = cc.apply(name, re.float(), m)
        assert same_bits(cc.apply(name, re, m), Cplx(wide.real.bfloat16(), wide.imag.bfloat16())), name


# ---- 4. derivatives of first and second order against torch autograd of the dense-matrix formulation (float64) ---------
def _dense_matrix(n, m, p):
    """K [n, m] complex128 on the CPU: y = x K"""
    return cc.direct(torch.eye(n, dtype=torch.complex128), m, *p)


def _loss(yr, yi, c):
    return (yr ** 2 * c[0]).sum() + (yi ** 3 * c[1]).sum() + (yr * yi * c[2]).sum()


def _two_derivatives(fn, planes, c, v):
    yr, yi = fn(*planes)
    g = torch.autograd.grad(_loss(yr, yi, c), planes, create_graph=True)
    h = torch.autograd.grad(sum((a * b).sum() for a, b in zip(g, v)), planes)
    return [t.detach() for t in g], list(h)


@pytest.mark.parametrize("real", [False, True], ids=["cplx", "real"])
@pytest.mark.parametrize("name", ["zoom", "spiral_in"])
@pytest.mark.parametrize("n,m", [(40, 23), (9, 40)])
def test_first_and_second_derivatives(n, m, name, real):
    K = _dense_matrix(n, m, cc.contour_params(name, n, m))
    g = torch.Generator().manual_seed(n + m)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g).to(DEV)  # noqa: E731
    planes = [rnd(3, n).requires_grad_() for _ in range(1 if real else 2)]
    c, v = [rnd(3, m) for _ in range(3)], [rnd(3, n) for _ in planes]

    def ours(*p):
        y = cc.apply(name, p[0] if real else Cplx(*p), m)
        return y.real, y.imag

    def dense(*p):
        y = torch.complex(p[0], torch.zeros_like(p[0]) if real else p[1]) @ K
        return y.real, y.imag

    got = _two_derivatives(ours, planes, c, v)
    cpu = lambda ts: [t.detach().cpu() for t in ts]  # noqa: E731
    want = _two_derivatives(dense, [t.requires_grad_() for t in cpu(planes)], cpu(c), cpu(v))
    for order, (gs, ws) in enumerate(zip(got, want), 1):
        for a, b in zip(gs, ws):
            err = float(torch.linalg.norm(a.cpu() - b) / torch.linalg.norm(b))
            print(f"derivative {order}: {err}")
            assert err <= F64_TOL, (order, err)                    # the repository's float64 bound (fft_cases)


# ---- 5. gradient parity in float32, one shape per path ------------------------------------------------------------------
@pytest.mark.parametrize("real", [False, True], ids=["cplx", "real"])
@pytest.mark.parametrize("n,m", [(100, 37), (513, 513), (5000, 3194)])
def test_gradient_parity_f32(n, m, real):
    for name in ("zoom_endpoint", "spiral_out"):
        p = cc.contour_params(name, n, m)
        re, im = cc.gaussian((3, n), torch.float32, seed=5)
        gr, gi = cc.gaussian((3, m), torch.float32, seed=6)
        xr, xi = re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_()
        y = cc.apply(name, xr if real else Cplx(xr, xi), m)
        grads = torch.autograd.grad((y.real * gr.to(DEV)).sum() + (y.imag * gi.to(DEV)).sum(), (xr,) if real else (xr, xi))
        want = cc.adjoint(cc.c128(gr, gi), n, *p)
        if real:
            assert grads[0].shape == (3, n) and grads[0].dtype == torch.float32
            err = float(torch.linalg.norm(grads[0].double().cpu() - want.real) / torch.linalg.norm(want.real))
        else:
            err = cc.normwise(Cplx(*grads), want)
        print(name, "gradient norm-wise error", err)
        assert err <= cc.F32_TOL, (name, err)


# ---- 6. the same input gives the same bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 37), (513, 513), (5000, 3194)])
def test_rerun_gives_the_same_bits(n, m):
    re, im = cc.gaussian((3, n), torch.float32, seed=8)
    x = Cplx(re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_())

    def step():
        y = cc.apply("spiral_in", x, m)
        return (y.real, y.imag) + torch.autograd.grad((y.real ** 2).sum() + (y.imag ** 2).sum(), (x.real, x.imag))

    first = step()
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(first, step()))


# ---- 7. hipGraph ---------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    n, m = 300, 100

    def step(re, im):
        y = cplx.zoom_fft(Cplx(re, im), (0.2, 0.6), m)
        z = cplx.czt(re, m, 1.00001 * complex(math.cos(0.01), -math.sin(0.01)), 0.999j)
        loss = (y.real.float() ** 2).sum() + (y.imag.float() ** 2).sum() + (z.real.float() * z.imag.float()).sum()
        return (y.real, y.imag, z.real, z.imag) + torch.autograd.grad(loss, (re, im))

    re0, im0 = cc.gaussian((5, n), torch.bfloat16, seed=51)
    sre, sim = re0.to(DEV).requires_grad_(), im0.to(DEV).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sre, sim)                                    # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sre, sim)
    for seed in (52, 53):
        re, im = cc.gaussian((5, n), torch.bfloat16, seed=seed)
        with torch.no_grad():
            sre.copy_(re)
            sim.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_())
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


# ---- 8. czt(x) with the defaults is cplx.fft(x) ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(100, 100), (100, 128), (1000, 1000), (1000, 1024), (5000, 5000)])
def test_defaults_equal_fft(n, m):
    re, im = cc.gaussian((3, n), torch.float32, seed=9)
    x = Cplx(re.to(DEV), im.to(DEV))
    fft = cplx.fft(x, n=m)
    ref = cc.c128(fft.real, fft.imag)
    if m & (m - 1) == 0:
        assert same_bits(cplx.czt(x, m), fft)                                    # a power of two: the FFT kernel itself
    assert cc.normwise(cplx.czt(x, m), ref) <= cc.F32_TOL
    w = complex(math.cos(2 * math.pi / m), -math.sin(2 * math.pi / m))
    assert cc.normwise(cplx.czt(x, m, w), ref) <= cc.F32_TOL                     # the chirp-z kernel, w given
    zero = cplx.fft(Cplx(x.real, torch.zeros_like(x.real)), n=m)
    assert cc.normwise(cplx.czt(x.real, m), cc.c128(zero.real, zero.imag)) <= cc.F32_TOL   # a real input: the chirp-z kernel
    if m == n:
        assert cc.normwise(cplx.zoom_fft(x, 2.0, m), ref) <= cc.F32_TOL          # the whole circle


# ---- 9. an empty batch ---------------------------------------------------------------------------------------------------
def test_empty_batch():
    for x in (Cplx(torch.zeros(0, 64, device=DEV, requires_grad=True), torch.zeros(0, 64, device=DEV, requires_grad=True)),
              torch.zeros(2, 0, 64, device=DEV, requires_grad=True)):
        for out in (cplx.czt(x, 10, 0.999j), cplx.zoom_fft(x, 0.5, 10)):
            assert out.real.shape == x.shape[:-1] + (10,) and out.real.numel() == 0
            (out.real.sum() + out.imag.sum()).backward()
    assert x.grad.shape == x.shape
