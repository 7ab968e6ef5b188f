"""cplx.rfft / irfft / rfft2 / rfftn / hfft / ihfft on the GPU (csrc/rfft.hip through cplxmodule_amd/rfft.py): bit-exact on
the lengths whose rotations are +-1 and +-i, every path of the half-length route against float64, layout independence in
one launch and without a stray allocation, n / s / norm, the single rounding of bf16, gradients of first and second
order against torch's CPU autograd, bit-identical reruns, hipGraph replay and the errors raised on the device.  Cases:
rfft_cases.py; reference (torch.fft in complex128 / float64 on the CPU) and bounds: fft_cases.py."""
import pytest
import torch

import fft_cases as fc
import rfft_cases as rc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import rfft as hostrfft
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
IDS = ["f32", "bf16", "f64"]
WIDE = [torch.float32, torch.float64]
WIDE_IDS = ["f32", "f64"]


def dev_cplx(re, im, requires_grad=False):
    return Cplx(re.to(DEV).requires_grad_(requires_grad), im.to(DEV).requires_grad_(requires_grad))


def cplx_error(got, ref):
    return fc.normwise(got, ref)


# ---- 1. exact: n in {1, 2, 4} use the rotations +-1, +-i only; integers in, integers out, zero tolerance ---------------
def assert_exact_cplx(got, ref, scale, dtype):
    assert got.real.dtype == dtype and got.imag.dtype == dtype
    assert got.real.shape == ref.shape
    assert torch.equal(got.real.double().cpu(), ref.real.round() * scale), "real plane"
    assert torch.equal(got.imag.double().cpu(), ref.imag.round() * scale), "imaginary plane"


def assert_exact_real(got, ref, scale, dtype):
    assert torch.is_tensor(got) and got.dtype == dtype and got.shape == ref.shape
    assert torch.equal(got.double().cpu(), ref.round() * scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_exact_batch_counts_around_the_workgroup(n, dtype):
    V = hostrfft.plan(n, 1, dtype)[3]
    assert V == 256
    for vectors in (V - 1, V, V + 1, 2 * V + 3):
        x = fc.integers((vectors, n), dtype, seed=vectors + n)[0]
        xd = x.to(DEV)
        fwd = torch.fft.rfft(x.double(), dim=-1)                        # integers: unnormalised
        assert_exact_cplx(cplx.rfft(xd), fwd, 1.0, dtype)
        assert_exact_cplx(cplx.rfft(xd, norm="forward"), fwd, 1.0 / n, dtype)           # 1, 1/2, 1/4: exact
        assert_exact_cplx(cplx.ihfft(xd, norm="forward"), fwd.conj(), 1.0, dtype)
        assert_exact_cplx(cplx.ihfft(xd), fwd.conj(), 1.0 / n, dtype)
        # DC and Nyquist carry imaginary parts, which must not show in the result
        re, im = fc.integers((vectors, n // 2 + 1), dtype, seed=vectors + n + 7)
        assert bool((im[:, 0] != 0).any()) and bool((im[:, -1] != 0).any())
        z = dev_cplx(re, im)
        inv = torch.fft.irfft(fc.c128(re, im), n=n, dim=-1, norm="forward")
        herm = torch.fft.hfft(fc.c128(re, im), n=n, dim=-1)
        assert_exact_real(cplx.irfft(z, n=n, norm="forward"), inv, 1.0, dtype)
        assert_exact_real(cplx.irfft(z, n=n), inv, 1.0 / n, dtype)
        assert_exact_real(cplx.hfft(z, n=n), herm, 1.0, dtype)
        assert_exact_real(cplx.hfft(z, n=n, norm="forward"), herm, 1.0 / n, dtype)


# ---- 2. every path against float64 -------------------------------------------------------------------------------------
def check_paths(n, vectors, dtype):
    x, fwd, xr, xi, inv = rc.path_case(n, vectors, dtype)
    assert bool((xi[:, 0] != 0).all()) and bool((xi[:, -1] != 0).all())
    e_f = cplx_error(cplx.rfft(x.to(DEV)), fwd)
    e_i = rc.real_normwise(cplx.irfft(dev_cplx(xr, xi), n=n, norm="forward"), inv)
    path, cn, points = hostrfft.plan(n, vectors, dtype)[:3]
    print(f"rfft_parity n={n} vectors={vectors} {dtype}: {path} on {cn} complex points (M={points}) "
          f"rfft {e_f:.3g} irfft {e_i:.3g}")
    assert e_f <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_f, e_i)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", rc.PATH_LENGTHS)
def test_every_path(n, dtype):
    check_paths(n, 3, dtype)


def test_length_2_to_the_22():
    check_paths(1 << 22, 1, torch.float32)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
def test_partly_filled_last_workgroup(dtype):
    V = hostrfft.plan(128, 1, dtype)[3]
    assert V == 32
    check_paths(128, V + 1, dtype)


# ---- 3. the arithmetic of a vector does not depend on where it lies ----------------------------------------------------
LAYOUTS = ("contiguous", "channels_last", "transposed", "step2", "expanded")


def layouts_of(base):
    """views of the same values (a [5, 1, 4, 8] tensor broadcast to [5, 6, 4, 8]) behind five layouts, on the device"""
    full = base.to(DEV).expand(5, 6, 4, 8)
    dense = full.contiguous()
    buf = torch.zeros(5, 6, 4, 16, dtype=base.dtype, device=DEV)
    buf[..., ::2] = dense
    views = {"contiguous": dense, "channels_last": dense.contiguous(memory_format=torch.channels_last),
             "transposed": dense.transpose(1, 3).contiguous().transpose(1, 3), "step2": buf[..., ::2], "expanded": full}
    strides = set()
    for v in views.values():
        assert torch.equal(v, dense)
        strides.add(v.stride())
    assert len(strides) == len(views)
    return views


def round512(nbytes):
    return (nbytes + 511) // 512 * 512


@pytest.mark.parametrize("dim", [0, 1, 2, 3])
def test_layouts_give_identical_bits_in_one_launch_each(dim, monkeypatch):
    base = rc.real_gaussian((5, 1, 4, 8), torch.float32, seed=60 + dim)
    ref = torch.fft.rfft(base.double().expand(5, 6, 4, 8), dim=dim)
    calls = []

    def recording(name, *args):
        calls.append((name, args[0].value, args[1]))
        return orig(name, *args)

    orig = hostrfft.call
    monkeypatch.setattr(hostrfft, "call", recording)
    first = None
    for layout, x in layouts_of(base).items():
        n, y = x.shape[dim], None                         # (the previous result is released before the count starts)
        ws_bytes = hostrfft.plan(n, x.numel() // n, torch.float32)[4]
        torch.cuda.synchronize()
        del calls[:]
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = cplx.rfft(x, dim=dim)
        # exactly one launch, reading the tensor where it lies (no layout copy), with no imaginary plane
        assert calls == [("cplxamd_rfft", x.data_ptr(), None)], (layout, calls)
        # nothing but the two output planes of n // 2 + 1 entries stays allocated; at the peak, the workspace as well
        plane = round512(x.numel() // n * (n // 2 + 1) * 4)
        assert y.real.shape[dim] == n // 2 + 1 and y.real.numel() * 4 <= plane
        assert torch.cuda.memory_allocated() - before == 2 * plane, layout
        assert torch.cuda.max_memory_allocated() - before == 2 * plane + round512(ws_bytes), layout
        if layout != "expanded":                          # the result keeps the input's memory order
            order = lambda t: sorted(range(4), key=lambda d: (-t.stride(d), d))  # noqa: E731
            assert order(y.real) == order(x) and y.real.stride() == y.imag.stride()
        if first is None:
            first = y
            assert cplx_error(y, ref) <= fc.F32_TOL
        else:
            assert torch.equal(y.real.contiguous(), first.real.contiguous()), layout
            assert torch.equal(y.imag.contiguous(), first.imag.contiguous()), layout


def test_rfft2_is_one_real_and_one_complex_launch(monkeypatch):
    from cplxmodule_amd import fft as hostfft
    names = []
    for mod in (hostrfft, hostfft):
        orig = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *args, _orig=orig: (names.append(name), _orig(name, *args))[1])
    x = rc.real_gaussian((2, 3, 16, 12), torch.float32, seed=70).to(DEV)
    y = cplx.rfft2(x)
    assert names == ["cplxamd_rfft", "cplxamd_fft"]
    del names[:]
    cplx.irfft2(y)
    assert names == ["cplxamd_fft", "cplxamd_rfft"]


def test_planes_without_a_common_layout_are_copied_once(monkeypatch):
    _, _, xr, xi, inv = rc.path_case(64, 30, torch.float32)
    z = Cplx(xr.to(DEV), xi.to(DEV).t().contiguous().t())
    assert z.real.stride() != z.imag.stride()
    calls = []
    orig = hostrfft.call
    monkeypatch.setattr(hostrfft, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    assert rc.real_normwise(cplx.irfft(z, n=64, norm="forward"), inv) <= fc.F32_TOL
    assert calls == ["cplxamd_rfft"]
    # more than three batch runs: every second index of four batch dims
    big = rc.real_gaussian((4, 4, 4, 4, 16), torch.float32, seed=5)
    v = big.to(DEV)[::2, ::2, ::2, ::2]
    assert cplx_error(cplx.rfft(v), torch.fft.rfft(big[::2, ::2, ::2, ::2].double())) <= fc.F32_TOL


# ---- 4. n / s and norm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
def test_padding_truncation_and_norms(dtype):
    x = rc.real_gaussian((5, 64), dtype, seed=21)
    re, im = rc.half_spectrum((5, 33), dtype, seed=22)
    z = dev_cplx(re, im)
    for norm in (None, "backward", "ortho", "forward"):
        for n in (96, 48, 47, 97, None):
            got, ref = cplx.rfft(x.to(DEV), n=n, norm=norm), torch.fft.rfft(x.double(), n=n, norm=norm)
            assert got.real.shape == ref.shape and got.real.dtype == dtype
            assert cplx_error(got, ref) <= fc.tol(dtype), ("rfft", n, norm)
        for n in (96, 48, 47, 97, 64, 65, None):          # fewer entries than n // 2 + 1: zero padding; more: truncation
            got, ref = cplx.irfft(z, n=n, norm=norm), torch.fft.irfft(fc.c128(re, im), n=n, norm=norm)
            assert got.shape == ref.shape and got.dtype == dtype
            assert rc.real_normwise(got, ref) <= fc.tol(dtype), ("irfft", n, norm)
    for n in (9, 10):
        xs = rc.real_gaussian((4, n), dtype, seed=23 + n)
        for norm in (None, "ortho", "forward"):
            back = cplx.irfft(cplx.rfft(xs.to(DEV), norm=norm), n=n, norm=norm)
            assert back.shape == xs.shape and rc.real_normwise(back, xs.double()) <= fc.tol(dtype), (n, norm)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("shape", [(2, 3, 16, 12), (2, 3, 9, 10)])
def test_rfft2_and_irfft2(shape, dtype):
    x = rc.real_gaussian(shape, dtype, seed=24)
    re, im = rc.half_spectrum(shape, dtype, seed=25)
    z = dev_cplx(re, im)
    for kw in (dict(), dict(norm="ortho"), dict(s=(12, 7)), dict(dim=(1, 2), norm="forward"), dict(dim=(3, 0))):
        got, ref = cplx.rfft2(x.to(DEV), **kw), torch.fft.rfft2(x.double(), **kw)
        assert got.real.shape == ref.shape and cplx_error(got, ref) <= fc.tol(dtype), ("rfft2", kw)
        got, ref = cplx.irfft2(z, **kw), torch.fft.irfft2(fc.c128(re, im), **kw)
        assert got.shape == ref.shape and rc.real_normwise(got, ref) <= fc.tol(dtype), ("irfft2", kw)
    back = cplx.irfft2(cplx.rfft2(x.to(DEV)), s=shape[-2:])
    assert rc.real_normwise(back, x.double()) <= fc.tol(dtype)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
def test_rfftn_dims_and_shapes(dtype):
    x = rc.real_gaussian((6, 5, 8, 10), dtype, seed=26)
    re, im = rc.half_spectrum((6, 5, 8, 10), dtype, seed=27)
    z = dev_cplx(re, im)
    for kw in (dict(), dict(dim=(0, 2)), dict(s=(4, 12)), dict(s=(9, 8, 7), dim=(1, 2, 0), norm="ortho"),
               dict(dim=(-1, 1), norm="forward"), dict(s=(5,), dim=(2,))):
        got, ref = cplx.rfftn(x.to(DEV), **kw), torch.fft.rfftn(x.double(), **kw)
        assert got.real.shape == ref.shape and cplx_error(got, ref) <= fc.tol(dtype), ("rfftn", kw)
        got, ref = cplx.irfftn(z, **kw), torch.fft.irfftn(fc.c128(re, im), **kw)
        assert got.shape == ref.shape and rc.real_normwise(got, ref) <= fc.tol(dtype), ("irfftn", kw)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [8, 9, 100])
def test_hfft_and_ihfft(n, dtype):
    x = rc.real_gaussian((3, n), dtype, seed=28 + n)
    re, im = rc.half_spectrum((3, n // 2 + 1), dtype, seed=29 + n)
    z = dev_cplx(re, im)
    for norm in (None, "ortho", "forward"):
        for m in (None, n, n + 3):
            got, ref = cplx.ihfft(x.to(DEV), n=m, norm=norm), torch.fft.ihfft(x.double(), n=m, norm=norm)
            assert got.real.shape == ref.shape and cplx_error(got, ref) <= fc.tol(dtype), ("ihfft", m, norm)
            got, ref = cplx.hfft(z, n=m, norm=norm), torch.fft.hfft(fc.c128(re, im), n=m, norm=norm)
            assert got.shape == ref.shape and rc.real_normwise(got, ref) <= fc.tol(dtype), ("hfft", m, norm)
    # the identities the kernels rest on: hfft(X) = irfft(conj X, norm="forward"), ihfft(x) = conj rfft(x, norm="forward")
    conj = Cplx(z.real, -z.imag)
    assert rc.real_normwise(cplx.hfft(z, n=n), cplx.irfft(conj, n=n, norm="forward").double().cpu()) <= 2 * fc.tol(dtype)
    f = cplx.rfft(x.to(DEV), norm="forward")
    assert cplx_error(cplx.ihfft(x.to(DEV)), fc.c128(f.real, -f.imag)) <= 2 * fc.tol(dtype)


# ---- 5. bf16 is rounded once -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rfft1000", "rfft2_16", "rfft2_64", "irfft1000"])
def test_bf16_rounds_once(case):
    if case == "rfft1000":
        x = rc.real_gaussian((4, 1000), torch.bfloat16, seed=31)
        got, ref = cplx.rfft(x.to(DEV)), torch.fft.rfft(x.double())
        assert got.real.dtype == torch.bfloat16 and got.imag.dtype == torch.bfloat16
        bad, worst = fc.bf16_violations(got, ref)
    elif case == "irfft1000":
        re, im = rc.half_spectrum((4, 501), torch.bfloat16, seed=33)
        got, ref = cplx.irfft(dev_cplx(re, im), n=1000), torch.fft.irfft(fc.c128(re, im), n=1000)
        assert got.dtype == torch.bfloat16
        bad, worst = rc.bf16_real_violations(got, ref)
    else:
        n = int(case.split("_")[1])
        x = rc.real_gaussian((3, n, n), torch.bfloat16, seed=32 + n)
        got, ref = cplx.rfft2(x.to(DEV)), torch.fft.rfft2(x.double())
        assert got.real.dtype == torch.bfloat16 and got.imag.dtype == torch.bfloat16
        bad, worst = fc.bf16_violations(got, ref)
    print(f"rfft_parity bf16 {case}: {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} of the bound")
    assert bad == 0, (bad, worst)


# ---- 6. gradients against torch's CPU float64 autograd of the same expression ------------------------------------------
def rfft_loss(fn, x, power):
    y = fn(x)
    re, im = (y.real, y.imag)
    return ((re.double() ** 2 + im.double() ** 2) ** (power // 2)).sum()


def irfft_loss(fn, re, im, power, weight):
    return ((fn(re, im).double() ** power) * weight).sum()


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [8, 9, 100, 1024, 2048])
def test_first_order_gradients(n, dtype):
    x = rc.real_gaussian((3, n), dtype, seed=41)
    re, im = rc.half_spectrum((3, n // 2 + 1), dtype, seed=42)
    for kw in (dict(), dict(n=n + n // 2), dict(n=n - n // 4), dict(norm="ortho"), dict(norm="ortho", n=n + 1)):
        xc = x.double().requires_grad_()
        ref, = torch.autograd.grad(rfft_loss(lambda t: torch.fft.rfft(t, dim=-1, **kw), xc, 2), xc)
        xg = x.to(DEV).requires_grad_()
        got, = torch.autograd.grad(rfft_loss(lambda t: cplx.rfft(t, **kw), xg, 2), xg)
        assert got.dtype == dtype and got.shape == x.shape
        e_r = rc.real_normwise(got, ref)
        # irfft: a weighted sum of squares, so that the incoming gradient is no Hermitian-symmetric special case
        m = kw.get("n", 2 * (n // 2))
        w = rc.real_gaussian((3, m), torch.float64, seed=43)
        rc_, ic_ = re.double().requires_grad_(), im.double().requires_grad_()
        ref = torch.autograd.grad(irfft_loss(lambda a, b: torch.fft.irfft(torch.complex(a, b), dim=-1, **kw), rc_, ic_, 2, w),
                                  (rc_, ic_))
        rg, ig = re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_()
        got = torch.autograd.grad(irfft_loss(lambda a, b: cplx.irfft(Cplx(a, b), **kw), rg, ig, 2, w.to(DEV)), (rg, ig))
        assert got[0].dtype == dtype and got[0].shape == re.shape
        e_i = fc.normwise(torch.complex(got[0].double().cpu(), got[1].double().cpu()), torch.complex(ref[0], ref[1]))
        print(f"rfft_parity gradients n={n} {dtype} {kw}: rfft {e_r:.3g} irfft {e_i:.3g}")
        assert e_r <= fc.tol(dtype) and e_i <= fc.tol(dtype), (kw, e_r, e_i)
        # the imaginary parts of DC and (even length) Nyquist do not enter irfft: their gradient is exactly 0
        assert bool((got[1][:, 0] == 0).all())
        if m % 2 == 0 and m // 2 < re.shape[1]:
            assert bool((got[1][:, m // 2] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rfft2_gradients(dtype):
    x = rc.real_gaussian((2, 3, 16, 12), dtype, seed=44)
    xc = x.double().requires_grad_()
    ref, = torch.autograd.grad(rfft_loss(torch.fft.rfft2, xc, 2), xc)
    xg = x.to(DEV).requires_grad_()
    got, = torch.autograd.grad(rfft_loss(cplx.rfft2, xg, 2), xg)
    assert got.dtype == dtype
    err = rc.real_normwise(got, ref)
    print(f"rfft_parity rfft2 gradient {dtype}: {err:.3g}")
    if dtype == torch.bfloat16:
        # as test_gpu_fft.py::test_fft2_gradients: y is rounded to bf16 once (2^-8 per entry), the loss' gradient 2 y
        # inherits that, and the gradient, one more transform in float32 (1e-5 each way), is rounded once more (2^-8)
        assert err <= 2.0 ** -7 + 2e-5
    else:
        assert err <= fc.tol(dtype)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [8, 100])
def test_hessian_vector_products(n, dtype):
    """d <d sum|y|^4 / dx, v> / dx for y = rfft(x), and the same for sum w y^4 with y = irfft(X)"""
    x = rc.real_gaussian((3, n), dtype, seed=45)
    v = rc.real_gaussian((3, n), torch.float64, seed=46)

    def hvp(fn, t, vec):
        g, = torch.autograd.grad(rfft_loss(fn, t, 4), t, create_graph=True)
        return torch.autograd.grad((g.double() * vec).sum(), t)[0]

    ref = hvp(lambda t: torch.fft.rfft(t, dim=-1), x.double().requires_grad_(), v)
    got = hvp(cplx.rfft, x.to(DEV).requires_grad_(), v.to(DEV))
    e_r = rc.real_normwise(got, ref)
    re, im = rc.half_spectrum((3, n // 2 + 1), dtype, seed=47)
    vr, vi = fc.gaussian((3, n // 2 + 1), torch.float64, seed=48)
    w = rc.real_gaussian((3, n), torch.float64, seed=49)

    def hvp2(fn, a, b, va, vb, weight):
        g = torch.autograd.grad(irfft_loss(fn, a, b, 4, weight), (a, b), create_graph=True)
        return torch.autograd.grad((g[0].double() * va).sum() + (g[1].double() * vb).sum(), (a, b))

    ref = hvp2(lambda a, b: torch.fft.irfft(torch.complex(a, b), n=n, dim=-1), re.double().requires_grad_(),
               im.double().requires_grad_(), vr, vi, w)
    got = hvp2(lambda a, b: cplx.irfft(Cplx(a, b), n=n), re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_(),
               vr.to(DEV), vi.to(DEV), w.to(DEV))
    e_i = fc.normwise(torch.complex(got[0].double().cpu(), got[1].double().cpu()), torch.complex(ref[0], ref[1]))
    print(f"rfft_parity second order n={n} {dtype}: rfft {e_r:.3g} irfft {e_i:.3g}")
    assert e_r <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_r, e_i)


# ---- 7. reruns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 2048, 65536])
def test_reruns_are_bit_identical(n):
    x, _, xr, xi, _ = rc.path_case(n, 3, torch.float32)
    xd, z = x.to(DEV), dev_cplx(xr, xi)
    a, b = cplx.rfft(xd), cplx.rfft(xd)
    assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)
    assert torch.equal(cplx.irfft(z, n=n), cplx.irfft(z, n=n))
    assert torch.equal(cplx.irfft(a, n=n), cplx.irfft(b, n=n))


# ---- 8. hipGraph -------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    def step(x):
        y = cplx.rfft(x, norm="ortho")
        back = cplx.irfft(Cplx(y.real * 0.5, y.imag), n=x.shape[-1], norm="ortho")
        g, = torch.autograd.grad((back.float() ** 2).sum(), x)
        return y.real, y.imag, back, g

    x0 = rc.real_gaussian((8, 6, 200), torch.bfloat16, seed=51)
    sx = x0.to(DEV).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx)                                          # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx)
    for seed in (52, 53):
        x = rc.real_gaussian((8, 6, 200), torch.bfloat16, seed=seed)
        with torch.no_grad():
            sx.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(x.to(DEV).requires_grad_())
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


# ---- 9. errors on the device -------------------------------------------------------------------------------------------
def test_device_errors_and_empty_batches():
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.irfft(Cplx(torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16)))
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.rfft(torch.zeros(1, 8, device=DEV), n=(1 << 22) + 1)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.hfft(Cplx(torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV)), n=(1 << 22) + 1)
    with pytest.raises(CplxAmdError):
        cplx.rfft(torch.zeros(4, 8, device=DEV, dtype=torch.float16))
    with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
        cplx.ihfft(Cplx(torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV)))
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.irfft(torch.zeros(4, 8, device=DEV))
    with pytest.raises(CplxAmdError, match="different devices|no CPU path"):
        cplx.irfft(Cplx(torch.zeros(4, 8, device=DEV), torch.zeros(4, 8)))
    empty = torch.zeros(0, 64, device=DEV, requires_grad=True)
    out = cplx.rfft(empty)
    assert out.real.shape == (0, 33) and out.imag.shape == (0, 33)
    (out.real.sum() + out.imag.sum()).backward()
    assert empty.grad.shape == (0, 64)
    assert cplx.rfft(empty, n=100).real.shape == (0, 51)
    ez = Cplx(torch.zeros(0, 33, device=DEV, requires_grad=True), torch.zeros(0, 33, device=DEV, requires_grad=True))
    back = cplx.irfft(ez)
    assert back.shape == (0, 64)
    back.sum().backward()
    assert ez.real.grad.shape == (0, 33) and ez.imag.grad.shape == (0, 33)
    assert cplx.hfft(ez, n=9).shape == (0, 9) and cplx.rfft2(torch.zeros(0, 4, 6, device=DEV)).real.shape == (0, 4, 4)
