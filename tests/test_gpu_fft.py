"""cplx.fft / ifft / fft2 / fftn on the GPU (csrc/fft.hip through cplxmodule_amd/fft.py): bit-exact on the lengths whose
rotations are +-1 and +-i, every path against complex128, unit impulses, layout independence, n / s / norm, the single
rounding of bf16 planes, gradients of first and second order, bit-identical reruns, hipGraph replay and the errors
raised on the device.  Cases, reference (torch.fft in complex128 on the CPU) and bounds: fft_cases.py."""
import pytest
import torch

import fft_cases as fc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
IDS = ["f32", "bf16", "f64"]


def on_device(re, im, requires_grad=False):
    return Cplx(re.to(DEV).requires_grad_(requires_grad), im.to(DEV).requires_grad_(requires_grad))


def relayout(t, layout):
    """the same values behind another layout (4-d tensors)"""
    if layout == "channels_last":
        v = t.contiguous(memory_format=torch.channels_last)
    elif layout == "transposed":
        v = t.transpose(1, 3).contiguous().transpose(1, 3)
    elif layout == "sliced":                              # every second element of a buffer twice as long
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        buf[..., ::2] = t
        v = buf[..., ::2]
    else:
        return t
    assert torch.equal(v, t) and v.stride() != t.stride()
    return v


def same_bits(a, b):
    return torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)


# ---- 1. exact: n in {1, 2, 4} use the rotations +-1, +-i only; integers in, integers out, zero tolerance ---------------
def exact_ref(re, im, fn, scale=1.0, **kw):
    ref = fc.reference(re, im, fn, norm="backward" if fn.startswith("f") else "forward", **kw)
    return torch.complex(ref.real.round(), ref.imag.round()) * scale


def assert_exact(got, ref, dtype):
    assert got.real.dtype == dtype and got.imag.dtype == dtype
    assert got.real.shape == ref.shape
    assert torch.equal(got.real.double().cpu(), ref.real), "real plane"
    assert torch.equal(got.imag.double().cpu(), ref.imag), "imaginary plane"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 4])
def test_exact_batch_counts_around_the_workgroup(n, dtype):
    V = hostfft.plan(n, 1, dtype)[1]
    assert V == 256
    for vectors in (V - 1, V, V + 1, 2 * V + 3):
        re, im = fc.integers((vectors, n), dtype, seed=vectors + n)
        z = on_device(re, im)
        assert_exact(cplx.fft(z), exact_ref(re, im, "fft"), dtype)
        assert_exact(cplx.ifft(z, norm="forward"), exact_ref(re, im, "ifft"), dtype)
        assert_exact(cplx.fft(z, norm="forward"), exact_ref(re, im, "fft", 1.0 / n), dtype)      # 1, 1/2, 1/4: exact
        assert_exact(cplx.ifft(z), exact_ref(re, im, "ifft", 1.0 / n), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_fft2_4x4(dtype):
    re, im = fc.integers((3, 5, 4, 4), dtype, seed=1)
    z = on_device(re, im)
    assert_exact(cplx.fft2(z), exact_ref(re, im, "fft2"), dtype)
    assert_exact(cplx.ifft2(z, norm="forward"), exact_ref(re, im, "ifft2"), dtype)
    assert_exact(cplx.fft2(z, norm="forward"), exact_ref(re, im, "fft2", 1.0 / 16), dtype)
    assert_exact(cplx.fftn(z, dim=(0, 3), s=(2, 4)), exact_ref(re, im, "fftn", dim=(0, 3), s=(2, 4)), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_exact_beyond_a_65535_grid(dtype):
    re, im = fc.integers((70000, 4), dtype, seed=2)
    assert_exact(cplx.fft(on_device(re, im)), exact_ref(re, im, "fft"), dtype)
    # the same vectors as columns: the packed vectors of a workgroup lie next to each other in memory
    ret, imt = re.t().contiguous(), im.t().contiguous()
    assert_exact(cplx.fft(on_device(ret, imt), dim=0), exact_ref(ret, imt, "fft", dim=0), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim", [0, 1, 2, 3])
def test_exact_along_each_dim(dim, dtype):
    """[5, 4, 3, 4] with n = 4: dim 0 is truncated, dim 2 zero-padded inside the loader"""
    re, im = fc.integers((5, 4, 3, 4), dtype, seed=3 + dim)
    z = on_device(re, im)
    assert_exact(cplx.fft(z, n=4, dim=dim), exact_ref(re, im, "fft", n=4, dim=dim), dtype)
    assert_exact(cplx.ifft(z, n=4, dim=dim, norm="forward"), exact_ref(re, im, "ifft", n=4, dim=dim), dtype)
    assert_exact(cplx.fft(z, n=2, dim=dim - 4), exact_ref(re, im, "fft", n=2, dim=dim), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["channels_last", "transposed", "sliced", "expanded"])
def test_exact_on_views(layout, dtype):
    re, im = fc.integers((3, 4, 5, 4), dtype, seed=11)
    if layout == "expanded":
        re, im = re[:, :1], im[:, :1]
        z = Cplx(re.to(DEV).expand(3, 4, 5, 4), im.to(DEV).expand(3, 4, 5, 4))
        re, im = re.expand(3, 4, 5, 4), im.expand(3, 4, 5, 4)
        assert z.real.stride(1) == 0
    else:
        z = Cplx(relayout(re.to(DEV), layout), relayout(im.to(DEV), layout))
    for dim in (1, 3):
        got = cplx.fft(z, dim=dim)
        assert_exact(got, exact_ref(re, im, "fft", dim=dim), dtype)
        if layout != "expanded":                          # the result keeps the input's memory order
            assert got.real.stride() == torch.empty_like(z.real).stride() == got.imag.stride()
    assert_exact(cplx.fft2(z, dim=(1, 3)), exact_ref(re, im, "fft2", dim=(1, 3)), dtype)


# ---- 2. every path against complex128 --------------------------------------------------------------------------------
def check_paths(n, vectors, dtype):
    re, im, fwd, inv = fc.path_case(n, vectors, dtype)
    z = on_device(re, im)
    e_f, e_i = fc.normwise(cplx.fft(z), fwd), fc.normwise(cplx.ifft(z, norm="forward"), inv)
    print(f"fft n={n} vectors={vectors} {dtype}: path={hostfft.plan(n, vectors, dtype)[0]} forward {e_f:.3g} inverse {e_i:.3g}")
    assert e_f <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_f, e_i)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", fc.PATH_LENGTHS)
def test_every_path(n, dtype):
    check_paths(n, 3, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_partly_filled_last_workgroup(dtype):
    V = hostfft.plan(64, 1, dtype)[1]
    assert V == 32
    check_paths(64, V + 1, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_length_2_to_the_20(dtype):
    check_paths(1 << 20, 1, dtype)


# ---- 3. unit impulses: every output has modulus 1 --------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 100, 4096])
def test_unit_impulses(n):
    pos = [0, 1, n // 2 + 1, n - 1]
    re = torch.zeros(len(pos), n)
    re[torch.arange(len(pos)), torch.tensor(pos)] = 1.0
    im = torch.zeros_like(re)
    for fn, ours in (("fft", cplx.fft), ("ifft", lambda z: cplx.ifft(z, norm="forward"))):
        got = ours(on_device(re, im))
        ref = fc.reference(re, im, fn, norm="backward" if fn == "fft" else "forward")
        got = fc.c128(got.real, got.imag)
        assert float((got.abs() - 1).abs().max()) <= 1e-5
        assert float((got - ref).abs().max()) <= 1e-5


# ---- 4. the arithmetic of a vector does not depend on where it lies --------------------------------------------------
@pytest.mark.parametrize("n", [64, 100])
def test_layouts_give_identical_bits_in_one_launch_each(n, monkeypatch):
    re, im, fwd, _ = fc.path_case(n, 30, torch.float32)
    re, im, fwd = (t.reshape(2, 3, 5, n) for t in (re, im, fwd))
    calls = []

    def recording(name, *args):
        calls.append((name, args[0].value, args[1].value))
        return orig(name, *args)

    orig = hostfft.call
    monkeypatch.setattr(hostfft, "call", recording)
    results = []
    for layout in ("contiguous", "channels_last", "transposed", "sliced"):
        z = Cplx(relayout(re.to(DEV), layout), relayout(im.to(DEV), layout))
        del calls[:]
        y = cplx.fft(z)
        # exactly one launch, reading the planes where they lie: no layout copy
        assert calls == [("cplxamd_fft", z.real.data_ptr(), z.imag.data_ptr())], (layout, calls)
        del calls[:]
        y2 = cplx.fft2(z, dim=(0, 3))
        assert [c[0] for c in calls] == ["cplxamd_fft"] * 2 and calls[0][1:] == (z.real.data_ptr(), z.imag.data_ptr())
        results.append((y, y2))
    assert fc.normwise(results[0][0], fwd) <= fc.F32_TOL
    for y, y2 in results[1:]:
        assert torch.equal(y.real.contiguous(), results[0][0].real) and torch.equal(y.imag.contiguous(), results[0][0].imag)
        assert torch.equal(y2.real.contiguous(), results[0][1].real) and torch.equal(y2.imag.contiguous(), results[0][1].imag)


def test_planes_without_a_common_layout_are_copied_once():
    re, im, fwd, _ = fc.path_case(64, 30, torch.float32)
    z = Cplx(re.to(DEV), im.to(DEV).t().contiguous().t())
    assert z.real.stride() != z.imag.stride()
    assert fc.normwise(cplx.fft(z), fwd) <= fc.F32_TOL
    # more than three batch runs: every second index of four batch dims
    g = torch.Generator().manual_seed(5)
    big = torch.randn(2, 4, 4, 4, 4, 16, generator=g)
    vr, vi = big[0].to(DEV)[::2, ::2, ::2, ::2], big[1].to(DEV)[::2, ::2, ::2, ::2]
    assert len(hostfft._runs(vr.shape, vr.stride(), hostfft._dense_like(vr, 4, 16)[1], 4)) == 4
    ref = fc.reference(big[0, ::2, ::2, ::2, ::2], big[1, ::2, ::2, ::2, ::2], "fft")
    assert fc.normwise(cplx.fft(Cplx(vr, vi)), ref) <= fc.F32_TOL


# ---- 5. n / s and norm -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_padding_truncation_and_norms(dtype):
    re, im = fc.gaussian((5, 64), dtype, seed=21)
    z = on_device(re, im)
    for n in (96, 48, None):
        for norm in (None, "backward", "ortho", "forward"):
            for fn in ("fft", "ifft"):
                got = getattr(cplx, fn)(z, n=n, norm=norm)
                ref = fc.reference(re, im, fn, n=n, norm=norm)
                assert got.real.shape == ref.shape and got.real.dtype == dtype
                assert fc.normwise(got, ref) <= fc.tol(dtype), (n, norm, fn)
    for norm in (None, "ortho", "forward"):
        back = cplx.ifft(cplx.fft(z, norm=norm), norm=norm)
        assert fc.normwise(back, fc.c128(re, im)) <= fc.tol(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fftn_dims_and_shapes(dtype):
    re, im = fc.gaussian((6, 5, 8, 10), dtype, seed=22)
    z = on_device(re, im)
    for kw in (dict(dim=(0, 2)), dict(s=(4, 12)), dict(s=(9, 8, 7), dim=(1, 2, 0), norm="ortho"), dict(),
               dict(dim=(-1, 1), norm="forward")):
        for fn in ("fftn", "ifftn"):
            got, ref = getattr(cplx, fn)(z, **kw), fc.reference(re, im, fn, **kw)
            assert got.real.shape == ref.shape
            assert fc.normwise(got, ref) <= fc.tol(dtype), (fn, kw)
    for kw in (dict(), dict(s=(12, 6)), dict(dim=(0, 1), norm="ortho")):
        for fn in ("fft2", "ifft2"):
            assert fc.normwise(getattr(cplx, fn)(z, **kw), fc.reference(re, im, fn, **kw)) <= fc.tol(dtype), (fn, kw)
    sh = cplx.fftshift(cplx.fft2(z), dim=(-2, -1))
    assert fc.normwise(sh, torch.fft.fftshift(fc.reference(re, im, "fft2"), dim=(-2, -1))) <= fc.tol(dtype)


# ---- 6. bf16 planes are rounded once ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fft1000", "fft2_16", "fft2_64"])
def test_bf16_rounds_once(case):
    if case == "fft1000":
        re, im = fc.gaussian((4, 1000), torch.bfloat16, seed=31)
        got, ref = cplx.fft(on_device(re, im)), fc.reference(re, im, "fft")
    else:
        n = int(case.split("_")[1])
        re, im = fc.gaussian((3, n, n), torch.bfloat16, seed=32 + n)
        got, ref = cplx.fft2(on_device(re, im)), fc.reference(re, im, "fft2")
    assert got.real.dtype == torch.bfloat16 and got.imag.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(got, ref)
    print(f"bf16 {case}: {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} of the bound")
    assert bad == 0, (bad, worst)


# ---- 7. gradients against torch autograd through torch.fft in complex128 ---------------------------------------------
def loss_and_grads(fn, re, im, power, order, v=None):
    """first order: d sum|y|^power / d(re, im); second order: d <grad, v> / d(re, im)"""
    y = fn(re, im)
    loss = ((y[0].double() ** 2 + y[1].double() ** 2) ** (power // 2)).sum()
    if order == 1:
        return torch.autograd.grad(loss, (re, im))
    g = torch.autograd.grad(loss, (re, im), create_graph=True)
    return torch.autograd.grad((g[0].double() * v[0]).sum() + (g[1].double() * v[1]).sum(), (re, im))


def ours_fn(name, **kw):
    def fn(re, im):
        y = getattr(cplx, name)(Cplx(re, im), **kw)
        return y.real, y.imag
    return fn


def torch_fn(name, **kw):
    def fn(re, im):
        y = getattr(torch.fft, name)(torch.complex(re, im), **kw)
        return y.real, y.imag
    return fn


def grad_error(got, ref):
    return fc.normwise(torch.complex(got[0].double().cpu(), got[1].double().cpu()), torch.complex(ref[0], ref[1]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [8, 100, 1024, 2048])
def test_first_order_gradients(n, dtype):
    re, im = fc.gaussian((3, n), dtype, seed=41)
    for name, kw in (("fft", dict()), ("fft", dict(n=n + n // 2)), ("ifft", dict(n=n - n // 4)), ("fft", dict(norm="ortho")),
                     ("ifft", dict(norm="ortho", n=n + 1))):
        ref = loss_and_grads(torch_fn(name, dim=-1, **kw), re.double().requires_grad_(), im.double().requires_grad_(), 2, 1)
        got = loss_and_grads(ours_fn(name, **kw), re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_(), 2, 1)
        assert got[0].dtype == dtype and got[0].shape == re.shape
        assert grad_error(got, ref) <= fc.tol(dtype), (name, kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=["f32", "f64", "bf16"])
def test_fft2_gradients(dtype):
    re, im = fc.gaussian((2, 3, 16, 12), dtype, seed=42)
    ref = loss_and_grads(torch_fn("fft2"), re.double().requires_grad_(), im.double().requires_grad_(), 2, 1)
    got = loss_and_grads(ours_fn("fft2"), re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_(), 2, 1)
    assert got[0].dtype == dtype
    if dtype == torch.bfloat16:
        # y is rounded to bf16 once (2^-8 per entry), the loss' gradient 2 y inherits that, and the gradient, one more
        # transform in float32 (1e-5 each way), is rounded once more (2^-8)
        assert grad_error(got, ref) <= 2.0 ** -7 + 2e-5
    else:
        assert grad_error(got, ref) <= fc.tol(dtype)


@pytest.mark.parametrize("n", [8, 100])
def test_second_order_gradients(n):
    """float64 at 1e-11; float32 at 4 x the error of the same computation through torch's own complex64 torch.fft on
    the device (the factor covers another summation order).  Both values are printed (profiles/fft_parity.txt)."""
    re, im = fc.gaussian((3, n), torch.float64, seed=43)
    v = fc.gaussian((3, n), torch.float64, seed=44)
    ref = loss_and_grads(torch_fn("fft", dim=-1), re.clone().requires_grad_(), im.clone().requires_grad_(), 4, 2, v)
    vd = tuple(t.to(DEV) for t in v)
    got64 = loss_and_grads(ours_fn("fft"), re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_(), 4, 2, vd)
    assert grad_error(got64, ref) <= fc.F64_TOL
    re32, im32 = re.float(), im.float()
    ref32 = loss_and_grads(torch_fn("fft", dim=-1), re32.double().requires_grad_(), im32.double().requires_grad_(), 4, 2, v)
    ours = grad_error(loss_and_grads(ours_fn("fft"), re32.to(DEV).requires_grad_(), im32.to(DEV).requires_grad_(), 4, 2, vd),
                      ref32)
    theirs = grad_error(loss_and_grads(torch_fn("fft", dim=-1), re32.to(DEV).requires_grad_(), im32.to(DEV).requires_grad_(),
                                       4, 2, vd), ref32)
    print(f"fft_parity second order n={n}: ours {ours:.3e}  torch.fft complex64 {theirs:.3e}  ratio {ours / theirs:.2f}")
    assert ours <= 4 * theirs, (ours, theirs)


# ---- 8. reruns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 1024, 32768])
def test_reruns_are_bit_identical(n):
    re, im, _, _ = fc.path_case(n, 3, torch.float32)
    z = on_device(re, im)
    a, b = cplx.fft(z), cplx.fft(z)
    assert same_bits(a, b)
    assert same_bits(cplx.ifft(a), cplx.ifft(b))


# ---- 9. hipGraph -----------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    def step(re, im):
        y = cplx.fft2(Cplx(re, im))
        loss = (y.real.float() ** 2).sum() + (y.imag.float() ** 2).sum()
        return (y.real, y.imag) + torch.autograd.grad(loss, (re, im))

    re0, im0 = fc.gaussian((4, 8, 32, 32), torch.bfloat16, seed=51)
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
        re, im = fc.gaussian((4, 8, 32, 32), torch.bfloat16, seed=seed)
        with torch.no_grad():
            sre.copy_(re)
            sim.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_())
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


# ---- 10. errors on the device ----------------------------------------------------------------------------------------
def test_device_errors_and_empty_batches():
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.fft(Cplx(torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16)))
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.fft(Cplx(torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV)), n=(1 << 22) + 1)
    with pytest.raises(CplxAmdError):
        cplx.fft(Cplx(torch.zeros(4, 8, device=DEV, dtype=torch.float16), torch.zeros(4, 8, device=DEV, dtype=torch.float16)))
    empty = Cplx(torch.zeros(0, 64, device=DEV, requires_grad=True), torch.zeros(0, 64, device=DEV, requires_grad=True))
    out = cplx.fft(empty)
    assert out.real.shape == (0, 64) and out.imag.shape == (0, 64)
    (out.real.sum() + out.imag.sum()).backward()
    assert empty.real.grad.shape == (0, 64)
    assert cplx.fft(empty, n=100).real.shape == (0, 100)
