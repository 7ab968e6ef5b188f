"""cplx.exp / log / sin / cos / tan / sinh / cosh / tanh on the GPU (csrc/cplxfn.hip): values and gradients against
torch complex128, layouts, parity with the reference (tests/golden/cplx_fn.npz, scripts/gen_cplxfn_golden.py), large
arguments where the reference gives NaN, one library call each way, second order, hipGraph replay and 64-bit indexing.
u = 2^-24; |.| is the complex modulus per element."""
import numpy as np
import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")
U = 2.0 ** -24
TINY, HUGE = 1e-30, 1e37       # compare where the float32 result is neither subnormal-small nor near overflow


def _cplx():
    from cplxmodule_amd import cplx
    return cplx


def _ref(fn, zr, zi):
    """f(z) in complex128 on the device, z the given planes' values."""
    return getattr(torch, fn)(torch.complex(zr.detach().double(), zi.detach().double()))


def _deriv(fn, z):
    return {"exp": torch.exp, "log": lambda z: 1 / z, "sin": torch.cos, "cos": lambda z: -torch.sin(z),
            "tan": lambda z: 1 / torch.cos(z) ** 2, "sinh": torch.cosh, "cosh": torch.sinh,
            "tanh": lambda z: 1 / torch.cosh(z) ** 2}[fn](z)


def _for_autograd(fn, z):
    """f(z) in a spelling whose complex128 autograd does not cancel.  torch's tanh / tan backward forms 1 - tanh^2 /
    1 + tan^2, which is 0 in float64 once |Re z| (|Im z| for tan) passes ~19 while |f'| ~ 4 e^{-2|x|} is not; through
    tanh z = 1 - 2 / (e^{2z} + 1) the chain rule gives 4 e^{2z} / (e^{2z} + 1)^2, accurate everywhere."""
    if fn == "tanh":
        return 1 - 2 / (torch.exp(2 * z) + 1)
    if fn == "tan":
        return -1j * (1 - 2 / (torch.exp(2j * z) + 1))
    return getattr(torch, fn)(z)


def _check_values(fn, yr, yi, ref, dtype):
    got = torch.complex(yr.double(), yi.double()).reshape(-1)
    ref = ref.reshape(-1)
    mag = ref.abs()
    keep = torch.isfinite(ref) & (mag > TINY) & (mag < HUGE)
    assert keep.float().mean() > 0.9
    err = (got - ref).abs()
    if dtype == torch.float32:
        ok = err <= 16 * U * mag
        if fn == "log":
            ok |= ((got.real - ref.real).abs() <= 4 * U) & ((got.imag - ref.imag).abs() <= 16 * U * mag)
    else:
        ok = err <= 2.0 ** -8 * mag
    bad = keep & ~ok
    assert not bad.any(), (fn, dtype, int(bad.sum()), got[bad][:4].tolist(), ref[bad][:4].tolist())


def _points(shape, dtype, scale=2.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    zr = (scale * torch.randn(shape, generator=g, device=DEV)).to(dtype)
    zi = (scale * torch.randn(shape, generator=g, device=DEV)).to(dtype)
    return zr, zi


# ---- 1. values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 7, 4097, 1 << 20])
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_values_against_complex128(fn, n, dtype):
    zr, zi = _points((n,), dtype, seed=n)
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    assert y.real.dtype == dtype and y.real.shape == zr.shape
    _check_values(fn, y.real, y.imag, _ref(fn, zr, zi), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["channels_last", "transposed", "sliced"])
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_values_and_layout_of_non_contiguous_inputs(fn, layout, dtype):
    zr, zi = _points((3, 17, 9, 11), dtype, seed=5)
    if layout == "channels_last":
        zr, zi = zr.contiguous(memory_format=torch.channels_last), zi.contiguous(memory_format=torch.channels_last)
    elif layout == "transposed":
        zr, zi = zr.transpose(1, 3), zi.transpose(1, 3)
    else:
        zr, zi = zr[:, 1::2, :, 3:], zi[:, 1::2, :, 3:]
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    assert y.real.shape == zr.shape
    if layout == "channels_last":
        for t in (y.real, y.imag):
            assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
    else:
        assert y.real.is_contiguous() and y.imag.is_contiguous()
    _check_values(fn, y.real, y.imag, _ref(fn, zr, zi), dtype)


# ---- 2. layout: a channels-last input is handed to the kernel as it is ------------------------------------------------
def test_channels_last_makes_no_nchw_copy(monkeypatch):
    from cplxmodule_amd import ops
    zr, zi = _points((4, 16, 8, 8), torch.float32, seed=1)
    zr, zi = (t.contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in (zr, zi))
    seen, real_call = [], ops.call

    def spy(name, *args):
        seen.append((name, args))
        return real_call(name, *args)

    monkeypatch.setattr(ops, "call", spy)
    y = _cplx().tanh(_cplx().Cplx(zr, zi))
    g = torch.randn_like(zr)
    torch.autograd.grad((y.real * g).sum() + (y.imag * g).sum(), (zr, zi))
    assert [s[0] for s in seen] == ["cplxamd_cplx_fn_fwd", "cplxamd_cplx_fn_bwd"]
    assert seen[0][1][0].value == zr.data_ptr() and seen[0][1][1].value == zi.data_ptr()
    assert seen[1][1][0].value == zr.data_ptr() and seen[1][1][1].value == zi.data_ptr()
    assert y.real.is_contiguous(memory_format=torch.channels_last)


# ---- 3. gradients ----------------------------------------------------------------------------------------------------
def _grad_points(dtype):
    """A Gaussian cloud plus the saturated region of tanh / tan: |Re z| or |Im z| in [10, 40]."""
    g = torch.Generator(device=DEV).manual_seed(7)
    n = 4096
    sat = 10 + 30 * torch.rand(n, generator=g, device=DEV)
    sign = torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    other = 2 * torch.randn(n, generator=g, device=DEV)
    cloud_r, cloud_i = 2 * torch.randn(n, generator=g, device=DEV), 2 * torch.randn(n, generator=g, device=DEV)
    zr = torch.cat([cloud_r, sign * sat, other])
    zi = torch.cat([cloud_i, other, sign * sat])
    gr, gi = torch.randn(3 * n, generator=g, device=DEV), torch.randn(3 * n, generator=g, device=DEV)
    return zr.to(dtype), zi.to(dtype), gr.to(dtype), gi.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_gradients_against_complex128(fn, dtype):
    zr, zi, gr, gi = _grad_points(dtype)
    zr.requires_grad_(True)
    zi.requires_grad_(True)
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    dr, di = torch.autograd.grad((y.real, y.imag), (zr, zi), (gr, gi))
    assert dr.dtype == dtype
    xr, xi = zr.detach().double().requires_grad_(True), zi.detach().double().requires_grad_(True)
    w = _for_autograd(fn, torch.complex(xr, xi))
    rr, ri = torch.autograd.grad((w.real * gr.double()).sum() + (w.imag * gi.double()).sum(), (xr, xi))
    scale = _deriv(fn, torch.complex(xr, xi).detach()).abs() * torch.complex(gr.double(), gi.double()).abs()
    keep = torch.isfinite(scale) & (scale > TINY) & (scale < HUGE) & torch.isfinite(rr) & torch.isfinite(ri)
    assert keep.float().mean() > 0.5
    err = torch.complex(dr.double() - rr, di.double() - ri).abs()
    bound = (32 * U if dtype == torch.float32 else 2.0 ** -7) * scale
    bad = keep & ~(err <= bound)
    assert not bad.any(), (fn, dtype, int(bad.sum()), zr[bad][:3].tolist(), zi[bad][:3].tolist())


# ---- 4. parity with the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_matches_reference_golden(fn, golden):
    g = golden("cplx_fn")
    t = lambda k: torch.from_numpy(g[k].astype(np.float32)).to(DEV)  # noqa: E731   (inputs are float32 values)
    zr, zi = t("z_re").requires_grad_(True), t("z_im").requires_grad_(True)
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    dr, di = torch.autograd.grad((y.real, y.imag), (zr, zi), (t("g_re"), t("g_im")))
    for got, ref in ((y.real, fn + "_re"), (y.imag, fn + "_im"), (dr, fn + "_dre"), (di, fn + "_dim")):
        ref = g[ref]
        keep = np.isfinite(ref)
        got = got.detach().double().cpu().numpy()[keep]
        ref = ref[keep]
        assert np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref), (fn, np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---- 5. large arguments, extreme moduli, NaN -------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["tan", "tanh"])
def test_tan_tanh_large_arguments_are_finite(fn):
    g = torch.Generator(device=DEV).manual_seed(11)
    big = torch.cat([torch.logspace(0, 4, 200, device=DEV), torch.tensor([100.0, 1e4], device=DEV)])
    big = torch.cat([big, -big])
    small = 3 * torch.randn(big.numel(), generator=g, device=DEV)
    zr, zi = torch.cat([big, small]), torch.cat([small, big])
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    assert torch.isfinite(y.real).all() and torch.isfinite(y.imag).all()
    ref = _ref(fn, zr, zi)
    err = (torch.complex(y.real.double(), y.imag.double()) - ref).abs()
    assert (err <= 16 * U * ref.abs() + 1e-38).all()
    one = lambda a, b: getattr(_cplx(), fn)(_cplx().Cplx(torch.tensor([a], device=DEV), torch.tensor([b], device=DEV)))  # noqa: E731
    if fn == "tan":
        w = one(0.0, 100.0)
        assert abs(w.real.item()) < 1e-30 and w.imag.item() == 1.0          # the reference: nan
    else:
        w = one(100.0, 1.0)
        assert w.real.item() == 1.0 and abs(w.imag.item()) < 1e-30          # the reference: nan


def test_log_at_extreme_moduli_and_nan_propagation():
    fmax, tmin = float(np.finfo(np.float32).max), float(np.finfo(np.float32).smallest_subnormal)
    zr = torch.tensor([fmax, fmax, -fmax, tmin, tmin, 0.0, -tmin], device=DEV)
    zi = torch.tensor([fmax, 1.0, -fmax, tmin, 0.0, tmin, -tmin], device=DEV)
    y = _cplx().log(_cplx().Cplx(zr, zi))
    assert torch.isfinite(y.real).all() and torch.isfinite(y.imag).all()
    _check_values("log", y.real, y.imag, _ref("log", zr, zi), torch.float32)
    z0 = _cplx().log(_cplx().Cplx(torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)))
    assert z0.real.item() == -float("inf") and z0.imag.item() == 0.0
    nan = float("nan")
    zr = torch.tensor([nan, 1.0, nan, -2.0], device=DEV)
    zi = torch.tensor([1.0, nan, -0.5, nan], device=DEV)
    for fn in FUNCTIONS:
        for dtype in (torch.float32, torch.bfloat16):
            y = getattr(_cplx(), fn)(_cplx().Cplx(zr.to(dtype), zi.to(dtype)))
            assert torch.isnan(y.real).all() and torch.isnan(y.imag).all(), fn


# ---- 6. one library call each way ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_one_launch_each_way(fn, monkeypatch):
    from cplxmodule_amd import ops
    zr, zi = (t.requires_grad_(True) for t in _points((64, 33), torch.float32, seed=3))
    names, real_call = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    assert names == ["cplxamd_cplx_fn_fwd"]
    torch.autograd.grad((y.real.sum() + 2 * y.imag.sum()), (zr, zi))
    assert names == ["cplxamd_cplx_fn_fwd", "cplxamd_cplx_fn_bwd"]


# ---- 7. second order -------------------------------------------------------------------------------------------------
def _second_order(fn, zr, zi, gr, gi, hr, hi, via):
    zr, zi = zr.detach().clone().requires_grad_(True), zi.detach().clone().requires_grad_(True)
    yr, yi = via(fn, zr, zi)
    dr, di = torch.autograd.grad((yr * gr).sum() + (yi * gi).sum(), (zr, zi), create_graph=True)
    er, ei = torch.autograd.grad((dr * hr).sum() + (di * hi).sum(), (zr, zi))
    return [t.detach().double() for t in (yr, yi, dr, di, er, ei)]


def _via_cplx(fn, zr, zi):
    y = getattr(_cplx(), fn)(_cplx().Cplx(zr, zi))
    return y.real, y.imag


def _via_torch(fn, zr, zi):
    w = getattr(torch, fn)(torch.complex(zr, zi))
    return w.real, w.imag


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_second_order_float32_and_float64(fn):
    zr, zi = _points((1000,), torch.float64, scale=1.0, seed=9)
    gr, gi, hr, hi = _points((2, 1000), torch.float64, scale=1.0, seed=10)[0].unbind(0) + \
        _points((2, 1000), torch.float64, scale=1.0, seed=12)[0].unbind(0)
    ref = _second_order(fn, zr, zi, gr, gi, hr, hi, _via_torch)
    f = lambda t: t.float()  # noqa: E731
    got32 = _second_order(fn, f(zr), f(zi), f(gr), f(gi), f(hr), f(hi), _via_cplx)
    for a, b in zip(got32, ref):
        assert torch.linalg.norm(a - b) <= 1e-5 * torch.linalg.norm(b), fn
    got64 = _second_order(fn, zr, zi, gr, gi, hr, hi, _via_cplx)
    for a, b in zip(got64, ref):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), fn


# ---- 8. graph replay -------------------------------------------------------------------------------------------------
def test_graph_replay_of_tanh_is_bit_identical_to_eager():
    zr, zi = _points((257, 129), torch.float32, seed=4)
    x = _cplx().Cplx(zr.clone(), zi.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _cplx().tanh(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _cplx().tanh(x)
    for seed in (21, 22):
        nr, ni = _points((257, 129), torch.float32, scale=6.0, seed=seed)
        x.real.copy_(nr)
        x.imag.copy_(ni)
        graph.replay()
        torch.cuda.synchronize()
        eager = _cplx().tanh(_cplx().Cplx(nr, ni))
        assert torch.equal(y.real, eager.real) and torch.equal(y.imag, eager.imag)


# ---- 9. 64-bit indexing ----------------------------------------------------------------------------------------------
def test_bf16_call_past_2_31_elements():
    n, period = (1 << 31) + 5, 1 << 16
    pr, pi = _points((period,), torch.bfloat16, seed=13)
    small = _cplx().exp(_cplx().Cplx(pr, pi))
    zr = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    zi = torch.empty_like(zr)
    m = n // period
    for t, p in ((zr, pr), (zi, pi)):             # element e holds p[e % period]
        t[:m * period].view(m, period).copy_(p.expand(m, period))
        t[m * period:].copy_(p[:n - m * period])
    y = _cplx().exp(_cplx().Cplx(zr, zi))
    del zr, zi
    g = torch.Generator(device=DEV).manual_seed(5)
    idx = torch.cat([torch.randint(0, n, (4096,), generator=g, device=DEV),
                     torch.arange(n - 13, n, device=DEV),                        # the last 16-byte vector and the tail
                     torch.arange((1 << 31) - 4, (1 << 31) + 4, device=DEV), torch.tensor([0, 1, 7, 8], device=DEV)])
    for got, ref in ((y.real, small.real), (y.imag, small.imag)):
        a, b = got[idx].float(), ref[idx % period].float()
        assert torch.allclose(a, b, rtol=2.0 ** -7, atol=0), (a - b).abs().max()
    del y
    torch.cuda.empty_cache()
