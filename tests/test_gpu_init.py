"""nn.init on the device: the three kernels of csrc/init.hip through the C ABI against numpy in float64, and the device
route of cplx_polar_factor / cplx_trabelsi_independent_ under the bounds of tests/test_init_host.py."""
import math

import numpy as np
import pytest
import torch

from cplxmodule_amd import Cplx, _lib
from cplxmodule_amd._lib import call, ptr, stream_ptr
from cplxmodule_amd.nn import init

import init_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float64: _lib.F64}
PLANES = (torch.float32, torch.float64)


def workspace():
    return torch.empty(int(_lib.load().cplxamd_init_ws_bytes()), dtype=torch.uint8, device=DEV)


def planes(rs, shape, dtype, mean=0.0):
    a = torch.from_numpy(rs.randn(2, *shape) + mean).to(dtype)
    return a[0].contiguous().to(DEV), a[1].contiguous().to(DEV)


def f64(t):
    return t.double().cpu().numpy()


# ---- kernels through the C ABI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PLANES, ids=("f32", "f64"))
def test_init_moments(dtype):
    """[sum re, sum im, sum |z|^2] against math.fsum of the same values, relative 1e-12: float64 accumulation of n terms
    of one sign errs by at most n 2^-53 relative (1.2e-10 for the longest case, whose sums of squares are what the bound
    is about; observed far below), and the sums of the mean-1000 planes are where a float32 accumulator would lose
    everything.  n = 1, 63, 64, 65: around one wave; 4097: several blocks and a tail; the last case exceeds the block
    cap (grid-stride) and the odd offset takes the unvectorised loads."""
    rs = np.random.RandomState(0)
    ws, out = workspace(), torch.zeros(3, dtype=torch.float64, device=DEV)
    cases = [(n, mean, 0) for n in (1, 63, 64, 65, 4097) for mean in (0.0, 1000.0)] + [(4097, 1000.0, 1)]
    if dtype == torch.float32:
        cases.append((1024 * 256 * 4 + 1003, 0.0, 0))
    for n, mean, off in cases:
        re, im = planes(rs, (n + off,), dtype, mean)
        re, im = re[off:], im[off:]
        call("cplxamd_init_moments", ptr(re), ptr(im), n, CODE[dtype], ptr(out), ptr(ws), stream_ptr())
        x, y = f64(re), f64(im)
        want = [math.fsum(x), math.fsum(y), math.fsum(x * x + y * y)]
        got = out.tolist()
        print(f"moments {dtype} n={n} mean={mean} off={off}: rel {[abs(g - w) / abs(w) for g, w in zip(got, want)]}")
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        # the variance survives the cancellation: m2 / n - |mean|^2 of planes with mean 1000 and std 1
        if mean and n > 1:
            var = got[2] / n - (got[0] ** 2 + got[1] ** 2) / n ** 2
            np.testing.assert_allclose(var, x.var() + y.var(), rtol=1e-6)
    # deterministic: the same bits on a second launch
    first = out.clone()
    call("cplxamd_init_moments", ptr(re), ptr(im), n, CODE[dtype], ptr(out), ptr(ws), stream_ptr())
    assert torch.equal(first, out)


@pytest.mark.parametrize("dtype", PLANES, ids=("f32", "f64"))
def test_init_ns_poly(dtype):
    """P within 1 ulp (of the planes' type) of the exact a I + b G (observed: 0.5 ulp, one rounding everywhere) and
    ||G - I||_F^2 relative 1e-6 (float32 planes) / 1e-12 (float64), on a random Hermitian G; k = 600 exceeds the block cap."""
    rs = np.random.RandomState(1)
    ws, res = workspace(), torch.zeros(1, dtype=torch.float64, device=DEV)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for k in (1, 17, 64, 65, 600):
        a = rs.randn(k, k) + 1j * rs.randn(k, k)
        g = np.eye(k) + 0.1 * (a + a.conj().T)
        gr, gi = torch.from_numpy(g.real.copy()).to(dtype).to(DEV), torch.from_numpy(g.imag.copy()).to(dtype).to(DEV)
        for ca, cb in ((1.5, -0.5), (1.875, -1.25)):
            pr, pi = torch.full_like(gr, 9.0), torch.full_like(gi, 9.0)
            call("cplxamd_init_ns_poly", ptr(gr), ptr(gi), ptr(pr), ptr(pi), k, ca, cb, CODE[dtype], ptr(res), ptr(ws),
                 stream_ptr())
            hr, hi = gr.cpu().numpy(), gi.cpu().numpy()
            # the reference in extended precision (64-bit significand: b * g is exact there, the sum errs by 2^-64), NOT in
            # the planes' own arithmetic: numpy's two roundings are up to 1.5 ulp off where a + b g cancels
            assert np.finfo(np.longdouble).nmant >= 63
            ld = np.longdouble
            want_r = ld(cb) * hr.astype(ld) + ld(ca) * np.eye(k, dtype=ld)
            want_i = ld(cb) * hi.astype(ld)
            for got, want in ((pr.cpu().numpy(), want_r), (pi.cpu().numpy(), want_i)):
                assert got.dtype == npdt
                ulp = np.spacing(np.abs(want).astype(npdt)).astype(ld)
                err = np.abs(got.astype(ld) - want) / ulp
                print(f"ns_poly {dtype} k={k} a={ca} b={cb}: max error {float(err.max()):.3f} ulp")
                assert np.all(err <= 1.0)
            r2 = ((hr.astype(np.float64) - np.eye(k)) ** 2 + hi.astype(np.float64) ** 2).sum()
            np.testing.assert_allclose(res.item(), r2, rtol=1e-6 if dtype == torch.float32 else 1e-12)


def bf16_round(a):
    return torch.from_numpy(a.astype(np.float32)).bfloat16().double().numpy()


@pytest.mark.parametrize("in_dtype", PLANES, ids=("f32", "f64"))
def test_init_scale_store(in_dtype):
    """out = in * f, f from the moments on the device, against the same float64 arithmetic in numpy.  f goes through one
    division and one square root, each within an ulp of float64, so a float64 output (float64 planes) agrees to 4 * 2^-53
    relative; a float32 / bfloat16 output (float32 planes) is that product rounded once, which can differ from numpy's
    rounding (bfloat16: through float32 here) by one ulp of the output type only where the product sits next to a tie."""
    rs = np.random.RandomState(2)
    ws = workspace()
    stat = torch.zeros(8, dtype=torch.float64, device=DEV)
    for rows, cols in ((5, 3), (65, 130)):
        ir, ii = planes(rs, (rows, cols), in_dtype, mean=0.25)
        n = rows * cols
        call("cplxamd_init_moments", ptr(ir), ptr(ii), n, CODE[in_dtype], ptr(stat[0:3]), ptr(ws), stream_ptr())
        m0, m1, m2 = stat[0:3].tolist()
        z = f64(ir) + 1j * f64(ii)
        np.testing.assert_allclose(1 / np.sqrt(m2 / n - (m0 * m0 + m1 * m1) / n ** 2), 1 / z.std(), rtol=1e-12)
        factors = {_lib.INIT_SCALE_NORM: 1.0 / math.sqrt(m2), _lib.INIT_SCALE_STD: 0.125 / math.sqrt(m2 / n - (m0 * m0 + m1 * m1) / n ** 2),
                   _lib.INIT_SCALE_CONST: -3.0}
        targets = {_lib.INIT_SCALE_NORM: 1.0, _lib.INIT_SCALE_STD: 0.125, _lib.INIT_SCALE_CONST: -3.0}
        for mode, f in factors.items():
            for transpose in (0, 1):
                want = z.conj().T * f if transpose else z * f
                for out_dtype in ((torch.float32, torch.bfloat16) if in_dtype == torch.float32 else (torch.float64,)):
                    o_r, o_i = (torch.full(want.shape, 7.0, dtype=out_dtype, device=DEV) for _ in range(2))
                    stat[4] = 5.0
                    call("cplxamd_init_scale_store", ptr(ir), ptr(ii), ptr(o_r), ptr(o_i), rows, cols, transpose, mode,
                         targets[mode], None if mode == _lib.INIT_SCALE_CONST else ptr(stat[0:3]), ptr(stat[4:5]), CODE[in_dtype],
                         CODE[out_dtype], stream_ptr())
                    assert stat[4].item() == 0.0
                    for got, w in ((f64(o_r), want.real), (f64(o_i), want.imag)):
                        if out_dtype == torch.float64:
                            np.testing.assert_allclose(got, w, rtol=4 * C.U[torch.float64], atol=0)
                        elif out_dtype == torch.float32:
                            np.testing.assert_allclose(got, w.astype(np.float32).astype(np.float64), rtol=2.0 ** -23, atol=0)
                            assert (got == w.astype(np.float32)).mean() >= 0.99
                        else:
                            # one bfloat16 ulp (8 significant bits: 2^(e - 7) for a value in [2^e, 2^(e + 1)))
                            ulp = 2.0 ** (np.floor(np.log2(np.abs(bf16_round(w)))) - 7)
                            assert np.all(np.abs(got - bf16_round(w)) <= ulp)
                            assert (got == bf16_round(w)).mean() >= 0.99
    # a factor that does not exist: nothing is stored, the status says so
    ir, ii = planes(rs, (5, 3), in_dtype)
    bad = [(_lib.INIT_SCALE_NORM, [0.0, 0.0, 0.0]), (_lib.INIT_SCALE_STD, [15.0, 0.0, 15.0]),      # all ones: variance 0
           (_lib.INIT_SCALE_NORM, [0.0, 0.0, float("nan")]), (_lib.INIT_SCALE_STD, [0.0, 0.0, float("inf")])]
    for transpose in (0, 1):
        for mode, mom in bad:
            stat[0:3] = torch.tensor(mom, dtype=torch.float64)
            stat[4] = 5.0
            o_r, o_i = (torch.full((15,), 7.0, dtype=in_dtype, device=DEV) for _ in range(2))
            call("cplxamd_init_scale_store", ptr(ir), ptr(ii), ptr(o_r), ptr(o_i), 5, 3, transpose, mode, 1.0, ptr(stat[0:3]),
                 ptr(stat[4:5]), CODE[in_dtype], CODE[in_dtype], stream_ptr())
            assert stat[4].item() == 1.0 and bool((o_r == 7.0).all()) and bool((o_i == 7.0).all())


# ---- the device route ----------------------------------------------------------------------------------------------------
WEIGHTS = (((48, 80), torch.float32), ((80, 48), torch.float32), ((8, 6, 3, 3), torch.float32), ((3, 7, 5, 5), torch.float64),
           ((48, 80), torch.bfloat16), ((8, 6, 3, 3), torch.bfloat16))


@pytest.mark.parametrize("shape,dtype", WEIGHTS, ids=lambda v: C.tag(v) if isinstance(v, tuple) else str(v)[6:])
def test_all_five_run_and_the_orthogonal_one_is_orthogonal(shape, dtype):
    torch.manual_seed(17)
    for name in C.NEW:
        w = Cplx.empty(*shape, dtype=dtype, device=DEV)
        assert getattr(init, name)(w) is w
        assert w.real.is_cuda and np.isfinite(C.c128(w)).all() and np.abs(C.c128(w)).max() > 0, name
    for kind in C.KINDS + ("Glorot", "XAVIER", "KaiMing", "HE"):
        w = Cplx.empty(*shape, dtype=dtype, device=DEV)
        C.check_independent(init.cplx_trabelsi_independent_(w, kind=kind), kind)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
def test_polar_factor_against_the_float64_svd(dtype):
    """max |M - U V^H| <= 64 u (float32) / 128 u (float64) for the device route AND for the host route on the same Z (they
    need not be bit-equal).  The test prints each figure before it asserts.  Observed on an MI355X: device route at most
    9.3 u in float32 ((33, 33)) and 14.2 u in float64 ((33, 33)); host route on the same Z, on that machine's host, 6.4 u and 10.8 u (13.4 u
    in float64 on another host: another BLAS summation order); the two
    routes differ by at most 6.8 u and 13.7 u."""
    for i, shape in enumerate(C.POLAR_SHAPES):
        z = C.gaussian(shape, dtype, 100 + i)
        zd = z.to(DEV)
        md = init.cplx_polar_factor(zd)
        assert md.real.is_cuda
        err_d, err_h = C.polar_error(zd, md), C.polar_error(z, init.cplx_polar_factor(z))
        both = np.abs(C.c128(md) - C.c128(init.cplx_polar_factor(z))).max() / C.U[dtype]
        print(f"polar {shape} {dtype}: device {err_d:.2f} u, host {err_h:.2f} u, device - host {both:.2f} u")
        assert err_d <= C.POLAR_BOUND[dtype] and err_h <= C.POLAR_BOUND[dtype], shape
    m = C.c128(init.cplx_polar_factor(C.gaussian((130, 67), dtype, 7).to(DEV)))
    assert np.abs(m.conj().T @ m - np.eye(67)).max() <= 32 * C.U[dtype]
    m = C.c128(init.cplx_polar_factor(C.gaussian((21, 25), dtype, 8).to(DEV)))
    assert np.abs(m @ m.conj().T - np.eye(21)).max() <= 32 * C.U[dtype]


def test_polar_factor_of_bf16_and_of_a_strided_input():
    z = C.gaussian((21, 25), torch.bfloat16, 9).to(DEV)
    m = init.cplx_polar_factor(z)
    assert m.dtype == torch.bfloat16 and m.shape == z.shape and m.real.is_cuda
    assert np.abs(C.c128(m) - C.svd_polar(z)).max() <= C.U[torch.bfloat16] + 64 * C.U[torch.float32]
    base = C.gaussian((25, 21), torch.float64, 10).to(DEV)
    assert np.array_equal(C.c128(init.cplx_polar_factor(base.t())),
                          C.c128(init.cplx_polar_factor(Cplx(base.real.t().contiguous(), base.imag.t().contiguous()))))


def test_same_seed_same_draw_next_call_another():
    C.check_seeding(DEV)


def test_writes_reach_the_parameters_of_layers():
    C.check_layers(DEV)


def test_non_contiguous_tensors_are_filled_in_place():
    C.check_strided(DEV)


def test_requires_grad_is_kept_and_no_graph_is_recorded():
    C.check_autograd_flags(DEV)


def test_one_dimensional_tensors_and_bad_kinds_are_rejected():
    C.check_rejections(DEV)


def test_polar_factor_raises_on_zero_nonfinite_and_rank_deficient_input():
    C.check_polar_failures(DEV)


def test_a_draw_over_the_step_cap_is_drawn_again(monkeypatch):
    C.check_redraw(DEV, monkeypatch)


def test_on_a_side_stream():
    z = C.gaussian((130, 67), torch.float32, 12).to(DEV)
    w = Cplx.empty(80, 48, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m = init.cplx_polar_factor(z)
        torch.manual_seed(31)
        init.cplx_trabelsi_independent_(w)
    side.synchronize()
    assert C.polar_error(z, m) <= C.POLAR_BOUND[torch.float32]
    C.check_independent(w)
    ref = Cplx.empty(80, 48, device=DEV)
    torch.manual_seed(31)
    init.cplx_trabelsi_independent_(ref)
    torch.cuda.synchronize()
    assert np.array_equal(C.c128(w), C.c128(ref))


def test_initialised_layer_runs_forward():
    from cplxmodule_amd.nn import CplxLinear
    layer = CplxLinear(96, 64).to(DEV)
    torch.manual_seed(3)
    init.cplx_trabelsi_independent_(layer.weight, kind="he")
    m = C.matrix_of(layer.weight)
    assert C.gram_defect(m) <= C.orthogonality_bound(torch.float32)
    np.testing.assert_allclose(m.std(), 1 / np.sqrt(64), rtol=1e-5)
    x = Cplx(torch.randn(10, 96, device=DEV), torch.randn(10, 96, device=DEV))
    y = layer(x)
    assert y.shape == (10, 64) and bool(torch.isfinite(y.real).all()) and bool(torch.isfinite(y.imag).all())
    want = C.c128(x) @ C.c128(layer.weight).T + C.c128(layer.bias)
    np.testing.assert_allclose(C.c128(y), want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
