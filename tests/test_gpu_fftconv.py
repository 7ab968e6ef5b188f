"""cplx.fftconvolve on the GPU (csrc/fftconv.hip, fftconv_wgrad.hip through cplxmodule_amd/fftconv.py): bit-exact on
integer operands with 4-point blocks (forward and both gradients), every path against complex128, block seams, modes,
broadcasting and layouts (identical bits, one launch, no copy), the single rounding of bf16, gradients of first and
second order against torch's CPU autograd, bit-identical reruns, hipGraph replay and the errors raised on the device.
Cases, references and bounds: fftconv_cases.py."""
import functools

import pytest
import torch

import fft_cases as fc
import fftconv_cases as cc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import fftconv as hostconv
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
IDS = ["f32", "bf16", "f64"]
WIDE = [torch.float32, torch.float64]
WIDE_IDS = ["f32", "f64"]


def operand(re, im, dtype, grad=False):
    """planes on the CPU -> a Cplx (im given) or a real tensor on the device"""
    re = re.to(dtype).to(DEV).requires_grad_(grad)
    return re if im is None else Cplx(re, im.to(dtype).to(DEV).requires_grad_(grad))


def planes(y):
    return (y, None) if torch.is_tensor(y) else (y.real, y.imag)


def assert_equal(got, ref, dtype):
    """`got` (Cplx or real tensor) EQUALS the complex128 reference rounded once to dtype"""
    gr, gi = planes(got)
    assert gr.dtype == dtype and gr.shape == ref.shape and gr.is_contiguous()
    assert torch.equal(gr.double().cpu(), ref.real.to(dtype).double()), "real plane"
    if gi is None:
        assert not bool(ref.imag.any())
    else:
        assert torch.equal(gi.double().cpu(), ref.imag.to(dtype).double()), "imaginary plane"


def error(got, ref):
    gr, gi = planes(got)
    return fc.normwise(cc.c128((gr, gi)), ref)


# ---- 1. exact: integers, 4-point blocks (twiddles +-1, +-i) -------------------------------------------------------------
KINDS = {"cc": (True, True), "rc": (False, True), "cr": (True, False), "rr": (False, False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", cc.EXACT + cc.EXACT_BLOCKS, ids=lambda c: "x".join(map(str, c)))
def test_exact_forward(case, dtype):
    xr, xi, hr, hi = cc.exact_case(*case)
    for kind, (xc, hc) in KINDS.items():
        x64, h64 = torch.complex(xr, xi if xc else 0 * xi), torch.complex(hr, hi if hc else 0 * hi)
        x, h = operand(xr, xi if xc else None, dtype), operand(hr, hi if hc else None, dtype)
        for mode in cc.MODES:
            ref = cc.integer_reference(x64, h64, mode)
            assert float(ref.abs().max()) < 2 ** 24
            assert_equal(hostconv.fftconvolve(x, h, mode, log_l=cc.EXACT_LOG_L), ref, dtype)
            # the longer operand second: the same full result; "same" and "valid" by their own definition
            swapped = cc.reference(h64.expand(x64.shape[0], -1), x64, mode)
            swapped = torch.complex(swapped.real.round(), swapped.imag.round())
            assert_equal(hostconv.fftconvolve(h, x, mode, log_l=cc.EXACT_LOG_L), swapped, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", cc.EXACT + cc.EXACT_BLOCKS, ids=lambda c: "x".join(map(str, c)))
def test_exact_first_order_gradients(case, dtype):
    """loss = sum w_r Re y + w_i Im y with integer weights: the gradients are integer correlations, through P1 (conj)
    for the long operand and P2 for the filter; they EQUAL torch's complex128 gradients (bf16: rounded once).  The same
    cases as the forward: every kind of operand pair (a real operand's gradient is the real part: the null output
    plane), all modes, both operand orders."""
    xr, xi, hr, hi = cc.exact_case(*case)
    zero = lambda t: torch.zeros_like(t)
    for kind, (xc, hc) in KINDS.items():
        xs, hs = (xr, xi if xc else None), (hr, hi if hc else None)
        for mode in cc.MODES:
            for x_first in (True, False):
                cpu = [[t if t is None else t.clone().requires_grad_() for t in pl] for pl in (xs, hs)]
                x64, h64 = (torch.complex(pl[0], zero(pl[0]) if pl[1] is None else pl[1]) for pl in cpu)
                y = cc.reference(x64, h64, mode) if x_first else cc.reference(h64, x64, mode)
                wr, wi = cc.integers(y.shape, 90), cc.integers(y.shape, 91)
                leaves = [t for pl in cpu for t in pl if t is not None]
                loss = (y.real * wr).sum() + (0 if not (xc or hc) else (y.imag * wi).sum())
                ref = torch.autograd.grad(loss, leaves)
                dev = [[t if t is None else t.to(dtype).to(DEV).requires_grad_() for t in pl] for pl in (xs, hs)]
                x, h = (pl[0] if pl[1] is None else Cplx(*pl) for pl in dev)
                y = hostconv.fftconvolve(x, h, mode, log_l=cc.EXACT_LOG_L) if x_first else \
                    hostconv.fftconvolve(h, x, mode, log_l=cc.EXACT_LOG_L)
                yr, yi = planes(y)
                assert (yi is None) == (not (xc or hc))
                loss = (yr * wr.to(dtype).to(DEV)).sum() + (0 if yi is None else (yi * wi.to(dtype).to(DEV)).sum())
                got = torch.autograd.grad(loss, [t for pl in dev for t in pl if t is not None])
                for g, r in zip(got, ref):
                    assert g.dtype == dtype and g.shape == r.shape and float(r.abs().max()) < 2 ** 24
                    assert torch.equal(g.double().cpu(), r.round().to(dtype).double()), (kind, mode, x_first)


# ---- 2. every path ---------------------------------------------------------------------------------------------------
PATHS = [(100, 7), (1000, 33), (5000, 255), (5000, 257), (20000, 512), (20000, 2048), (20000, 4096), (6000, 5000), (4096, 4096)]


@functools.lru_cache(maxsize=None)
def path_case(a_len, k, dtype, rows=2):
    """(xr, xi, hr, hi) Gaussian planes on the CPU rounded to dtype, x [rows, A], h [K]; and the full reference"""
    xr, xi = cc.gaussian((rows, a_len), dtype, 3 * a_len + k), cc.gaussian((rows, a_len), dtype, 3 * a_len + k + 1)
    hr, hi = cc.gaussian((k,), dtype, 5 * a_len + k), cc.gaussian((k,), dtype, 5 * a_len + k + 1)
    return xr, xi, hr, hi, cc.reference(cc.c128((xr, xi)), cc.c128((hr, hi)), "full")


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("case", PATHS, ids=lambda c: "x".join(map(str, c)))
def test_every_path(case, dtype):
    a_len, k = case
    xr, xi, hr, hi, full = path_case(a_len, k, dtype)
    y = cplx.fftconvolve(operand(xr, xi, dtype), operand(hr, hi, dtype))
    err = error(y, full)
    print(f"fftconv_parity forward A={a_len} K={k} {dtype} path={hostconv.plan(a_len, k, 0, a_len + k - 1)['path']}: {err:.3g}")
    assert y.real.dtype == dtype and err <= fc.tol(dtype)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("a_len", cc.SEAMS_A)
def test_block_seams(a_len, dtype):
    xr, xi, hr, hi, full = path_case(a_len, cc.SEAMS_K, dtype, rows=3)
    x, h = operand(xr, xi, dtype), operand(hr, hi, dtype)
    for mode in cc.MODES:
        start, length = cc.window(a_len, cc.SEAMS_K, mode)
        assert error(cplx.fftconvolve(x, h, mode), full[..., start:start + length]) <= fc.tol(dtype), mode


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("k", [6, 7, 32, 33])
def test_modes(k, dtype):
    """all three modes, even and odd K, both operand orders"""
    xr, xi, hr, hi, _ = path_case(300, k, dtype)
    x, h = operand(xr, xi, dtype), operand(hr, hi, dtype)
    x64, h64 = cc.c128((xr, xi)), cc.c128((hr, hi))
    for mode in cc.MODES:
        a, b = cplx.fftconvolve(x, h, mode), cplx.fftconvolve(h, x, mode)
        ra, rb = cc.reference(x64, h64, mode), cc.reference(h64, x64, mode)
        assert a.real.shape == ra.shape and b.real.shape == rb.shape
        assert error(a, ra) <= fc.tol(dtype) and error(b, rb) <= fc.tol(dtype), mode


# ---- 3. broadcast and layout -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hshape", [(3,), (), (2, 1), (2, 3)], ids=lambda s: "h" + "x".join(map(str, s)))
def test_broadcast(hshape):
    a_len, k = 700, 9
    xr, xi = cc.gaussian((2, 3, a_len), torch.float32, 11), cc.gaussian((2, 3, a_len), torch.float32, 12)
    hr, hi = cc.gaussian(hshape + (k,), torch.float32, 13), cc.gaussian(hshape + (k,), torch.float32, 14)
    y = cplx.fftconvolve(operand(xr, xi, torch.float32), operand(hr, hi, torch.float32), "same")
    assert error(y, cc.reference(cc.c128((xr, xi)), cc.c128((hr, hi)), "same")) <= fc.F32_TOL
    # a broadcast signal: x [1, A] with h [4, K]
    hr, hi = cc.gaussian((4, k), torch.float32, 15), cc.gaussian((4, k), torch.float32, 16)
    y = cplx.fftconvolve(operand(xr[:1, 0], xi[:1, 0], torch.float32), operand(hr, hi, torch.float32))
    assert y.real.shape == (4, a_len + k - 1)
    assert error(y, cc.reference(cc.c128((xr[:1, 0], xi[:1, 0])), cc.c128((hr, hi)), "full")) <= fc.F32_TOL
    with pytest.raises(RuntimeError):
        cplx.fftconvolve(operand(xr, xi, torch.float32), operand(hr, hi, torch.float32))


def test_layouts_give_identical_bits_in_one_launch(monkeypatch):
    a_len, k = 1500, 33
    xr, xi = (cc.gaussian((4, 3, a_len), torch.float32, s).to(DEV) for s in (21, 22))
    hr, hi = (cc.gaussian((3, k), torch.float32, s).to(DEV) for s in (23, 24))
    calls = []

    def recording(name, *args):
        calls.append((name,) + tuple(None if a is None else a.value for a in args[:4]))
        return orig(name, *args)

    orig = hostconv.call
    monkeypatch.setattr(hostconv, "call", recording)

    def sliced(t):                                        # every second element of a buffer twice as long
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=DEV)
        buf[..., ::2] = t
        return buf[..., ::2]

    def transposed(t):                                    # the leading dims swapped in memory
        return t.transpose(0, 1).contiguous().transpose(0, 1)

    base = cplx.fftconvolve(Cplx(xr, xi), Cplx(hr, hi))
    for name, fx, fh in (("sliced", sliced, sliced), ("transposed", transposed, lambda t: t),
                         ("expanded filter", lambda t: t, lambda t: t[None].expand(4, 3, k))):
        x, h = Cplx(fx(xr), fx(xi)), Cplx(fh(hr), fh(hi))
        assert x.real.stride() != xr.stride() or h.real.stride() != hr.stride()
        del calls[:]
        y = cplx.fftconvolve(x, h)
        # one P1 launch that reads the planes at their own addresses: no layout copy
        assert calls == [("cplxamd_fftconv", x.real.data_ptr(), x.imag.data_ptr(), h.real.data_ptr(), h.imag.data_ptr())], name
        assert torch.equal(y.real, base.real) and torch.equal(y.imag, base.imag), name
    # an expanded SIGNAL shares its one row; the bits are those of its contiguous copy
    x1 = Cplx(xr[0, :1].expand(3, a_len), xi[0, :1].expand(3, a_len))
    del calls[:]
    y = cplx.fftconvolve(x1, Cplx(hr, hi))
    assert [c[:3] for c in calls] == [("cplxamd_fftconv", x1.real.data_ptr(), x1.imag.data_ptr())]
    yc = cplx.fftconvolve(Cplx(x1.real.contiguous(), x1.imag.contiguous()), Cplx(hr, hi))
    assert torch.equal(y.real, yc.real) and torch.equal(y.imag, yc.imag)
    # planes that share no layout, and more than three batch runs, are copied once and still right
    z = Cplx(xr, xi.transpose(0, 1).contiguous().transpose(0, 1))
    y = cplx.fftconvolve(z, Cplx(hr, hi))
    assert torch.equal(y.real, base.real) and torch.equal(y.imag, base.imag)
    big = cc.gaussian((4, 4, 4, 4, 64), torch.float32, 25).to(DEV)
    v = big[::2, ::2, ::2, ::2]
    y = cplx.fftconvolve(v, hr[0])
    assert error(y, cc.reference(cc.c128(v), cc.c128(hr[0]), "full")) <= fc.F32_TOL


# ---- 4. bf16 rounds once ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1000, 33), (20000, 512)], ids=lambda c: "x".join(map(str, c)))
def test_bf16_rounds_once(case):
    a_len, k = case
    xr, xi, hr, hi, full = path_case(a_len, k, torch.bfloat16)
    y = cplx.fftconvolve(operand(xr, xi, torch.bfloat16), operand(hr, hi, torch.bfloat16))
    assert y.real.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(y, full)
    print(f"fftconv_parity bf16 A={a_len} K={k}: {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} of the bound")
    assert bad == 0


# ---- 5. gradients against torch's CPU autograd in complex128 ---------------------------------------------------------
def loss_of(y, wr, wi, power=2):
    yr, yi = planes(y)
    out = ((yr.double() ** power) * wr).sum()
    return out if yi is None else out + ((yi.double() ** power) * wi).sum()


def ref_loss(x, h, mode, wr, wi, power, real_out):
    y = cc.reference(x, h, mode)
    out = ((y.real ** power) * wr).sum()
    return out if real_out else out + ((y.imag ** power) * wi).sum()


def gradient_errors(xs, hs, mode, dtype, xshape_note=""):
    """xs, hs: (re, im or None) CPU planes of dtype.  -> norm-wise errors of d/dx and d/dh of a weighted sum of squares"""
    leaves = [t.double().clone().requires_grad_() for t in xs + hs if t is not None]
    it = iter(leaves)
    x64 = [next(it) if t is not None else None for t in xs]
    h64 = [next(it) if t is not None else None for t in hs]
    cx = torch.complex(x64[0], x64[1] if x64[1] is not None else torch.zeros_like(x64[0]))
    ch = torch.complex(h64[0], h64[1] if h64[1] is not None else torch.zeros_like(h64[0]))
    shape = cc.reference(cx.detach(), ch.detach(), mode).shape
    wr, wi = cc.gaussian(shape, torch.float64, 61), cc.gaussian(shape, torch.float64, 62)
    real_out = xs[1] is None and hs[1] is None
    ref = torch.autograd.grad(ref_loss(cx, ch, mode, wr, wi, 2, real_out), leaves)
    dev = [t.to(DEV).requires_grad_() for t in xs + hs if t is not None]
    it = iter(dev)
    xd = [next(it) if t is not None else None for t in xs]
    hd = [next(it) if t is not None else None for t in hs]
    y = cplx.fftconvolve(xd[0] if xd[1] is None else Cplx(*xd), hd[0] if hd[1] is None else Cplx(*hd), mode)
    got = torch.autograd.grad(loss_of(y, wr.to(DEV), wi.to(DEV)), dev)
    errs = []
    for g, r in zip(got, ref):
        assert g.dtype == dtype and g.shape == r.shape
        errs.append(float(torch.linalg.norm(g.double().cpu() - r) / torch.linalg.norm(r)))
    return errs


GRAD_PATHS = [(100, 7), (1000, 33), (5000, 255), (5000, 257), (4096, 2048), (4096, 4096), (4500, 4100)]


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("case", GRAD_PATHS, ids=lambda c: "x".join(map(str, c)))
def test_first_order_gradients_on_every_path(case, dtype):
    a_len, k = case
    xr, xi, hr, hi, _ = path_case(a_len, k, dtype)
    errs = gradient_errors((xr, xi), (hr, hi), "full", dtype)
    print(f"fftconv_parity gradients A={a_len} K={k} {dtype}: " + " ".join(f"{e:.3g}" for e in errs))
    assert max(errs) <= fc.tol(dtype), errs


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("mode", cc.MODES)
def test_first_order_gradients_modes_filters_and_kinds(mode, dtype):
    a_len, k = 1200, 33
    xr, xi = cc.gaussian((2, 3, a_len), dtype, 31), cc.gaussian((2, 3, a_len), dtype, 32)
    for hshape in ((), (3,), (2, 3)):                    # one shared filter, one per channel, one per row
        hr, hi = cc.gaussian(hshape + (k,), dtype, 33), cc.gaussian(hshape + (k,), dtype, 34)
        for kind, (xc, hc) in KINDS.items():
            errs = gradient_errors((xr, xi if xc else None), (hr, hi if hc else None), mode, dtype)
            assert max(errs) <= fc.tol(dtype), (hshape, kind, errs)
    # the longer operand second
    errs = gradient_errors((cc.gaussian((3, k), dtype, 35), None), (xr[0], xi[0]), mode, dtype)
    assert max(errs) <= fc.tol(dtype), errs


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("case", [(100, 7), (1000, 33)], ids=lambda c: "x".join(map(str, c)))
def test_hessian_vector_products(case, dtype):
    """d <d sum |y|^4 / d(x, h), v> / d(x, h): the second order runs P1 and P2 on each other's gradients"""
    a_len, k = case
    xr, xi, hr, hi, _ = path_case(a_len, k, dtype)
    vs = [cc.gaussian(t.shape, torch.float64, 70 + i) for i, t in enumerate((xr, xi, hr, hi))]

    def hvp(leaves, fn, vecs):
        y = fn(*leaves)
        yr, yi = planes(y) if not (torch.is_tensor(y) and y.is_complex()) else (y.real, y.imag)
        loss = ((yr.double() ** 2 + yi.double() ** 2) ** 2).sum()
        g = torch.autograd.grad(loss, leaves, create_graph=True)
        return torch.autograd.grad(sum((a.double() * v).sum() for a, v in zip(g, vecs)), leaves)

    ref = hvp([t.double().clone().requires_grad_() for t in (xr, xi, hr, hi)],
              lambda a, b, c, d: cc.reference(torch.complex(a, b), torch.complex(c, d), "full"), vs)
    got = hvp([t.to(DEV).requires_grad_() for t in (xr, xi, hr, hi)],
              lambda a, b, c, d: cplx.fftconvolve(Cplx(a, b), Cplx(c, d)), [v.to(DEV) for v in vs])
    errs = [float(torch.linalg.norm(g.double().cpu() - r) / torch.linalg.norm(r)) for g, r in zip(got, ref)]
    print(f"fftconv_parity second order A={a_len} K={k} {dtype}: " + " ".join(f"{e:.3g}" for e in errs))
    assert max(errs) <= fc.tol(dtype), errs


# ---- 6. reruns, hipGraph, errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1000, 33), (5000, 257), (20000, 4096)], ids=lambda c: "x".join(map(str, c)))
def test_reruns_are_bit_identical(case):
    a_len, k = case
    xr, xi, hr, hi, _ = path_case(a_len, k, torch.float32)

    def run():
        leaves = [t.to(DEV).requires_grad_() for t in (xr, xi, hr, hi)]
        y = cplx.fftconvolve(Cplx(leaves[0], leaves[1]), Cplx(leaves[2], leaves[3]))
        return (y.real, y.imag) + torch.autograd.grad((y.real ** 2).sum() + (y.imag ** 2).sum(), leaves)

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_graph_replay_equals_eager():
    def step(xr, xi, h):
        y = cplx.fftconvolve(Cplx(xr, xi), h, "same")
        loss = (y.real.float() ** 2).sum() + (y.imag.float() ** 2).sum()
        return (y.real, y.imag) + torch.autograd.grad(loss, (xr, xi, h))

    shape, k = (4, 3, 3000), 33
    inputs = [cc.gaussian(shape, torch.bfloat16, 81).to(DEV).requires_grad_(), cc.gaussian(shape, torch.bfloat16, 82).to(DEV).requires_grad_(),
              cc.gaussian((3, k), torch.bfloat16, 83).to(DEV).requires_grad_()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*inputs)                                     # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*inputs)
    for seed in (84, 87):
        fresh = [cc.gaussian(t.shape, torch.bfloat16, seed + i).to(DEV) for i, t in enumerate(inputs)]
        with torch.no_grad():
            for t, f in zip(inputs, fresh):
                t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*[f.requires_grad_() for f in fresh])
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


def test_device_errors_and_empty_batches():
    x = torch.zeros(4, 64, device=DEV)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.fftconvolve(x, torch.zeros(8, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(CplxAmdError):
        cplx.fftconvolve(x.half(), torch.zeros(8, device=DEV, dtype=torch.float16))
    with pytest.raises(CplxAmdError):
        cplx.fftconvolve(x, torch.zeros(8))
    with pytest.raises(CplxAmdError, match="2\\^22"):
        cplx.fftconvolve(torch.zeros(1, (1 << 22) - 4000, device=DEV), torch.zeros(5000, device=DEV))
    empty = Cplx(torch.zeros(0, 64, device=DEV, requires_grad=True), torch.zeros(0, 64, device=DEV, requires_grad=True))
    h = torch.zeros(8, device=DEV, requires_grad=True)
    out = cplx.fftconvolve(empty, h)
    assert out.real.shape == (0, 71) and out.imag.shape == (0, 71)
    (out.real.sum() + out.imag.sum()).backward()
    assert empty.real.grad.shape == (0, 64) and h.grad.shape == (8,) and not bool(h.grad.any())
