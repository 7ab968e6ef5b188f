"""cplx.upfirdn / cplx.resample_poly on the GPU (csrc/upfirdn.hip, upfirdn_wgrad.hip through cplxmodule_amd/upfirdn.py):
bit-exact on integer operands (both forms of P1, P2, forward and both gradients, every real / complex pair, the tile and
packing seams), Gaussian data against the complex128 oracle and scipy's recorded outputs, layouts (identical bits, one
launch, no copy), the single rounding of bf16, gradcheck and gradgradcheck, bit-identical reruns, hipGraph replay and
empty batches.  Cases, oracle and bounds: upfirdn_cases.py."""
import functools

import pytest
import torch

import fft_cases as fc
import upfirdn_cases as uc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import upfirdn as hostup
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
KINDS = {"cc": (True, True), "rc": (False, True), "cr": (True, False), "rr": (False, False)}


def operand(re, im, dtype, grad=False):
    """planes on the CPU -> a Cplx (im given) or a real tensor on the device"""
    re = re.to(dtype).to(DEV).requires_grad_(grad)
    return re if im is None else Cplx(re, im.to(dtype).to(DEV).requires_grad_(grad))


def planes(y):
    return (y, None) if torch.is_tensor(y) else (y.real, y.imag)


def assert_equal(got, ref, dtype, what=""):
    """`got` (Cplx, pair of planes or real tensor) EQUALS the complex128 reference rounded once to dtype"""
    gr, gi = got if isinstance(got, tuple) else planes(got)
    assert gr.dtype == dtype and gr.shape == ref.shape and gr.is_contiguous(), what
    assert float(max(ref.real.abs().max(), ref.imag.abs().max())) < 2 ** 24
    assert torch.equal(gr.double().cpu(), ref.real.to(dtype).double()), f"real plane {what}"
    if gi is None:
        assert not bool(ref.imag.any()), what
    else:
        assert torch.equal(gi.double().cpu(), ref.imag.to(dtype).double()), f"imaginary plane {what}"


def error(got, ref):
    return fc.normwise(uc.c128(planes(got)), ref)


def z(re, im):
    return torch.complex(re, torch.zeros_like(re) if im is None else im)


def rows_p2(a, c, up, down, off, k):
    """the oracle's P2 summed over the rows (one shared result)"""
    return torch.from_numpy(sum(uc.p2(a[r].numpy(), c[r].numpy(), up, down, off, k) for r in range(a.shape[0])))


# ---- 1. exact: integers in [-4, 4] ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.exact_cases() + uc.PACKED, ids=lambda c: "x".join(map(str, c)))
def test_exact_forward_and_primitives(case):
    rows, n, k, up, down = case
    xr, xi, hr, hi = uc.exact_case(rows, n, k)
    length = uc.length_upfirdn(n, k, up, down)
    for kind, (xc, hc) in KINDS.items():
        x64, h64 = z(xr, xi if xc else None), z(hr, hi if hc else None)
        ref = uc.rows_p1(x64, h64, up, down, 0, length)
        corr = uc.rows_p1(x64, h64, up, down, 1, length, True)           # the correlation form, an odd offset
        c64 = z(uc.integers((rows, length), 50), uc.integers((rows, length), 51) if hc else None)
        taps = rows_p2(x64, c64, up, down, 0, k)
        for dtype in DTYPES:
            x, h = operand(xr, xi if xc else None, dtype), operand(hr, hi if hc else None, dtype)
            y = cplx.upfirdn(h, x, up, down)
            assert torch.is_tensor(y) == (kind == "rr")
            assert_equal(y, ref, dtype, f"{kind} conv")
            xp, hp = planes(x), planes(h)
            assert_equal(hostup.conv(*xp, hp[0][None], None if hp[1] is None else hp[1][None], up, down, 1, length, True,
                                     xc or hc), corr, dtype, f"{kind} corr")
            c = operand(c64.real, c64.imag if hc else None, dtype)
            assert_equal(hostup.wgrad(*xp, *planes(c), up, down, 0, k, (1,), xc or hc), taps[None], dtype, f"{kind} P2")


@pytest.mark.parametrize("case", uc.exact_cases() + uc.PACKED, ids=lambda c: "x".join(map(str, c)))
def test_exact_first_order_gradients(case):
    """loss = sum w_r Re y + w_i Im y with integer weights g = w_r + i w_i: dx = P1 corr(g, h; down, up, 0) and
    dh = P2(x, g; up, down, 0) are integer sums; they EQUAL the oracle's (bf16: rounded once).  The gradient of a real
    operand is the real part."""
    rows, n, k, up, down = case
    xr, xi, hr, hi = uc.exact_case(rows, n, k)
    length = uc.length_upfirdn(n, k, up, down)
    wr, wi = uc.integers((rows, length), 90), uc.integers((rows, length), 91)
    for kind, (xc, hc) in KINDS.items():
        x64, h64 = z(xr, xi if xc else None), z(hr, hi if hc else None)
        g64 = z(wr, wi if (xc or hc) else None)
        dx = uc.rows_p1(g64, h64, down, up, 0, n, True)
        dh = rows_p2(x64, g64, up, down, 0, k)
        for dtype in (torch.float32, torch.bfloat16):
            x, h = operand(xr, xi if xc else None, dtype, True), operand(hr, hi if hc else None, dtype, True)
            yr, yi = planes(cplx.upfirdn(h, x, up, down))
            loss = (yr * wr.to(dtype).to(DEV)).sum() + (0 if yi is None else (yi * wi.to(dtype).to(DEV)).sum())
            leaves = [t for t in planes(x) + planes(h) if t is not None]
            got = iter(torch.autograd.grad(loss, leaves))
            for name, ref, cplx_op in (("dx", dx, xc), ("dh", dh, hc)):
                gr = next(got)
                gi = next(got) if cplx_op else None
                ref = ref if cplx_op else torch.complex(ref.real, torch.zeros_like(ref.real))
                assert_equal((gr, gi), ref, dtype, f"{kind} {name}")


def test_exact_with_64_bit_phase_arithmetic():
    """up = 2^20, down = 2^21 + 2^18: a tile of 1024 outputs spans 1024 down > 2^31, so the phase of an output is taken with
    the kernel's 64-bit division (every other case fits 32 bits), and n down exceeds 2^31 from output 911 on.  Every
    fourth output meets tap 0 (n down mod up = (n mod 4) 2^18), the others meet none and must be exact zeros."""
    up, down, n, k = 1 << 20, (1 << 21) + (1 << 18), 3000, 5
    xr, xi, hr, hi = uc.exact_case(2, n, k)
    length = uc.length_upfirdn(n, k, up, down)
    p = hostup.plan(n, k, length, up, down)
    assert p["T"] == 1024 and p["tiles"] == 2 and p["T"] * down + up >= 2 ** 31 and (length - 1) * down >= 2 ** 31
    ref = uc.rows_p1(z(xr, xi), z(hr, hi), up, down, 0, length)
    assert int((ref != 0).sum()) > length // 8
    for dtype in (torch.float32, torch.bfloat16):
        assert_equal(cplx.upfirdn(operand(hr, hi, dtype), operand(xr, xi, dtype), up, down), ref, dtype)
    corr = uc.rows_p1(z(xr, xi), z(hr, hi), up, down, -3, length, True)      # every fourth output meets tap 3
    assert int((corr != 0).sum()) > length // 8
    x, h = operand(xr, xi, torch.float32), operand(hr, hi, torch.float32)
    assert_equal(hostup.conv(x.real, x.imag, h.real[None], h.imag[None], up, down, -3, length, True, True), corr, torch.float32)


def test_exact_beyond_2_to_31_samples():
    """a real bf16 row of 2^31 + 4096 samples decimated by 2^21 with three taps: the sample index and n down pass 2^31"""
    n, down = (1 << 31) + 4096, 1 << 21
    x = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    length = uc.length_upfirdn(n, 3, 1, down)
    at = (torch.arange(length, dtype=torch.int64)[:, None] * down - torch.arange(3)[None]).reshape(-1)
    at = at[(at >= 0) & (at < n)]
    x[at.to(DEV)] = uc.integers((len(at),), 17).to(torch.bfloat16).to(DEV)
    h = uc.integers((3,), 18)
    y = cplx.upfirdn(h.to(torch.bfloat16).to(DEV), x, 1, down)
    assert y.shape == (length,) and length == 1025
    idx = torch.arange(length, dtype=torch.int64)[:, None] * down - torch.arange(3)[None]
    ok = (idx >= 0) & (idx < n)
    vals = torch.where(ok, x[idx.clamp(0, n - 1).to(DEV)].double().cpu(), torch.zeros(()).double())
    ref = (vals * h[None]).sum(-1)
    assert bool(ref[-1] != 0) or bool(ref[-2] != 0)
    assert torch.equal(y.double().cpu(), ref.to(torch.bfloat16).double())


# ---- 2. Gaussian data against the oracle ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_case(n, k, up, down, dtype, rows=2):
    """(xr, xi, hr, hi) Gaussian planes on the CPU rounded to dtype, x [rows, N], h [K]; and the oracle's upfirdn"""
    xr, xi = uc.gaussian((rows, n), dtype, 3 * n + k), uc.gaussian((rows, n), dtype, 3 * n + k + 1)
    hr, hi = uc.gaussian((k,), dtype, 5 * n + k), uc.gaussian((k,), dtype, 5 * n + k + 1)
    ref = uc.rows_p1(uc.c128((xr, xi)), uc.c128((hr, hi)), up, down, 0, uc.length_upfirdn(n, k, up, down))
    return xr, xi, hr, hi, ref


TOLERANCED = [(300, 33, 3, 2), (2000, 161, 1, 8), (700, 81, 4, 1), (500, 3201, 160, 147), (150, 4096, 1, 1), (150, 4096, 3, 2),
              (150, 4097, 3, 2), (4100, 1281, 1, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", TOLERANCED, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_against_the_oracle(case, dtype):
    n, k, up, down = case
    xr, xi, hr, hi, ref = gauss_case(n, k, up, down, dtype)
    y = cplx.upfirdn(operand(hr, hi, dtype), operand(xr, xi, dtype), up, down)
    err = error(y, ref)
    path = hostup.plan(n, k, ref.shape[-1], up, down, dtype=dtype)
    print(f"upfirdn_parity forward N={n} K={k} {up}/{down} {dtype} path={path['path']} segs={path['segs']}: {err:.3g}")
    assert y.real.dtype == dtype and y.real.shape == ref.shape and err <= fc.tol(dtype)


@pytest.mark.parametrize("case", [(300, 33, 3, 2), (2000, 161, 1, 8), (500, 3201, 160, 147)], ids=lambda c: "x".join(map(str, c)))
def test_bf16_rounds_once(case):
    n, k, up, down = case
    xr, xi, hr, hi, ref = gauss_case(n, k, up, down, torch.bfloat16)
    y = cplx.upfirdn(operand(hr, hi, torch.bfloat16), operand(xr, xi, torch.bfloat16), up, down)
    assert y.real.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(y, ref)
    print(f"upfirdn_parity bf16 N={n} K={k} {up}/{down}: {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} of the bound")
    assert bad == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_resample_poly_against_golden_scipy(dtype):
    g = uc.golden()
    for i, (n, up, down) in enumerate(uc.GOLDEN_RESAMPLE):
        x = uc.golden_input(n, 3000 + i)
        xr, xi = torch.from_numpy(x.real.copy()).to(dtype), torch.from_numpy(x.imag.copy()).to(dtype)
        # scipy's result for the values the kernel was given: the golden one in float64, within float32's input rounding
        ref = torch.from_numpy(g[f"resample_{n}_{up}_{down}"])
        y = cplx.resample_poly(Cplx(xr.to(DEV), xi.to(DEV)), up, down)
        assert y.real.shape == ref.shape and y.real.dtype == dtype
        assert error(y, ref) <= fc.tol(dtype), (n, up, down)
        yr = cplx.resample_poly(xr.to(DEV), up, down)
        assert torch.is_tensor(yr) and error(yr, torch.from_numpy(g[f"resample_real_{n}_{up}_{down}"]) + 0j) <= fc.tol(dtype)
    for i, (n, up, down, k) in enumerate(uc.GOLDEN_WINDOW):
        x, w = uc.golden_input(n, 4000 + i), uc.golden_input(k, 5000 + i, cplx=False)
        xc = Cplx(torch.from_numpy(x.real.copy()).to(dtype).to(DEV), torch.from_numpy(x.imag.copy()).to(dtype).to(DEV))
        y = cplx.resample_poly(xc, up, down, torch.from_numpy(w).to(dtype).to(DEV))
        assert error(y, torch.from_numpy(g[f"window_{n}_{up}_{down}_{k}"])) <= fc.tol(dtype), (n, up, down, k)
    i, (n, k, up, down) = 3, uc.GOLDEN_UPFIRDN[3]
    x, h = uc.golden_input(n, 1000 + i), uc.golden_input(k, 2000 + i)
    y = cplx.upfirdn(operand(torch.from_numpy(h.real.copy()), torch.from_numpy(h.imag.copy()), dtype),
                     operand(torch.from_numpy(x.real.copy()), torch.from_numpy(x.imag.copy()), dtype), up, down)
    assert error(y, torch.from_numpy(g[f"upfirdn_{n}_{k}_{up}_{down}"])) <= fc.tol(dtype)
    # equal rates after the gcd: a copy of the input
    same = cplx.resample_poly(xc, 4, 4)
    assert torch.equal(same.real, xc.real) and same.real.data_ptr() != xc.real.data_ptr()


# ---- 3. broadcast and layout -----------------------------------------------------------------------------------------
def test_layouts_give_identical_bits_in_one_launch(monkeypatch):
    n, k, up, down = 700, 21, 3, 2
    xr, xi = (uc.gaussian((4, 3, n), torch.float32, s).to(DEV) for s in (21, 22))
    hr, hi = (uc.gaussian((3, k), torch.float32, s).to(DEV) for s in (23, 24))
    calls = []

    def recording(name, *args):
        calls.append((name,) + tuple(None if a is None else a.value for a in args[:4]))
        return orig(name, *args)

    orig = hostup.call
    monkeypatch.setattr(hostup, "call", recording)

    def sliced(t):                                        # every second element of a buffer twice as long
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=DEV)
        buf[..., ::2] = t
        return buf[..., ::2]

    def transposed(t):                                    # the leading dims swapped in memory
        return t.transpose(0, 1).contiguous().transpose(0, 1)

    base = cplx.upfirdn(Cplx(hr, hi), Cplx(xr, xi), up, down)          # a filter per channel
    ref = torch.stack([uc.rows_p1(uc.c128((xr[b], xi[b])), uc.c128((hr, hi)), up, down, 0, base.real.shape[-1]) for b in range(4)])
    assert error(base, ref) <= fc.F32_TOL
    for name, fx, fh in (("sliced", sliced, sliced), ("transposed", transposed, lambda t: t),
                         ("expanded filter", lambda t: t, lambda t: t[None].expand(4, 3, k))):
        x, h = Cplx(fx(xr), fx(xi)), Cplx(fh(hr), fh(hi))
        assert x.real.stride() != xr.stride() or h.real.stride() != hr.stride()
        del calls[:]
        y = cplx.upfirdn(h, x, up, down)
        # one P1 launch that reads the planes at their own addresses: no layout copy
        assert calls == [("cplxamd_upfirdn", x.real.data_ptr(), x.imag.data_ptr(), h.real.data_ptr(), h.imag.data_ptr())], name
        assert torch.equal(y.real, base.real) and torch.equal(y.imag, base.imag), name
    # a shared filter: the bits of the per-channel launch with that filter repeated
    shared = cplx.upfirdn(Cplx(hr[0], hi[0]), Cplx(xr, xi), up, down)
    rep = cplx.upfirdn(Cplx(hr[:1].repeat(3, 1), hi[:1].repeat(3, 1)), Cplx(xr, xi), up, down)
    assert torch.equal(shared.real, rep.real) and torch.equal(shared.imag, rep.imag)
    # an expanded SIGNAL shares its one row; the bits are those of its contiguous copy
    x1 = Cplx(xr[0, :1].expand(3, n), xi[0, :1].expand(3, n))
    del calls[:]
    y = cplx.upfirdn(Cplx(hr, hi), x1, up, down)
    assert [c[:3] for c in calls] == [("cplxamd_upfirdn", x1.real.data_ptr(), x1.imag.data_ptr())]
    yc = cplx.upfirdn(Cplx(hr, hi), Cplx(x1.real.contiguous(), x1.imag.contiguous()), up, down)
    assert torch.equal(y.real, yc.real) and torch.equal(y.imag, yc.imag)
    # four batch runs force the copy; the bits are those of the contiguous operand
    big = uc.gaussian((4, 4, 4, 4, 64), torch.float32, 25).to(DEV)
    v = big[::2, ::2, ::2, ::2]
    del calls[:]
    y = cplx.upfirdn(hr[0], v, up, down)
    assert len(calls) == 1 and calls[0][1] != v.data_ptr()
    assert torch.equal(y, cplx.upfirdn(hr[0], v.contiguous(), up, down))
    with pytest.raises(RuntimeError):
        cplx.upfirdn(Cplx(hr[:2], hi[:2]), Cplx(xr, xi), up, down)


# ---- 4. derivatives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_gradcheck_and_gradgradcheck(kind):
    xc, hc = KINDS[kind]
    up, down = 3, 2
    leaves = [uc.gaussian((2, 3, 11), torch.float64, 41).to(DEV).requires_grad_()]
    if xc:
        leaves.append(uc.gaussian((2, 3, 11), torch.float64, 42).to(DEV).requires_grad_())
    leaves.append(uc.gaussian((3, 5), torch.float64, 43).to(DEV).requires_grad_())
    if hc:
        leaves.append(uc.gaussian((3, 5), torch.float64, 44).to(DEV).requires_grad_())

    def build(args):
        it = iter(args)
        xr = next(it)
        x = Cplx(xr, next(it)) if xc else xr
        hr = next(it)
        return x, (Cplx(hr, next(it)) if hc else hr)

    def fn_upfirdn(*args):
        x, h = build(args)
        return tuple(p for p in planes(cplx.upfirdn(h, x, up, down)) if p is not None)

    def fn_resample(*args):                               # the filter as a tensor window: its gradient goes through P2
        x, h = build(args)
        w = h[0] if torch.is_tensor(h) else h.real[0] + h.imag[0]
        return tuple(p for p in planes(cplx.resample_poly(x, up, down, w)) if p is not None)

    assert torch.autograd.gradcheck(fn_upfirdn, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(fn_upfirdn, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(fn_resample, leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("case", [(300, 33, 3, 2), (2000, 161, 1, 8), (500, 3201, 160, 147), (150, 4097, 3, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_float32_gradients_against_float64(case):
    n, k, up, down = case
    xr, xi, hr, hi, _ = gauss_case(n, k, up, down, torch.float32)

    def grads(dtype):
        leaves = [t.to(dtype).to(DEV).requires_grad_() for t in (xr, xi, hr, hi)]
        y = cplx.upfirdn(Cplx(leaves[2], leaves[3]), Cplx(leaves[0], leaves[1]), up, down)
        w = uc.gaussian(y.real.shape, torch.float64, 61).to(dtype).to(DEV)
        return torch.autograd.grad(((y.real ** 2 + y.imag ** 2) * w).sum(), leaves)

    for got, ref in zip(grads(torch.float32), grads(torch.float64)):
        assert got.dtype == torch.float32
        err = float(torch.linalg.norm(got.double() - ref) / torch.linalg.norm(ref))
        assert err <= fc.F32_TOL, err


# ---- 5. reruns, hipGraph, empty batches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(300, 33, 3, 2), (3000, 3201, 160, 147)], ids=lambda c: "x".join(map(str, c)))
def test_reruns_are_bit_identical(case):
    n, k, up, down = case
    xr, xi, hr, hi = (uc.gaussian(s, torch.float32, 70 + i) for i, s in enumerate(((8, n), (8, n), (k,), (k,))))

    def run():
        leaves = [t.to(DEV).requires_grad_() for t in (xr, xi, hr, hi)]
        y = cplx.upfirdn(Cplx(leaves[2], leaves[3]), Cplx(leaves[0], leaves[1]), up, down)
        return (y.real, y.imag) + torch.autograd.grad((y.real ** 2).sum() + (y.imag ** 2).sum(), leaves)

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_graph_replay_equals_eager():
    def step(xr, xi, h):
        y = cplx.resample_poly(Cplx(xr, xi), 3, 2, h)
        loss = (y.real.float() ** 2).sum() + (y.imag.float() ** 2).sum()
        return (y.real, y.imag) + torch.autograd.grad(loss, (xr, xi, h))

    shape, k = (4, 3, 1500), 33
    inputs = [uc.gaussian(shape, torch.bfloat16, 81).to(DEV).requires_grad_(), uc.gaussian(shape, torch.bfloat16, 82).to(DEV).requires_grad_(),
              uc.gaussian((k,), torch.bfloat16, 83).to(DEV).requires_grad_()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*inputs)                                     # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*inputs)
    for seed in (84, 87):
        fresh = [uc.gaussian(t.shape, torch.bfloat16, seed + i).to(DEV) for i, t in enumerate(inputs)]
        with torch.no_grad():
            for t, f in zip(inputs, fresh):
                t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*[f.requires_grad_() for f in fresh])
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


def test_device_errors_and_empty_batches(monkeypatch):
    x = torch.zeros(4, 64, device=DEV)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.upfirdn(torch.zeros(8, device=DEV, dtype=torch.bfloat16), x)
    with pytest.raises(CplxAmdError):
        cplx.upfirdn(torch.zeros(8, device=DEV, dtype=torch.float16), x.half())
    with pytest.raises(CplxAmdError):
        cplx.upfirdn(torch.zeros(8), x)
    calls = []
    orig = hostup.call
    monkeypatch.setattr(hostup, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    empty = Cplx(torch.zeros(0, 64, device=DEV, requires_grad=True), torch.zeros(0, 64, device=DEV, requires_grad=True))
    h = torch.zeros(8, device=DEV, requires_grad=True)
    out = cplx.upfirdn(h, empty, 3, 2)
    assert out.real.shape == (0, 99) and out.imag.shape == (0, 99)
    (out.real.sum() + out.imag.sum()).backward()
    assert empty.real.grad.shape == (0, 64) and h.grad.shape == (8,) and not bool(h.grad.any())
    assert cplx.resample_poly(empty, 3, 2).real.shape == (0, 96)
    assert calls == []                                    # nothing was launched
