"""cplx.lfilter / cplx.sosfilt on the GPU (csrc/iir.hip through cplxmodule_amd/iir.py): bit-exact on integer operands
(every real / complex pair, zi and zf, the chunk, tile and segment seams, the reverse | conj primitive, the forced split
path, first-order gradients), Gaussian data against the complex128 oracle and scipy's recorded outputs, layouts
(identical bits, one launch, no copy), the composed routes, gradcheck and gradgradcheck, bit-identical reruns, hipGraph
replay, empty inputs and errors.  Cases, oracle and bounds: iir_cases.py."""
import functools

import numpy as np
import pytest
import torch

import fft_cases as fc
import iir_cases as ic
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import iir as hostiir
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
KINDS = {"cc": (True, True), "rc": (False, True), "cr": (True, False), "rr": (False, False)}
GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)


def dev(z, dtype, real=False, grad=False):
    """a numpy complex array -> a Cplx (or, `real`, the real plane as a tensor) on the device, rounded to dtype"""
    z = np.asarray(z, dtype=np.complex128)
    re = torch.from_numpy(z.real.copy()).to(dtype).to(DEV).requires_grad_(grad)
    return re if real else Cplx(re, torch.from_numpy(z.imag.copy()).to(dtype).to(DEV).requires_grad_(grad))


def rounded(z, dtype):
    """the values the kernel is given: complex128 of the planes rounded to dtype"""
    z = np.asarray(z, dtype=np.complex128)
    q = lambda p: torch.from_numpy(p.copy()).to(dtype).double().numpy()        # noqa: E731
    return q(z.real) + 1j * q(z.imag)


def planes(y):
    return (y, None) if torch.is_tensor(y) else (y.real, y.imag)


def c128(y):
    yr, yi = planes(y)
    return torch.complex(yr.detach().double().cpu(), torch.zeros_like(yr).double().cpu() if yi is None else yi.detach().double().cpu())


def assert_equal(got, ref, dtype, what=""):
    """`got` (Cplx or real tensor) EQUALS the complex128 numpy reference rounded once to dtype"""
    gr, gi = planes(got)
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert gr.dtype == dtype and gr.shape == ref.shape, (what, gr.shape, ref.shape)
    assert float(max(ref.real.abs().max(), ref.imag.abs().max())) < 2 ** 24, what
    assert torch.equal(gr.double().cpu(), ref.real.to(dtype).double()), f"real plane {what}"
    if gi is None:
        assert not bool(ref.imag.any()), what
    else:
        assert torch.equal(gi.double().cpu(), ref.imag.to(dtype).double()), f"imaginary plane {what}"


def error(got, ref):
    return fc.normwise(c128(got), torch.from_numpy(np.ascontiguousarray(ref)))


# ---- 1. exact: integers in [-4, 4] ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ic.INT_FILTERS))
def test_exact_lfilter_at_the_seams(name):
    b, a, nmax = ic.INT_FILTERS[name]
    d = max(len(a), len(b)) - 1
    p = hostiir.plan(4097, d)
    assert (p["chunk"], p["tile"]) == (64, 4096) and hostiir.plan(4097, d, dtype=torch.float64)["tile"] == 2048
    for n in ic.seam_lengths(d, nmax):
        x, zi = ic.exact_case(name, n)
        ref, _ = ic.lfilter(b, a, x)
        refz, zf = ic.lfilter(b, a, x, zi)
        for dtype in DTYPES:
            y = cplx.lfilter(dev(b, dtype), dev(a, dtype), dev(x, dtype))
            assert_equal(y, ref, dtype, f"{name} N={n}")
            yz, f = cplx.lfilter(dev(b, dtype), dev(a, dtype), dev(x, dtype), dev(zi, dtype))
            assert_equal(yz, refz, dtype, f"{name} N={n} zi")
            assert_equal(f, zf, dtype, f"{name} N={n} zf")


@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_operand_pairs(kind):
    """every real / complex pair of signal and filter (a real operand is its real plane); all-real gives a real tensor"""
    xc, hc = KINDS[kind]
    for name in ("rot", "six", "eight"):
        b, a, _ = ic.INT_FILTERS[name]
        b, a = (np.asarray(b, dtype=np.complex128), np.asarray(a, dtype=np.complex128))
        if not hc:
            b, a = b.real + 0j, a.real + 0j
        if name == "rot" and not hc:
            a = np.array([1, -1], dtype=np.complex128)    # (the real part of 1 / (1 - i z^-1) is a pure gain)
        d = max(len(a), len(b)) - 1
        for n in (17, 4097):
            x, zi = ic.int_data((3, n), n, real=not xc), ic.int_data((3, d), n + 1, real=not (xc or hc))
            refz, zf = ic.lfilter(b, a, x, zi)
            for dtype in DTYPES:
                args = (dev(b, dtype, not hc), dev(a, dtype, not hc), dev(x, dtype, not xc))
                y = cplx.lfilter(*args)
                assert torch.is_tensor(y) == (kind == "rr")
                assert_equal(y, ic.lfilter(b, a, x)[0], dtype, f"{kind} {name} N={n}")
                yz, f = cplx.lfilter(*args, dev(zi, dtype, not (xc or hc)))
                assert_equal(yz, refz, dtype, f"{kind} {name} N={n} zi")
                assert_equal(f, zf, dtype, f"{kind} {name} N={n} zf")


@pytest.mark.parametrize("rows", [1, 3, 300])
def test_exact_rows_and_cascades(rows):
    n = 4100
    x = ic.int_data((rows, n), rows)
    for name in ic.INT_CASCADES:
        sos = ic.int_sos(name)
        zi = ic.int_data((rows, len(sos), 2), rows + 5)
        ref, zf = ic.sosfilt(sos, x, zi)
        for dtype in DTYPES:
            y, f = cplx.sosfilt(dev(sos, dtype), dev(x, dtype), dev(zi, dtype))
            assert_equal(y, ref, dtype, f"{name} rows={rows}")
            assert_equal(f, zf, dtype, f"{name} rows={rows} zf")
            assert_equal(cplx.sosfilt(dev(sos, dtype), dev(x, dtype)), ic.sosfilt(sos, x)[0], dtype, name)
    b, a, _ = ic.INT_FILTERS["three"]
    assert_equal(cplx.lfilter(dev(b, torch.float32), dev(a, torch.float32), dev(x, torch.float32)), ic.lfilter(b, a, x)[0],
                 torch.float32, f"rows={rows}")


def primitive(secs, x, zi, dtype, reverse, conj, force=None):
    """hostiir.run on one shared cascade: secs [(b, a)] padded -> (y, zf) as Cplx"""
    c = np.stack([np.concatenate([b, a]) for b, a in secs])[None]
    cc, xx = dev(c, dtype), dev(x, dtype)
    zz = None if zi is None else dev(zi, dtype)
    yr, yi, fr, fi = hostiir.run(xx.real, xx.imag, cc.real, cc.imag, None if zz is None else zz.real,
                                 None if zz is None else zz.imag, reverse, conj, True, True, force)
    return Cplx(yr, yi), Cplx(fr, fi)


@pytest.mark.parametrize("name", ["rot", "six", "eight"])
def test_exact_reverse_and_conj_primitive(name):
    b, a, _ = ic.INT_FILTERS[name]
    sec = ic.pad_section(b, a)
    d = len(sec[1]) - 1
    for n in (17, 4097 + 300):
        x, zi = ic.int_data((3, n), n + 2), ic.int_data((3, d), n + 3)
        for reverse, conj in ((True, True), (True, False), (False, True)):
            ref, zf = ic.lfilter(b, a, x, zi, reverse=reverse, conj=conj)
            for dtype in DTYPES:
                y, f = primitive([sec], x, zi[:, None], dtype, reverse, conj)
                assert_equal(y, ref, dtype, f"{name} N={n} reverse={reverse} conj={conj}")
                assert_equal(f, zf[:, None], dtype, f"{name} N={n} zf")
    sos = ic.int_sos("three")
    x, zi = ic.int_data((3, 4500), 9), ic.int_data((3, 3, 2), 10)
    ref, zf = ic.sosfilt(sos[::-1], x, zi[:, ::-1], reverse=True, conj=True)   # the oracle walks the sections backwards
    y, f = primitive([(s[:3], s[3:]) for s in sos], x, zi, torch.float32, True, True)
    assert_equal(y, ref, torch.float32, "cascade reverse | conj")
    assert_equal(f, zf[:, ::-1], torch.float32, "cascade reverse | conj zf")


@pytest.mark.parametrize("segments", [2, 3, 7])
def test_forced_split_path(segments, monkeypatch):
    n = 5003
    calls = []
    orig = hostiir.call
    monkeypatch.setattr(hostiir, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    monkeypatch.setattr(hostiir, "_FORCE_SEGMENTS", segments)
    p = hostiir.plan(n, 2)
    assert p["path"] == "split" and p["segments"] == segments and n % p["seg_len"] != 0
    x = ic.int_data((3, n), segments)
    for name in ("cumsum", "six", "eight"):
        b, a, _ = ic.INT_FILTERS[name]
        d = max(len(a), len(b)) - 1
        zi = ic.int_data((3, d), segments + 1)
        ref, zf = ic.lfilter(b, a, x, zi)
        for dtype in DTYPES:
            del calls[:]
            y, f = cplx.lfilter(dev(b, dtype), dev(a, dtype), dev(x, dtype), dev(zi, dtype))
            assert calls == ["cplxamd_iir", "cplxamd_iir", "cplxamd_iir_scan", "cplxamd_iir"]
            assert_equal(y, ref, dtype, f"{name} split {segments}")
            assert_equal(f, zf, dtype, f"{name} split {segments} zf")
    sos = ic.int_sos("three")
    zi = ic.int_data((3, 3, 2), 11)
    ref, zf = ic.sosfilt(sos, x, zi)
    y, f = cplx.sosfilt(dev(sos, torch.float32), dev(x, torch.float32), dev(zi, torch.float32))
    assert_equal(y, ref, torch.float32, "cascade split")
    assert_equal(f, zf, torch.float32, "cascade split zf")
    # per-row filters (the transition matrix per filter) and Gaussian data: within the tolerance of the oracle
    g = ic.golden()
    for dtype in (torch.float32, torch.float64):
        bb = np.stack([g["butter2_b"], np.pad(g["dcblock_b"] * 0.5, (0, 1)), g["butter2_b"] * 2])
        aa = np.stack([g["butter2_a"], np.pad(g["dcblock_a"], (0, 1)), g["butter2_a"]])
        xg = rounded(ic.gauss_data((3, n), 12), dtype)
        ref, _ = ic.lfilter(rounded(bb, dtype), rounded(aa, dtype), xg)
        y = cplx.lfilter(dev(bb, dtype), dev(aa, dtype), dev(xg, dtype))
        assert error(y, ref) <= fc.tol(dtype)
        sos = rounded(g["butter8sos_sos"], dtype)
        ref, _ = ic.sosfilt(sos, xg)
        assert error(cplx.sosfilt(dev(sos, dtype), dev(xg, dtype)), ref) <= fc.tol(dtype)


def oracle_gradients(b, a, x, zi, g):
    """dx, db, da (k >= 1), dzi of loss = Re sum conj(g) y, by the identities of iir.py, rows sharing the filter"""
    d = max(len(a), len(b)) - 1
    bp, ap = ic.pad_section(b, a)
    y, _ = ic.lfilter(b, a, x, zi)
    dx, _ = ic.lfilter(b, a, g, reverse=True, conj=True)
    gt, _ = ic.lfilter([1], a, g, reverse=True, conj=True)
    n = x.shape[-1]
    db = np.array([np.sum(np.conj(x[:, :n - k]) * gt[:, k:]) for k in range(d + 1)])
    da = np.array([-np.sum(np.conj(y[:, :n - k]) * gt[:, k:]) for k in range(d + 1)])
    dz = np.pad(gt[:, :d], ((0, 0), (0, max(d - n, 0))))
    return dx, db[:len(b)], da[:len(a)], dz


@pytest.mark.parametrize("name", ["rot", "cos", "six", "three"])
def test_exact_first_order_gradients(name):
    b, a, _ = ic.INT_FILTERS[name]
    d = max(len(a), len(b)) - 1
    for n in (2, 50, 300):
        x, zi, g = ic.int_data((3, n), n + 20), ic.int_data((3, d), n + 21), ic.int_data((3, n), n + 22)
        dx, db, da, dz = oracle_gradients(np.asarray(b, dtype=complex), np.asarray(a, dtype=complex), x, zi, g)
        for dtype in (torch.float32, torch.float64):
            tb, ta, tx, tz = (dev(v, dtype, grad=True) for v in (b, a, x, zi))
            y, _ = cplx.lfilter(tb, ta, tx, tz)
            w = dev(g, dtype)
            loss = (y.real * w.real).sum() + (y.imag * w.imag).sum()
            leaves = [tx.real, tx.imag, tb.real, tb.imag, ta.real, ta.imag, tz.real, tz.imag]
            got = torch.autograd.grad(loss, leaves)
            assert_equal(Cplx(got[0], got[1]), dx, dtype, f"{name} N={n} dx")
            assert_equal(Cplx(got[2], got[3]), db, dtype, f"{name} N={n} db")
            assert_equal(Cplx(got[4][1:], got[5][1:]), da[1:], dtype, f"{name} N={n} da")
            assert_equal(Cplx(got[6], got[7]), dz, dtype, f"{name} N={n} dzi")


# ---- 2. Gaussian data -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_case(name, dtype, n=5000):
    g = ic.golden()
    b, a = rounded(g[f"{name}_b"], dtype), rounded(g[f"{name}_a"], dtype)
    x, zi = rounded(ic.gauss_data((2, n), 31), dtype), rounded(ic.gauss_data((2, max(len(a), len(b)) - 1), 32), dtype)
    return b, a, x, zi, ic.lfilter(b, a, x)[0], ic.lfilter(b, a, x, zi)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ic.GAUSS_BA)
def test_gaussian_lfilter_against_the_oracle(name, dtype):
    b, a, x, zi, ref, (refz, zf) = gauss_case(name, dtype)
    y = cplx.lfilter(dev(b, dtype), dev(a, dtype), dev(x, dtype))
    yz, f = cplx.lfilter(dev(b, dtype), dev(a, dtype), dev(x, dtype), dev(zi, dtype))
    errs = error(y, ref), error(yz, refz), error(f, zf)
    print(f"iir_parity lfilter {name} {dtype}: y {errs[0]:.3g}, with zi {errs[1]:.3g}, zf {errs[2]:.3g}")
    assert max(errs) <= fc.tol(dtype)


@pytest.mark.parametrize("name", ["butter2", "dcblock", "cpole"])
def test_bf16_rounds_once(name):
    b, a, x, zi, ref, (refz, zf) = gauss_case(name, torch.bfloat16)
    y, f = cplx.lfilter(dev(b, torch.bfloat16), dev(a, torch.bfloat16), dev(x, torch.bfloat16), dev(zi, torch.bfloat16))
    assert y.real.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(y, torch.from_numpy(refz))
    badf, worstf = fc.bf16_violations(f, torch.from_numpy(zf))
    print(f"iir_parity bf16 {name}: {bad} + {badf} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {max(worst, worstf):.3f}")
    assert bad == 0 and badf == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_against_golden_scipy(dtype):
    g = ic.golden()
    for name in ic.GAUSS_BA:
        b, a = g[f"{name}_b"], g[f"{name}_a"]
        real = not (np.iscomplexobj(b) or np.iscomplexobj(a))
        for kind in ("real", "cplx"):
            x, zi = g[f"x_{kind}"], g[f"{name}_zi"]
            allreal = kind == "real" and real
            args = (dev(b, dtype, real), dev(a, dtype, real), dev(x, dtype, kind == "real"))
            y = cplx.lfilter(*args)
            assert torch.is_tensor(y) == allreal
            assert error(y, g[f"{name}_{kind}_y"] + 0j) <= fc.tol(dtype), (name, kind)
            yz, f = cplx.lfilter(*args, dev(zi, dtype, allreal))
            assert error(yz, g[f"{name}_{kind}_yz"] + 0j) <= fc.tol(dtype), (name, kind)
            assert error(f, g[f"{name}_{kind}_zf"] + 0j) <= fc.tol(dtype), (name, kind)
    sos, zi = g["butter8sos_sos"], g["butter8sos_zi"]
    for kind in ("real", "cplx"):
        x = g[f"x_{kind}"]
        r = kind == "real"
        assert error(cplx.sosfilt(dev(sos, dtype, True), dev(x, dtype, r)), g[f"butter8sos_{kind}_y"] + 0j) <= fc.tol(dtype)
        y, f = cplx.sosfilt(dev(sos, dtype, True), dev(x, dtype, r), dev(zi, dtype, r))
        assert error(y, g[f"butter8sos_{kind}_yz"] + 0j) <= fc.tol(dtype)
        assert error(f, g[f"butter8sos_{kind}_zf"] + 0j) <= fc.tol(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_per_channel_filters_and_sosfilt(dtype):
    g = ic.golden()
    n = 4200
    x = rounded(ic.gauss_data((4, 3, n), 41), dtype)
    bb = rounded(np.stack([g["butter4_b"], g["cheby4_b"], g["ellip4_b"]]), dtype)
    aa = rounded(np.stack([g["butter4_a"], g["cheby4_a"], g["ellip4_a"]]), dtype)
    y = cplx.lfilter(dev(bb, dtype, True), dev(aa, dtype, True), dev(x, dtype))
    ref = np.stack([ic.lfilter(bb, aa, x[i])[0] for i in range(4)])
    assert error(y, ref) <= fc.tol(dtype)
    sos = rounded(np.stack([g["butter8sos_sos"], g["butter8sos_sos"][::-1] * 0.5, g["butter8sos_sos"]]), dtype)
    zi = rounded(ic.gauss_data((4, 3, 4, 2), 42), dtype)
    y, f = cplx.sosfilt(dev(sos, dtype, True), dev(x, dtype), dev(zi, dtype))
    out = [ic.sosfilt(sos, x[i], zi[i]) for i in range(4)]
    assert error(y, np.stack([o[0] for o in out])) <= fc.tol(dtype)
    assert error(f, np.stack([o[1] for o in out])) <= fc.tol(dtype)


# ---- 3. layouts -----------------------------------------------------------------------------------------------------------
def test_layouts_give_identical_bits_in_one_launch(monkeypatch):
    g = ic.golden()
    n = 4200
    xr, xi = (fc.gaussian((4, 3, n), torch.float32, s)[0].to(DEV) for s in (21, 22))
    b = dev(np.stack([g["butter4_b"], g["cheby4_b"], g["ellip4_b"]]), torch.float32, True)
    a = dev(np.stack([g["butter4_a"], g["cheby4_a"], g["ellip4_a"]]), torch.float32, True)
    sos = dev(g["butter8sos_sos"], torch.float32, True)
    calls = []

    def recording(name, *args):
        calls.append((name,) + tuple(None if v is None else v.value for v in args[:2]))
        return orig(name, *args)

    orig = hostiir.call
    monkeypatch.setattr(hostiir, "call", recording)

    def sliced(t):                                        # every second element of a buffer twice as long
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=DEV)
        buf[..., ::2] = t
        return buf[..., ::2]

    def transposed(t):                                    # the leading dims swapped in memory
        return t.transpose(0, 1).contiguous().transpose(0, 1)

    base = cplx.lfilter(b, a, Cplx(xr, xi))
    base_sos = cplx.sosfilt(sos, Cplx(xr, xi))
    for name, fx in (("sliced", sliced), ("transposed", transposed)):
        x = Cplx(fx(xr), fx(xi))
        assert x.real.stride() != xr.stride()
        del calls[:]
        y = cplx.lfilter(b, a, x)
        ys = cplx.sosfilt(sos, x)
        # one launch each that reads the planes at their own addresses: no layout copy
        assert calls == [("cplxamd_iir", x.real.data_ptr(), x.imag.data_ptr())] * 2, name
        assert torch.equal(y.real, base.real) and torch.equal(y.imag, base.imag), name
        assert torch.equal(ys.real, base_sos.real) and torch.equal(ys.imag, base_sos.imag), name
    # an expanded SIGNAL shares its one row; the bits are those of its contiguous copy
    x1 = Cplx(xr[0, :1].expand(3, n), xi[0, :1].expand(3, n))
    del calls[:]
    y = cplx.lfilter(b, a, x1)
    assert calls == [("cplxamd_iir", x1.real.data_ptr(), x1.imag.data_ptr())]
    yc = cplx.lfilter(b, a, Cplx(x1.real.contiguous(), x1.imag.contiguous()))
    assert torch.equal(y.real, yc.real) and torch.equal(y.imag, yc.imag)
    # an expanded filter: the bits of the per-channel call
    y = cplx.lfilter(b[None].expand(4, 3, 5), a[None].expand(4, 3, 5), Cplx(xr, xi))
    assert torch.equal(y.real, base.real) and torch.equal(y.imag, base.imag)
    # four batch runs force the copy; the bits are those of the contiguous operand
    big = fc.gaussian((4, 4, 4, 4, 64), torch.float32, 25)[0].to(DEV)
    v = big[::2, ::2, ::2, ::2]
    del calls[:]
    y = cplx.lfilter(b[0], a[0], v)
    assert len(calls) == 1 and calls[0][1] != v.data_ptr()
    assert torch.equal(y, cplx.lfilter(b[0], a[0], v.contiguous()))
    with pytest.raises(RuntimeError):
        cplx.lfilter(b[:2], a[:2], Cplx(xr, xi))


# ---- 4. the composed routes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_composed_routes_against_the_oracle(dtype):
    g = ic.golden()
    n = 3000
    x = rounded(ic.gauss_data((2, n), 51), dtype)
    # nb = 40 with zi: one polyphase launch, zi as an added sequence, the all-pole kernel
    b, a = rounded(ic.gauss_data((40,), 52), dtype), rounded(g["butter4_a"], dtype)
    zi = rounded(ic.gauss_data((2, 39), 53), dtype)
    ref, zf = ic.lfilter(b, a, x, zi)
    y, f = cplx.lfilter(dev(b, dtype), dev(a, dtype, True), dev(x, dtype), dev(zi, dtype))
    assert error(y, ref) <= fc.tol(dtype) and error(f, zf) <= fc.tol(dtype)
    short, fs = cplx.lfilter(dev(b, dtype), dev(a, dtype, True), dev(x[:, :7], dtype), dev(zi, dtype))     # N < D
    rs, rf = ic.lfilter(b, a, x[:, :7], zi)
    assert error(short, rs) <= fc.tol(dtype) and error(fs, rf) <= fc.tol(dtype)
    # 20 sections: two chained launches
    sos = rounded(np.tile(g["butter8sos_sos"], (5, 1)), dtype)
    zi = rounded(ic.gauss_data((2, 20, 2), 54), dtype)
    ref, zf = ic.sosfilt(sos, x, zi)
    y, f = cplx.sosfilt(dev(sos, dtype, True), dev(x, dtype), dev(zi, dtype))
    assert error(y, ref) <= fc.tol(dtype) and error(f, zf) <= fc.tol(dtype)
    assert error(cplx.sosfilt(dev(sos, dtype, True), dev(x, dtype)), ic.sosfilt(sos, x)[0]) <= fc.tol(dtype)
    # sos.requires_grad: the cascade composed from per-section filters
    sos = rounded(g["butter8sos_sos"], dtype)
    ts = dev(sos, dtype, True, grad=True)
    y, f = cplx.sosfilt(ts, dev(x, dtype), dev(zi[:, :4], dtype))
    ref, zf = ic.sosfilt(sos, x, zi[:, :4])
    assert error(y, ref) <= fc.tol(dtype) and error(f, zf) <= fc.tol(dtype)
    (y.real.sum() + f.imag.sum()).backward()
    assert ts.grad.shape == (4, 6) and bool(torch.isfinite(ts.grad).all())
    # D = 0 is a scale
    y = cplx.lfilter(dev([2 + 1j], dtype), dev([4], dtype), dev(x, dtype))
    assert error(y, x * (2 + 1j) / 4) <= fc.tol(dtype)


# ---- 5. derivatives -------------------------------------------------------------------------------------------------------
def leaf(shape, seed, scale=1.0):
    return (fc.gaussian(shape, torch.float64, seed)[0] * scale).to(DEV).requires_grad_()


@pytest.mark.parametrize("kind", ["cplx", "real"])
def test_gradcheck_and_gradgradcheck_lfilter(kind):
    """N = 40, D = 3; leaves x, b, a, zi.  The gradients of real operands are real: the leaves are real planes."""
    n, planes_ = 40, 2 if kind == "cplx" else 1
    a0 = torch.tensor([[1.5, -0.4, 0.3, 0.1], [1.2, 0.5, -0.2, 0.1]], dtype=torch.float64)
    leaves = []
    for p in range(planes_):
        leaves += [leaf((2, n), 100 + p), leaf((2, 3), 102 + p), (a0 * (1 if p == 0 else 0.2)).to(DEV).requires_grad_(),
                   leaf((2, 3), 106 + p)]

    def fn(*args):
        ops = [args[i] if planes_ == 1 else Cplx(args[i], args[4 + i]) for i in range(4)]
        y, zf = cplx.lfilter(ops[1], ops[2], ops[0], ops[3])
        return tuple(p for p in planes(y) + planes(zf) if p is not None)

    assert torch.autograd.gradcheck(fn, leaves, **GC)
    assert torch.autograd.gradgradcheck(fn, leaves, **GC)


def test_gradcheck_and_gradgradcheck_cascade():
    """a 2-section cascade: the fused route (x only) and the composed one (dsos, dzi)"""
    n = 24
    sos0 = torch.tensor([[0.5, 0.3, 0.2, 1.5, -0.4, 0.3], [1.0, -0.5, 0.1, 0.8, 0.2, 0.1]], dtype=torch.float64)
    sos_r, sos_i = sos0.to(DEV), (0.1 * sos0.flip(-1)).to(DEV)
    xr, xi = leaf((2, n), 111), leaf((2, n), 112)

    def fused(xr, xi):
        return planes(cplx.sosfilt(Cplx(sos_r, sos_i), Cplx(xr, xi)))

    assert torch.autograd.gradcheck(fused, [xr, xi], **GC)
    assert torch.autograd.gradgradcheck(fused, [xr, xi], **GC)

    def composed(xr, xi, sr, si, zr, zi):
        y, zf = cplx.sosfilt(Cplx(sr, si), Cplx(xr, xi), Cplx(zr, zi))
        return planes(y) + planes(zf)

    leaves = [xr, xi, sos_r.clone().requires_grad_(), sos_i.clone().requires_grad_(), leaf((2, 2, 2), 113), leaf((2, 2, 2), 114)]
    assert torch.autograd.gradcheck(composed, leaves, **GC)
    assert torch.autograd.gradgradcheck(composed, leaves, **GC)
    real = [xr, sos_r.clone().requires_grad_()]
    assert torch.autograd.gradcheck(lambda x, s: cplx.sosfilt(s, x), real, **GC)


# ---- 6. reruns, hipGraph, empty inputs, errors ----------------------------------------------------------------------------
def test_reruns_are_bit_identical(monkeypatch):
    g = ic.golden()
    planes_ = [fc.gaussian(s, torch.float32, 70 + i)[0] for i, s in enumerate(((8, 9000), (8, 9000), (8, 4)))]
    b, a = (torch.from_numpy(g[f"butter4_{k}"]).float() for k in "ba")

    def run():
        leaves = [t.to(DEV).requires_grad_() for t in planes_ + [b, a]]
        y, zf = cplx.lfilter(leaves[3], leaves[4], Cplx(leaves[0], leaves[1]), leaves[2])
        loss = (y.real ** 2).sum() + (y.imag ** 2).sum() + zf.real.sum()
        return (y.real, y.imag, zf.real, zf.imag) + torch.autograd.grad(loss, leaves)

    for force in (0, 3):
        monkeypatch.setattr(hostiir, "_FORCE_SEGMENTS", force)
        for p, q in zip(run(), run()):
            assert torch.equal(p, q)


def test_graph_replay_equals_eager():
    g = ic.golden()
    sos = torch.from_numpy(g["butter8sos_sos"]).float().to(DEV)
    b, a = (torch.from_numpy(g[f"butter2_{k}"]).float().to(DEV) for k in "ba")

    def step(xr, xi):
        y = cplx.sosfilt(sos, Cplx(xr, xi))
        w, zf = cplx.lfilter(b, a, y, torch.ones(2, device=DEV))
        loss = (w.real ** 2).sum() + (w.imag ** 2).sum()
        return (w.real, w.imag, zf.real) + torch.autograd.grad(loss, (xr, xi))

    shape = (4, 3, 4500)
    inputs = [fc.gaussian(shape, torch.float32, 81 + i)[0].to(DEV).requires_grad_() for i in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*inputs)                                     # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*inputs)
    for seed in (84, 87):
        fresh = [fc.gaussian(shape, torch.float32, seed + i)[0].to(DEV) for i in range(2)]
        with torch.no_grad():
            for t, f in zip(inputs, fresh):
                t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*[f.requires_grad_() for f in fresh])
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


def test_errors_and_empty_inputs(monkeypatch):
    x = torch.zeros(4, 64, device=DEV)
    b, a = torch.ones(2, device=DEV), torch.tensor([1.0, -0.5], device=DEV)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.lfilter(b.bfloat16(), a, x)
    with pytest.raises(CplxAmdError):
        cplx.lfilter(b.half(), a.half(), x.half())
    with pytest.raises(CplxAmdError):
        cplx.lfilter(b.cpu(), a.cpu(), x.cpu())
    with pytest.raises(CplxAmdError):
        cplx.lfilter(b, a, torch.zeros(4, 64, dtype=torch.complex64, device=DEV))
    with pytest.raises(CplxAmdError, match="sosfilt"):
        cplx.lfilter(b, torch.ones(10, device=DEV), x)
    with pytest.raises(CplxAmdError):
        cplx.sosfilt(torch.ones(2, 6), x)
    calls = []
    orig = hostiir.call
    monkeypatch.setattr(hostiir, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    empty = Cplx(torch.zeros(0, 64, device=DEV), torch.zeros(0, 64, device=DEV))
    out = cplx.lfilter(b, a, empty)
    assert out.real.shape == (0, 64) and out.imag.shape == (0, 64)
    y, zf = cplx.lfilter(b, a, torch.zeros(4, 0, device=DEV), torch.ones(4, 1, device=DEV))
    assert torch.is_tensor(y) and y.shape == (4, 0) and torch.equal(zf, torch.ones(4, 1, device=DEV))
    sos = torch.tensor([[1.0, 0, 0, 1, -0.5, 0]], device=DEV)
    assert cplx.sosfilt(sos, empty).real.shape == (0, 64)
    y, zf = cplx.sosfilt(sos, torch.zeros(0, 64, device=DEV), torch.zeros(1, 2, device=DEV))
    assert y.shape == (0, 64) and zf.shape == (0, 1, 2)
    assert calls == []                                    # nothing was launched
