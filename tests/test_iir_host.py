"""cplx.lfilter / cplx.sosfilt without a GPU: the plan (cplxamd_iir_plan is a pure function), the chunk / tile / segment
scheme of the kernel -- emulated in numpy from the plan's numbers alone and compared with the sequential oracle, EQUAL on
integer operands --, the oracle against the golden scipy outputs, every gradient identity by an inner-product test on
the oracle, the coverage condition of the Gaussian filters, every argument error with its exception type, the descriptor
and NULL-pointer rejections of the launchers (they return before any launch), and the headroom of the integer cases of
test_gpu_iir.py."""
import ctypes

import numpy as np
import pytest
import torch

import fft_cases as fc
import iir_cases as ic

from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import iir as hostiir
from cplxmodule_amd._lib import CplxAmdError


def words(bucket, chunk, sections, planes):
    tile = chunk * 64
    table = 2 * (bucket + 1) + bucket * chunk + bucket * bucket
    return planes * (tile + 64 + 1 + bucket * 64 + sections * bucket + sections * table)


# ---- the plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
def test_plan_table(dtype):
    chunk, word = (32, 8) if dtype == torch.float64 else (64, 4)
    for order, sections in ((1, 1), (2, 1), (3, 1), (8, 1), (1, 16), (2, 2), (2, 16)):
        for cx in (False, True):
            p = hostiir.plan(65536, order, sections, 1024, 1, dtype, cx)
            assert (p["chunk"], p["lanes"], p["tile"], p["threads"]) == (chunk, 64, 64 * chunk, 64)
            assert p["bucket"] == (8 if order > 2 else 2)
            assert p["lds_bytes"] == words(p["bucket"], chunk, sections, 2 if cx else 1) * word
            assert p["lds_bytes"] <= 76 * 1024            # two workgroups fit the 160 KiB of a CU
            assert p["path"] == "row" and (p["segments"], p["seg_len"], p["grid"], p["ws_bytes"]) == (1, 65536, 1024, 0)
            assert p["tiles"] == 65536 // p["tile"]


def test_plan_paths_and_rejections():
    # few rows of many tiles are cut into whole tiles, at least two per segment, up to 1024 one-wave workgroups
    p = hostiir.plan(1 << 22, 2, 1, 1, 1)
    assert p["path"] == "split" and (p["segments"], p["seg_len"], p["tiles"], p["grid"]) == (512, 8192, 2, 512)
    assert p["ws_bytes"] == 2 * 4 * (3 * 512 * 2 + 2 * 1 * 2 * 2)          # z, e, the final states; M and the unit states
    p = hostiir.plan(1 << 22, 2, 4, 8, 8, torch.float64, True)
    assert (p["segments"], p["seg_len"], p["grid"]) == (128, 32768, 1024)
    assert p["ws_bytes"] == 2 * 8 * (3 * 1024 * 8 + 2 * 8 * 8 * 8)
    p = hostiir.plan(65536, 2, 4, 256, 1)                                  # the benchmark's batch: a wave per CU, so cut in four
    assert p["path"] == "split" and (p["segments"], p["seg_len"], p["grid"]) == (4, 16384, 1024)
    assert hostiir.plan(1 << 22, 2, 1, 512, 1)["path"] == "split" and hostiir.plan(1 << 22, 2, 1, 513, 1)["path"] == "row"
    # eight states per section: measured slower when split at 256 rows, so only up to 128
    assert hostiir.plan(65536, 8, 1, 256, 1)["path"] == "row" and hostiir.plan(65536, 8, 1, 128, 1)["segments"] == 8
    assert hostiir.plan(1 << 22, 8, 1, 1, 1)["segments"] == 512
    assert hostiir.plan(4 * 4096 - 1, 2, 1, 1, 1)["path"] == "row" and hostiir.plan(4 * 4096, 2, 1, 1, 1)["segments"] == 2
    # the private switch: any row, segments of unequal last length
    p = hostiir.plan(5003, 8, 1, 3, 1, force_segments=7)
    assert p["path"] == "split" and (p["segments"], p["seg_len"], p["grid"]) == (7, 715, 21) and 5003 - 6 * 715 == 713
    assert hostiir.plan(3, 1, force_segments=7)["segments"] == 3
    # D = 8 / 9, cascades of biquads only, up to 16 sections a launch
    assert hostiir.plan(100, 8)["bucket"] == 8
    for order, sections in ((9, 1), (0, 1), (3, 2), (2, 17), (2, 0)):
        with pytest.raises(CplxAmdError, match="no plan"):
            hostiir.plan(100, order, sections)
    with pytest.raises(CplxAmdError, match="no plan"):
        hostiir.plan(0, 2)
    with pytest.raises(CplxAmdError, match="exceed"):
        hostiir.plan((1 << 40) + 1, 2)
    with pytest.raises(CplxAmdError):
        hostiir.plan(100, 2, dtype=torch.float16)
    out = (ctypes.c_int64 * len(_lib.IIR_PLAN_FIELDS))()
    assert _lib.load().cplxamd_iir_plan(100, 2, 1, 1, 1, _lib.F32, 1, 0, None) == -1
    assert _lib.load().cplxamd_iir_plan(100, 2, 1, 1, 1, _lib.F32, 2, 0, out) == -1
    assert _lib.load().cplxamd_iir_plan(100, 2, 1, -1, 1, _lib.F32, 1, 0, out) == -1


def test_launchers_reject_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    d = _lib.IirDesc(n=100, order=2, sections=1, segments=1, seg_len=100, x_es=1, runs=0, flags=0)
    ok = [one, one, one, one, None, None, one, one, None, None, ctypes.byref(d), 1, _lib.F32, None]

    def rc(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.cplxamd_iir(*args)

    assert rc(a2=None) == -1 and rc(a10=None) == -1       # no coefficients, no descriptor
    assert rc(a6=None, a7=None) == -1                     # neither y nor zf
    assert rc(a7=None) == -1 and rc(a8=one) == -1         # complex: y_i, zf_i missing
    assert rc(a11=0) == -1 and rc(a11=2) == -1            # real arithmetic forbids the imaginary planes
    assert rc(a0=None) == -1                              # x_i without x_r
    assert rc(a12=7) == -1
    for field, value in (("n", 0), ("order", 9), ("order", 0), ("sections", 17), ("segments", 0), ("segments", 101),
                         ("seg_len", 0), ("seg_len", 99), ("x_es", -1), ("runs", 4), ("flags", 4)):
        bad = _lib.IirDesc(n=100, order=2, sections=1, segments=1, seg_len=100, x_es=1, runs=0, flags=0)
        setattr(bad, field, value)
        assert lib.cplxamd_iir(*ok[:10], ctypes.byref(bad), 1, _lib.F32, None) == -1, field
    bad = _lib.IirDesc(n=100, order=2, sections=1, segments=3, seg_len=50, x_es=1, runs=0, flags=0)
    assert lib.cplxamd_iir(*ok[:10], ctypes.byref(bad), 1, _lib.F32, None) == -1      # an empty third segment
    bad = _lib.IirDesc(n=100, order=2, sections=1, segments=1, seg_len=100, x_es=1, runs=1, flags=0)
    bad.size[0], bad.x_stride[0] = 4, -1
    assert lib.cplxamd_iir(*ok[:10], ctypes.byref(bad), 1, _lib.F32, None) == -1
    bad.size[0], bad.x_stride[0] = 0, 0                   # no rows: nothing to do
    assert lib.cplxamd_iir(*ok[:10], ctypes.byref(bad), 1, _lib.F32, None) == 0
    scan = [one, one, one, one, None, None, one, one, 4, 1, 3, 2, 1, _lib.F32, None]

    def src(**change):
        args = list(scan)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.cplxamd_iir_scan(*args)

    assert src(a0=None) == -1 and src(a2=None) == -1 and src(a6=None) == -1 and src(a1=None) == -1 and src(a7=None) == -1
    assert src(a12=0) == -1 and src(a13=_lib.BF16) == -1 and src(a9=0) == -1 and src(a10=0) == -1
    assert src(a11=0) == -1 and src(a11=33) == -1 and src(a8=-1) == -1 and src(a5=one) == -1
    assert src(a8=0) == 0


# ---- the scheme -------------------------------------------------------------------------------------------------------
EMU_LENGTHS = (1, 63, 64, 65, 500, 4095, 4097)


@pytest.mark.parametrize("name", list(ic.INT_FILTERS))
def test_emulated_scheme_equals_the_oracle_on_integers(name):
    """float32 arithmetic (complex64), the plan's chunk, tile and segments: EQUAL, with and without zi, forward and
    reverse | conj, one segment and the forced split path"""
    b, a, nmax = ic.INT_FILTERS[name]
    sec = ic.pad_section(b, a)
    d = len(sec[1]) - 1
    for n in EMU_LENGTHS:
        if nmax and n > nmax:
            continue
        x, zi = (t[:1] for t in ic.exact_case(name, n))
        for force, reverse, conj, z in ((0, False, False, zi), (0, True, True, None), (3, False, False, zi), (2, True, True, zi)):
            p = hostiir.plan(n, d, 1, 1, 1, torch.float32, True, force)
            ref, zf = ic.lfilter(b, a, x, z, reverse=reverse, conj=conj)
            y, f = ic.emulate(x[0], [sec], z, p, reverse, conj)
            assert y.dtype == np.complex64 and np.array_equal(y.astype(np.complex128), ref[0]), (n, force, reverse)
            assert np.array_equal(f[0].astype(np.complex128), zf[0]), (n, force, reverse)


@pytest.mark.parametrize("name", list(ic.INT_CASCADES))
def test_emulated_cascades_equal_the_oracle_on_integers(name):
    sos = ic.int_sos(name)
    secs = [(s[:3], s[3:]) for s in sos]
    for n in (17, 1000, 4099):
        x, zi = ic.int_data((1, n), n + 3), ic.int_data((1, len(sos), 2), n + 4)
        for force in (0, 3):
            p = hostiir.plan(n, 2, len(sos), 1, 1, torch.float32, True, force)
            ref, zf = ic.sosfilt(sos, x, zi)
            y, f = ic.emulate(x[0], secs, zi[0], p)
            assert np.array_equal(y.astype(np.complex128), ref[0]) and np.array_equal(f.astype(np.complex128), zf[0]), (n, force)
        # float64's chunk of 32 and tile of 2048
        p = hostiir.plan(n, 2, len(sos), 1, 1, torch.float64, True, 2)
        y, f = ic.emulate(x[0], secs, zi[0], p, True, True, np.complex128)
        ref, zf = ic.sosfilt(sos[::-1], x, zi[:, ::-1], reverse=True, conj=True)
        assert np.array_equal(y, ref[0]) and np.array_equal(f, zf[0, ::-1])


def test_integer_cases_have_headroom():
    """every value of the GPU tests' integer cases stays below 2^24, and so does the sum of the D products of a state
    with an entry of the chunk tables (which reach chunk + 1 for the double integrator): float32 holds every
    intermediate of the chunked scheme exactly, so EQUAL is the right comparison"""
    for name, (b, a, nmax) in ic.INT_FILTERS.items():
        d = max(len(a), len(b)) - 1
        gain = ic.table_gain(ic.pad_section(b, a)[1])
        for n in ic.seam_lengths(d, nmax)[-3:]:
            y, zf = ic.lfilter(b, a, *ic.exact_case(name, n))
            top = max(np.abs(y.real).max(), np.abs(y.imag).max(), ic.lfilter.peak)
            assert d * max(gain, 1) * top < 2 ** 24, (name, n, gain, top)
    for name in ic.INT_CASCADES:
        for rows in (1, 3, 300):
            y, zf = ic.sosfilt(ic.int_sos(name), ic.int_data((rows, 4100), rows), ic.int_data((rows, len(ic.int_sos(name)), 2), rows + 5))
            assert 2 * 3 * max(np.abs(y.real).max(), np.abs(y.imag).max(), np.abs(zf.real).max(), np.abs(zf.imag).max()) < 2 ** 24


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def test_oracle_against_golden_scipy():
    g = ic.golden()
    for name in ic.GAUSS_BA:
        b, a = g[f"{name}_b"], g[f"{name}_a"]
        real = not (np.iscomplexobj(b) or np.iscomplexobj(a))
        for kind in ("real", "cplx"):
            x = g[f"x_{kind}"]
            zi = g[f"{name}_zi"].real if kind == "real" and real else g[f"{name}_zi"]
            assert np.allclose(ic.lfilter(b, a, x)[0], g[f"{name}_{kind}_y"], rtol=0, atol=1e-12)
            y, zf = ic.lfilter(b, a, x, zi)
            assert np.allclose(y, g[f"{name}_{kind}_yz"], rtol=0, atol=1e-12) and np.allclose(zf, g[f"{name}_{kind}_zf"], rtol=0, atol=1e-12)
    sos = g["butter8sos_sos"]
    for kind in ("real", "cplx"):
        x = g[f"x_{kind}"]
        zi = g["butter8sos_zi"].real if kind == "real" else g["butter8sos_zi"]
        assert np.allclose(ic.sosfilt(sos, x)[0], g[f"butter8sos_{kind}_y"], rtol=0, atol=1e-12)
        y, zf = ic.sosfilt(sos, x, zi)
        assert np.allclose(y, g[f"butter8sos_{kind}_yz"], rtol=0, atol=1e-12)
        assert np.allclose(zf, g[f"butter8sos_{kind}_zf"], rtol=0, atol=1e-12)


def coverage_cases():
    g = ic.golden()
    for name in ic.GAUSS_BA:
        yield name, (lambda x, dt, n=name: ic.lfilter(g[f"{n}_b"], g[f"{n}_a"], x, dtype=dt)[0])
    yield "butter8sos", (lambda x, dt: ic.sosfilt(g["butter8sos_sos"], x, dtype=dt)[0])
    yield "butter8sos x 5", (lambda x, dt: ic.sosfilt(np.tile(g["butter8sos_sos"], (5, 1)), x, dtype=dt)[0])
    b40 = ic.gauss_data((40,), 52)
    yield "nb = 40 over butter4", (lambda x, dt: ic.lfilter(b40, g["butter4_a"], x, dtype=dt)[0])


def test_gaussian_filters_are_covered_by_float32():
    """the float32 SEQUENTIAL recurrence (the oracle in complex64) is within a quarter of the float32 tolerance of the
    float64 one on every Gaussian filter of the GPU tests: the reference arithmetic alone stays inside the bound"""
    x = ic.gauss_data((1, ic.COVERAGE_N), 5)
    for name, run in coverage_cases():
        ref, got = run(x, np.complex128), run(x, np.complex64)
        err = fc.normwise(torch.from_numpy(got.astype(np.complex128)), torch.from_numpy(ref))
        print(f"iir_coverage {name}: {err:.3g}")
        assert got.dtype == np.complex64 and err <= ic.COVERAGE_BOUND, name


def test_emulated_scheme_on_gaussian_filters():
    """the chunk-parallel scheme in float32 stays at the sequential float32 error (split path included)"""
    g = ic.golden()
    x = ic.gauss_data((1, 6000), 6)
    for name in ("butter8", "cheby4", "dcblock", "cpole"):
        b, a = g[f"{name}_b"], g[f"{name}_a"]
        sec = ic.pad_section(b, a)
        ref, zf = ic.lfilter(b, a, x)
        for force in (0, 3):
            y, f = ic.emulate(x[0], [sec], None, hostiir.plan(6000, len(sec[1]) - 1, force_segments=force))
            assert fc.normwise(torch.from_numpy(y.astype(np.complex128)), torch.from_numpy(ref[0])) <= ic.COVERAGE_BOUND
            assert fc.normwise(torch.from_numpy(f.astype(np.complex128)), torch.from_numpy(zf)) <= fc.F32_TOL


# ---- the gradient identities ------------------------------------------------------------------------------------------
def test_gradient_identities_by_inner_products():
    """<g, dy> = Re sum conj(g) dy for a perturbation of each operand equals <gradient, perturbation> with
    dx = R(b, a; g), gt = R(1, a; g), dzi = gt[:D], db[k] = sum conj(x[n - k]) gt[n], da[k] = -sum conj(y[n - k]) gt[n]"""
    rs = np.random.RandomState(3)
    c = lambda *s: rs.randn(*s) + 1j * rs.randn(*s)       # noqa: E731
    n, d = 60, 3
    b, a = c(d + 1), np.concatenate([[1], 0.3 * c(d)])
    x, zi, g = c(1, n), c(1, d), c(1, n)
    inner = lambda u, v: float(np.real(np.sum(np.conj(u) * v)))                # noqa: E731
    y = ic.lfilter(b, a, x, zi)[0]
    dx = ic.lfilter(b, a, g, reverse=True, conj=True)[0]
    gt = ic.lfilter([1], a, g, reverse=True, conj=True)[0]
    db = np.array([np.sum(np.conj(x[0, :n - k]) * gt[0, k:]) for k in range(d + 1)])
    da = np.array([-np.sum(np.conj(y[0, :n - k]) * gt[0, k:]) for k in range(d + 1)])
    eps = 1e-6
    for what, grad, bump in (("x", dx, lambda e: ic.lfilter(b, a, x + e, zi)[0]), ("zi", gt[:, :d], lambda e: ic.lfilter(b, a, x, zi + e)[0]),
                             ("b", db, lambda e: ic.lfilter(b + e, a, x, zi)[0]),
                             ("a", da, lambda e: ic.lfilter(b, a + np.concatenate([[0], e[1:]]), x, zi)[0])):
        e = c(*np.shape(grad))
        lhs = inner(g, (bump(eps * e) - bump(-eps * e)) / (2 * eps))
        rhs = inner(grad[1:] if what == "a" else grad, e[1:] if what == "a" else e)
        assert abs(lhs - rhs) <= 1e-8 * max(1.0, abs(lhs)), what
    # the reverse | conj run is the adjoint of the plain one: <R(b, a; g), x> = <g, F(b, a; x)> from zero state
    assert abs(inner(dx, x) - inner(g, ic.lfilter(b, a, x)[0])) <= 1e-10 * abs(inner(dx, x))
    # zf from the last D samples (and zi where the row is shorter than D)
    for m in (n, 2):
        ym, zf = ic.lfilter(b, a, x[:, :m], zi)
        want = np.zeros(d, dtype=complex)
        for i in range(d):
            for k in range(i + 1, d + 1):
                if m + i - k >= 0:
                    want[i] += b[k] * x[0, m + i - k] - a[k] * ym[0, m + i - k]
            if i + m < d:
                want[i] += zi[0, i + m]
        assert np.allclose(zf[0], want, rtol=0, atol=1e-12)
    # zi enters as an added sequence: the all-pole filter applied to zi followed by zeros
    seq = np.concatenate([zi, np.zeros((1, n - d))], 1)
    assert np.allclose(ic.lfilter(b, a, x, zi)[0], ic.lfilter(b, a, x)[0] + ic.lfilter([1], a, seq)[0], rtol=0, atol=1e-12)


# ---- the argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors():
    x, b, a = torch.zeros(4, 64), torch.ones(3), torch.tensor([1.0, -0.5])
    with pytest.raises(CplxAmdError, match="torch complex"):
        cplx.lfilter(b, a, torch.zeros(4, 64, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.lfilter([1.0], a, x)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.lfilter(b.double(), a, x)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.lfilter(b, a, Cplx(x, x.double()))
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.lfilter(b.half(), a.half(), x.half())
    with pytest.raises(CplxAmdError, match="sosfilt"):
        cplx.lfilter(b, torch.ones(10), x)
    with pytest.raises(ValueError, match="0-d"):
        cplx.lfilter(b, a, torch.zeros(()))
    with pytest.raises(ValueError, match="empty"):
        cplx.lfilter(b, torch.zeros(0), x)
    with pytest.raises(ValueError, match="zi"):
        cplx.lfilter(b, a, x, torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        cplx.lfilter(torch.ones(3, 3), a, x)
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.lfilter(b, a, x)                             # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError, match="n_sections, 6"):
        cplx.sosfilt(torch.ones(2, 5), x)
    with pytest.raises(ValueError, match="no sections"):
        cplx.sosfilt(torch.ones(0, 6), x)
    with pytest.raises(ValueError, match="zi"):
        cplx.sosfilt(torch.ones(2, 6), x, torch.zeros(4, 3, 2))
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.sosfilt(torch.ones(2, 6), x)
