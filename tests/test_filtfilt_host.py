"""cplx.filtfilt / sosfiltfilt / lfilter_zi / sosfilt_zi without a GPU: the oracle of filtfilt_cases.py against scipy's
recorded outputs, the closed-form steady states on CPU tensors against scipy's, the exported index map of the extension
against numpy's for every logical index, the plan (cplxamd_filtfilt_plan is a pure function), the rejections of the
launcher (it returns before any launch), every argument error on CPU inputs, the coverage condition of the Gaussian
filters, and the exactness precondition of test_gpu_filtfilt.py's integer cases on their very data."""
import ctypes

import numpy as np
import pytest
import torch

import fft_cases as fc
import filtfilt_cases as ff
import iir_cases as ic

from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import filtfilt as hostff
from cplxmodule_amd import iir as hostiir
from cplxmodule_amd._lib import CplxAmdError


def close(got, ref, atol=1e-12):
    return np.allclose(got, ref, rtol=0, atol=atol)


def t64(z, real=False):
    z = np.asarray(z, dtype=np.complex128)
    re = torch.from_numpy(z.real.copy())
    return re if real else Cplx(re, torch.from_numpy(z.imag.copy()))


def c128(y):
    return y.numpy() + 0j if torch.is_tensor(y) else y.real.numpy() + 1j * y.imag.numpy()


# ---- the oracle and the closed forms against scipy ----------------------------------------------------------------------------
def test_oracle_against_golden_scipy():
    g = ff.golden()
    padlen = int(g["padlen"])
    for name in ic.GAUSS_BA:
        b, a = g[f"{name}_b"], g[f"{name}_a"]
        assert close(ff.lfilter_zi(b, a), g[f"{name}_zi"])
        for kind in ("real", "cplx"):
            for padtype in ff.PADTYPES:
                for tag, pl in (("default", None), ("padlen", padlen)):
                    ref = g[f"{name}_{kind}_{ff.key(padtype)}_{tag}"]
                    assert close(ff.filtfilt(b, a, g[f"x_{kind}"], padtype, pl), ref), (name, kind, padtype, tag)
    sos = g["butter8sos_sos"]
    assert close(ff.sosfilt_zi(sos), g["butter8sos_zi"])
    assert int(g["butter8sos_default_padlen"]) == ff.default_padlen(sections=len(sos))    # no zero b2 / a2 in this design
    for kind in ("real", "cplx"):
        for padtype in ff.PADTYPES:
            for tag, pl in (("default", None), ("padlen", padlen)):
                ref = g[f"butter8sos_{kind}_{ff.key(padtype)}_{tag}"]
                assert close(ff.sosfiltfilt(sos, g[f"x_{kind}"], padtype, pl), ref), (kind, padtype, tag)


def test_zi_closed_forms_on_cpu_tensors_against_scipy():
    g = ff.golden()
    for name in ic.GAUSS_BA:
        b, a = g[f"{name}_b"], g[f"{name}_a"]
        real = not (np.iscomplexobj(b) or np.iscomplexobj(a))
        zi = cplx.lfilter_zi(t64(b, real), t64(a, real))
        assert torch.is_tensor(zi) == real and close(c128(zi), g[f"{name}_zi"]), name
        assert close(c128(cplx.lfilter_zi(t64(3 * b, real), t64(3 * a, real))), g[f"{name}_zi"]), name   # a0 normalises
    # complex b over a real a, and the reverse
    zi = cplx.lfilter_zi(t64(g["cpole_b"]), t64(g["cpole_a"].real + 0.5, True))
    assert close(c128(zi), ff.lfilter_zi(g["cpole_b"], g["cpole_a"].real + 0.5))
    # batched filters, leading dims broadcast: [3, 5] taps against [2, 1, 5]
    names = ("butter4", "cheby4", "ellip4")
    bb, aa = (np.stack([g[f"{n}_{k}"] for n in names]) for k in "ba")
    zi = cplx.lfilter_zi(t64(bb, True), t64(aa[:2, None], True))
    assert zi.shape == (2, 3, 4) and close(zi.numpy()[1, 2], ff.lfilter_zi(bb[2], aa[1]).real)
    zi = cplx.lfilter_zi(t64(bb, True), t64(aa, True))
    assert zi.shape == (3, 4) and close(zi.numpy(), np.stack([g[f"{n}_zi"] for n in names]))
    assert cplx.lfilter_zi(torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)).shape == (0,)
    sos = g["butter8sos_sos"]
    assert close(cplx.sosfilt_zi(t64(sos, True)).numpy(), g["butter8sos_zi"])
    both = np.stack([sos, sos[::-1] * 0.5])
    zi = cplx.sosfilt_zi(t64(both, True))
    assert zi.shape == (2, 4, 2) and close(zi.numpy()[1], ff.sosfilt_zi(both[1]).real)
    csos = ic.int_sos("three")
    assert close(c128(cplx.sosfilt_zi(t64(csos))), ff.sosfilt_zi(csos))
    # differentiable
    b = torch.tensor([0.2, 0.3, 0.1], dtype=torch.float64, requires_grad=True)
    a = torch.tensor([1.5, -0.4, 0.3], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(cplx.lfilter_zi, [b, a])
    s = torch.tensor([[0.5, 0.3, 0.2, 1.5, -0.4, 0.3], [1.0, -0.5, 0.1, 0.8, 0.2, 0.1]], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(cplx.sosfilt_zi, [s])
    # exact on the integer filters of the GPU tests: Gaussian integers or half-integers
    for name in ff.EXACT_FILTERS:
        b, a, _ = ic.INT_FILTERS[name]
        tb, ta = t64(b), t64(a)
        zi = c128(cplx.lfilter_zi(Cplx(tb.real.float(), tb.imag.float()), Cplx(ta.real.float(), ta.imag.float())))
        assert np.array_equal(zi, ff.lfilter_zi(b, a)) and np.array_equal(2 * zi, np.round(2 * zi)), name


# ---- the index map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padtype", ["odd", "even", "constant"])
def test_exported_index_map_equals_numpy_extension(padtype):
    for n, e in ff.MAP_CASES + ((1, 0), (5, 0), (4096, 0)):
        x = ic.int_data((2, n), n + e)
        exported = ff.from_map(x, e, padtype, hostff.src_index)
        assert np.array_equal(exported, ff.extend(x, e, padtype)), (n, e)
        assert np.array_equal(exported, ff.from_map(x, e, padtype)), (n, e)
        assert all(hostff.src_index(m, n, e, padtype) == ff.src(m, n, e, padtype) for m in range(n + 2 * e))
    out = (ctypes.c_int64 * 2)()
    src = _lib.load().cplxamd_filtfilt_src
    assert src(0, 7, 6, 0, out) == 0 and tuple(out) == (6, 0)
    for m, n, e, mode in ((-1, 7, 6, 0), (19, 7, 6, 0), (0, 7, 7, 0), (0, 0, 0, 0), (0, 7, -1, 0), (0, 7, 6, 3)):
        assert src(m, n, e, mode, out) == -1, (m, n, e, mode)
    assert src(0, 7, 6, 0, None) == -1
    with pytest.raises(CplxAmdError):
        hostff.src_index(19, 7, 6, "odd")


# ---- the plan -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
def test_plan_fields_and_workspace_bytes(dtype):
    word = 8 if dtype == torch.float64 else 4
    for order, sections in ((1, 1), (2, 1), (8, 1), (2, 16)):
        for cx in (False, True):
            planes = 2 if cx else 1
            n, e, rows = 60000, 27, 1024
            p = hostff.plan(n, e, order, sections, rows, 1, dtype, cx)
            q = hostiir.plan(n + 2 * e, order, sections, rows, 1, dtype, cx)
            for field in _lib.IIR_PLAN_FIELDS:
                if field != "lds_bytes":
                    assert p[field] == q[field], field
            assert p["lds_bytes"] == q["lds_bytes"] + 2 * planes * word <= 76 * 1024      # the two anchors per plane
            assert p["ext_len"] == n + 2 * e and p["path"] == "row"
            assert p["signal_bytes"] == rows * (n + 2 * e) * planes * word                # the compute type: 4 for bf16
    p = hostff.plan(5003, 9, 2, 1, 3, 1, force_segments=7)
    assert p["path"] == "split" and (p["segments"], p["seg_len"], p["grid"]) == (7, 718, 21) and p["ext_len"] == 5021
    assert p["ws_bytes"] == hostiir.plan(5021, 2, 1, 3, 1, force_segments=7)["ws_bytes"] > 0
    assert hostff.plan(1 << 22, 27, 2, 4, 1, 1)["path"] == "split"
    for n, e in ((0, 0), (5, 5), (5, -1)):
        with pytest.raises(CplxAmdError, match="no plan"):
            hostff.plan(n, e, 2)
    for order, sections in ((9, 1), (0, 1), (3, 2), (2, 17)):
        with pytest.raises(CplxAmdError, match="no plan"):
            hostff.plan(100, 9, order, sections)
    with pytest.raises(CplxAmdError, match="exceed"):
        hostff.plan(1 << 40, 1, 2)
    assert _lib.load().cplxamd_filtfilt_plan(100, 9, 2, 1, 1, 1, _lib.F32, 1, 0, None) == -1


def test_launcher_rejects_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    fields = dict(n=100, edge=9, y_lo=9, y_n=100, order=2, sections=1, segments=1, seg_len=118, x_es=1, runs=0,
                  flags=_lib.FILTFILT_SCALE, mode=0, reserved=0)
    d = _lib.FiltFiltDesc(**fields)
    assert ctypes.sizeof(d) == 208
    ok = [one, one, one, one, one, one, one, one, None, None, ctypes.byref(d), 1, _lib.F32, _lib.F32, None]

    def rc(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.cplxamd_filtfilt_pass(*args)

    assert rc(a2=None) == -1 and rc(a10=None) == -1       # no coefficients, no descriptor
    assert rc(a6=None, a7=None) == -1                     # neither y nor zf
    assert rc(a7=None) == -1 and rc(a8=one) == -1         # complex: y_i, zf_i missing
    assert rc(a11=0) == -1 and rc(a11=2) == -1            # real arithmetic forbids the imaginary planes
    assert rc(a0=None) == -1                              # x_i without x_r
    assert rc(a4=None, a5=None) == -1                     # SCALE without a unit state
    for pair in ((_lib.BF16, _lib.BF16), (_lib.F64, _lib.F32), (_lib.F32, _lib.F64), (_lib.F16, _lib.F32), (7, 7)):
        assert rc(a12=pair[0], a13=pair[1]) == -1, pair
    for field, value in (("n", 0), ("edge", -1), ("edge", 100), ("y_lo", -1), ("y_n", 0), ("y_lo", 19), ("y_n", 110),
                         ("order", 9), ("order", 0), ("sections", 17), ("segments", 0), ("segments", 2), ("seg_len", 0),
                         ("seg_len", 117), ("seg_len", 119), ("x_es", -1), ("runs", 4), ("flags", 4), ("mode", 3),
                         ("reserved", 1)):
        bad = _lib.FiltFiltDesc(**dict(fields, **{field: value}))
        assert lib.cplxamd_filtfilt_pass(*ok[:10], ctypes.byref(bad), 1, _lib.F32, _lib.F32, None) == -1, (field, value)
    bad = _lib.FiltFiltDesc(**dict(fields, runs=1))
    bad.size[0], bad.z_stride[0] = 4, -1
    assert lib.cplxamd_filtfilt_pass(*ok[:10], ctypes.byref(bad), 1, _lib.F32, _lib.F32, None) == -1
    bad.size[0], bad.z_stride[0] = 0, 0                   # no rows: nothing to do
    assert lib.cplxamd_filtfilt_pass(*ok[:10], ctypes.byref(bad), 1, _lib.F32, _lib.F32, None) == 0


# ---- the argument errors: raised on CPU inputs, before any device check ---------------------------------------------------------
def test_argument_errors():
    x, b, a = torch.zeros(4, 64), torch.ones(3), torch.tensor([1.0, -0.5])
    sos = torch.tensor([[1.0, 0, 0, 1, -0.5, 0]])
    for run in (lambda **k: cplx.filtfilt(b, a, x, **k), lambda **k: cplx.sosfiltfilt(sos, x, **k)):
        with pytest.raises(ValueError, match="padtype"):
            run(padtype="reflect")
        with pytest.raises(ValueError, match="padlen"):
            run(padlen=-1)
        with pytest.raises(ValueError, match="The length of the input vector x must be greater than padlen, which is 64."):
            run(padlen=64)
        with pytest.raises(CplxAmdError, match="MI355X"):         # valid arguments: only now the device is looked at
            run(padlen=63)
        with pytest.raises(CplxAmdError, match="MI355X"):
            run(padtype=None, padlen=500)                         # no extension: padlen is not read, as in scipy
    with pytest.raises(ValueError, match="which is 9"):
        cplx.filtfilt(b, a, x[:, :9])                             # the default: 3 max(na, nb)
    with pytest.raises(ValueError, match="which is 9"):
        cplx.sosfiltfilt(sos, x[:, :9])                           # the default: 3 (2 n_sections + 1)
    with pytest.raises(CplxAmdError, match="torch complex"):
        cplx.filtfilt(b, a, torch.zeros(4, 64, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.filtfilt(b.double(), a, x)
    with pytest.raises(CplxAmdError):
        cplx.filtfilt(b.half(), a.half(), x.half())
    with pytest.raises(CplxAmdError, match="sosfiltfilt"):
        cplx.filtfilt(b, torch.ones(10), x)
    with pytest.raises(ValueError, match="empty"):
        cplx.filtfilt(torch.ones(0), a, x)
    with pytest.raises(ValueError, match="0-d"):
        cplx.filtfilt(b, a, torch.zeros(()))
    with pytest.raises(RuntimeError):
        cplx.filtfilt(torch.ones(3, 3), a, x)                     # 3 filters against 4 rows
    with pytest.raises(ValueError, match="n_sections, 6"):
        cplx.sosfiltfilt(torch.ones(2, 5), x)
    with pytest.raises(ValueError, match="no sections"):
        cplx.sosfilt_zi(torch.ones(0, 6))
    with pytest.raises(ValueError, match="empty"):
        cplx.lfilter_zi(b, torch.ones(0))
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.lfilter_zi(b.double(), a)


# ---- the coverage condition of the Gaussian cases -------------------------------------------------------------------------------
def f32(z):
    z = np.asarray(z, dtype=np.complex128)
    return z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)


def test_gaussian_filters_are_covered_by_float32():
    """the SEQUENTIAL complex64 filtfilt of every design at N = 8192 stays within a quarter of the float32 tolerance of the
    complex128 one on the same rounded operands, for all four padtypes: the kernel's bound of 1e-5 has room.  (scipy on
    the same designs: 2.3e-7 .. 1.3e-6, 3.2e-7 for the butter8 cascade; butter2 was not measured with scipy.)"""
    g = ic.golden()
    x = f32(ic.gauss_data((1, ff.COVERAGE_N), 5))
    runs = [(name, lambda x, p, dt, n=name: ff.filtfilt(f32(g[f"{n}_b"]), f32(g[f"{n}_a"]), x, p, None, dt))
            for name in ic.GAUSS_BA]
    runs.append(("butter8sos", lambda x, p, dt: ff.sosfiltfilt(f32(g["butter8sos_sos"]), x, p, None, dt)))
    for name, run in runs:
        for padtype in ff.PADTYPES:
            ref, got = run(x, padtype, np.complex128), run(x, padtype, np.complex64)
            err = fc.normwise(torch.from_numpy(got.astype(np.complex128)), torch.from_numpy(np.ascontiguousarray(ref)))
            print(f"filtfilt_coverage {name} {padtype}: {err:.3g}")
            assert got.dtype == np.complex64 and err <= ff.COVERAGE_BOUND, (name, padtype)


# ---- the exactness precondition of the integer GPU cases --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("ba", n) for n in ff.EXACT_FILTERS] + [("sos", n) for n in ff.EXACT_CASCADES])
def test_integer_cases_have_headroom(kind, name):
    """on the very data of test_gpu_filtfilt.py's exact tests every value on the way -- the extension, both passes, the
    states -- is a multiple of the filter's quantum, and the sum of the D products of a state with an entry of the chunk
    tables stays below 2^24 quanta (test_iir_host.py's bound): float32 holds every intermediate of the chunked scheme
    exactly, EQUAL is the right comparison.  The reference below 2^24 alone does not do: the cascade `two` at N =
    3 * 4096 + 77 peaks at 1.3e7 and its float32 run differs from the oracle in the last bit.  The cases of the list that the
    bound does not admit are filtfilt_cases.EXCLUDED, each shown here to miss it; they run in float64, which holds all."""
    q = ff.QUANTUM.get(name if kind == "ba" else None, 1.0)
    f = ff.exact_filter(kind, name)
    secs = [(s[:3], s[3:]) for s in f] if kind == "sos" else [f]
    d = max(len(ic.pad_section(b, a)[1]) - 1 for b, a in secs)
    gain = max(ic.table_gain(ic.pad_section(b, a)[1]) for b, a in secs)
    zi = ff.sosfilt_zi(f) if kind == "sos" else ff.lfilter_zi(*f)
    assert np.array_equal(zi / np.sqrt(q), np.round(zi / np.sqrt(q)))     # the unit state: multiples of sqrt(quantum)
    split = (ff.SPLIT_N, None)
    for n, padlen in ff.exact_cases(kind, name, float64=True) + [split]:
        out, peak = ff.exact_reference(kind, name, n, padlen)
        need = d * max(gain, 1) * peak / q
        assert (need < 2 ** 24) == ff.admitted(kind, name, (n, padlen)), (kind, name, n, padlen, peak)
        assert need < 2 ** 53
        for y in out.values():
            assert np.array_equal(y / q, np.round(y / q))
