"""cplx.fftconvolve without a GPU: the plan (cplxamd_fftconv_plan is a pure function), the overlap-save geometry it lays
out -- emulated in numpy from the plan's numbers alone and compared with numpy.convolve --, every argument error with its
exception type, the descriptor and NULL-pointer rejections of the launchers (they return before any launch), and the
headroom of the integer cases of test_gpu_fftconv.py."""
import ctypes

import numpy as np
import pytest
import torch

import fftconv_cases as cc

from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import fftconv as hostconv
from cplxmodule_amd._lib import CplxAmdError


# ---- the plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(cc.PLAN_TABLE), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_plan_table(case):
    a_len, k, mode = case
    start, length = cc.window(a_len, k, mode)
    p = hostconv.plan(a_len, k, start, length)
    assert (p["path"], p["L"], p["S"], p["blocks"], p["vectors_per_workgroup"]) == cc.PLAN_TABLE[case]
    if p["path"] == "fused":
        assert p["L"] >= k and p["S"] == p["L"] - k + 1 and p["L"] <= 8192
        assert p["blocks"] == 1 or p["blocks"] == -(-length // p["S"])
        assert p["ws_bytes"] >= 2 * p["L"] * 8             # twiddles and one filter spectrum


def test_plan_packing_seam_and_dtypes():
    # 1024 points: two blocks per 256-thread workgroup; 2048: one block per workgroup of 256 threads
    assert hostconv.plan(50000, 256, 0, 50255)["vectors_per_workgroup"] == 2
    assert hostconv.plan(50000, 257, 0, 50256)["vectors_per_workgroup"] == 1
    for log_l, vpw in ((2, 256), (3, 256), (4, 128), (8, 8), (10, 2), (11, 1), (13, 1)):
        assert hostconv.plan(50000, 3, 0, 50002, log_l=log_l)["vectors_per_workgroup"] == vpw
    # float64: the same geometry, spectra of twice the size
    f32, f64 = hostconv.plan(5000, 255, 0, 5254, 4, 2), hostconv.plan(5000, 255, 0, 5254, 4, 2, torch.float64)
    assert all(f32[key] == f64[key] for key in ("L", "S", "blocks", "vectors_per_workgroup", "in_shift", "out_lo"))
    assert f64["ws_bytes"] == 2 * f32["ws_bytes"] == 2 * (1024 * 8 + 2 * 1024 * 8)
    assert hostconv.plan(5000, 255, 0, 5254, dtype=torch.bfloat16)["ws_bytes"] == hostconv.plan(5000, 255, 0, 5254)["ws_bytes"]


def test_plan_log_l_override():
    p = hostconv.plan(772, 2, 0, 773, log_l=2)
    assert (p["L"], p["S"], p["blocks"], p["vectors_per_workgroup"]) == (4, 3, 258, 256)
    assert (p["wgrad_log_l"], p["wgrad_S"], p["wgrad_blocks"]) == (2, 3, 258)
    assert hostconv.plan(100, 4, 0, 103, log_l=2)["S"] == 1               # L = K: one output per block
    assert hostconv.plan(100, 7, 0, 106, log_l=13)["L"] == 8192
    for k, log_l in ((5, 2), (7, 14), (4096, 11), (3, -1)):
        with pytest.raises(CplxAmdError):
            hostconv.plan(100 + k, k, 0, 100, log_l=log_l)
    out = (ctypes.c_int64 * len(_lib.FFTCONV_PLAN_FIELDS))()
    lib = _lib.load()
    assert lib.cplxamd_fftconv_plan(100, 5, 0, 104, 1, 1, _lib.F32, 0, 2, out) == -1      # 2^log_l < K
    assert lib.cplxamd_fftconv_plan(100, 5, 0, 104, 1, 1, _lib.F32, 0, 14, out) == -1
    assert lib.cplxamd_fftconv_plan(100, 5, 0, 104, 1, 1, 99, 0, 0, out) == -1            # dtype
    assert lib.cplxamd_fftconv_plan(0, 5, 0, 104, 1, 1, _lib.F32, 0, 0, out) == -1
    assert lib.cplxamd_fftconv_plan(100, 5, 0, 104, -1, 1, _lib.F32, 0, 0, out) == -1
    assert lib.cplxamd_fftconv_plan(100, 5, 0, 104, 1, 1, _lib.F32, 0, 0, None) == -1
    assert lib.cplxamd_fftconv_plan(1 << 22, 4097, 0, 100, 1, 1, _lib.F32, 0, 0, out) == -3   # composed beyond 2^22


def test_plan_weight_gradient_chunks():
    # (b) of the benchmark: 32 x 64 rows of 16384, one filter of 1024 taps per channel: 32 reduced rows per filter
    p = hostconv.plan(16384, 1024, 0, 16384, 32 * 64, 64)
    assert (p["wgrad_log_l"], p["wgrad_S"], p["wgrad_blocks"]) == (12, 3073, 6)
    pairs = 32 * 6
    assert p["wgrad_chunks"] == 12 and p["wgrad_per_chunk"] == 16 and 12 * 16 >= pairs      # 64 x 12 = 768 workgroups
    assert p["wgrad_ws_bytes"] == 4096 * 8 + 64 * 12 * 4096 * 8
    # one shared filter of few taps: blocks of 2048 points, 768 chunks
    p = hostconv.plan(65536, 64, 0, 65536, 256, 1)
    assert (p["wgrad_log_l"], p["wgrad_blocks"]) == (11, 34) and p["wgrad_chunks"] * p["wgrad_per_chunk"] >= 256 * 34
    assert p["wgrad_chunks"] <= 768
    # further chunks are added only while the partials stay within 256 MiB; one partial per result is the floor, so with
    # many results the workspace exceeds that (here 2^14 results x 8192 complex128 x two slabs = 4 GiB)
    p = hostconv.plan(8192, 4096, 0, 8192, 1 << 16, 1 << 14, torch.float64)
    assert p["wgrad_chunks"] == 1 and p["wgrad_per_chunk"] == 4 * p["wgrad_blocks"]
    assert p["wgrad_ws_bytes"] == 8192 * 16 + (1 << 14) * 8192 * 16 * 2
    assert p["ws_bytes"] == 8192 * 16 + (1 << 14) * 8192 * 16
    # beyond 1 TiB of spectra (and sizes whose products leave 64 bits) the plan declines
    out = (ctypes.c_int64 * len(_lib.FFTCONV_PLAN_FIELDS))()
    lib = _lib.load()
    assert lib.cplxamd_fftconv_plan(8192, 4096, 0, 8192, 1 << 26, 1 << 26, _lib.F64, 0, 0, out) == -3
    assert lib.cplxamd_fftconv_plan(8192, 64, 0, 8192, 1 << 62, 1 << 62, _lib.F32, 0, 0, out) == -3
    with pytest.raises(CplxAmdError, match="workspace"):
        hostconv.plan(8192, 4096, 0, 8192, 1 << 26, 1 << 26, torch.float64)
    with pytest.raises(CplxAmdError, match="2\\^22"):
        hostconv.plan(1 << 22, 4097, 0, 100)


# ---- the geometry, from the plan's numbers alone ---------------------------------------------------------------------
def _operands(n, m, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, n) + 1j * rng.integers(-4, 5, n), rng.integers(-4, 5, m) + 1j * rng.integers(-4, 5, m))


@pytest.mark.parametrize("nm", cc.GEOMETRY, ids=lambda c: f"{c[0]}x{c[1]}")
def test_overlap_save_emulation_equals_numpy_convolve(nm):
    for n, m in (nm, nm[::-1]):
        x, h = _operands(n, m, 100 * n + m)
        a, b = (x, h) if n >= m else (h, x)
        full = np.convolve(x, h)
        for mode in cc.MODES:
            start, length = cc.window(n, m, mode)
            assert hostconv.window(n, m, mode) == (start, length)
            ref = full[start:start + length]
            for log_l in (None, 2 if len(b) <= 4 else None, 13):
                p = hostconv.plan(len(a), len(b), start, length, log_l=log_l)
                assert np.abs(cc.emulate(a, b, start, length, False, p) - ref).max() < 1e-6, (mode, log_l, p)
            # the window of the gradient w.r.t. the long operand: a correlation of `length` entries back to len(a)
            g, _ = _operands(length, 1, 7)
            for log_l in (None, 2 if len(b) <= 4 else None):
                p = hostconv.plan(length, len(b), -start, len(a), conj=True, log_l=log_l)
                got = cc.emulate(g, b, -start, len(a), True, p)
                assert np.abs(got - cc.direct(g, b, -start, len(a), True)).max() < 1e-6, (mode, log_l, p)


def test_windows_outside_the_support_are_zeros():
    a, b = _operands(50, 6, 3)
    for start, length, conj in ((-20, 100, False), (40, 60, False), (-30, 120, True), (-5, 20, True), (60, 10, False)):
        p = hostconv.plan(50, 6, start, length, conj=conj)
        assert np.abs(cc.emulate(a, b, start, length, conj, p) - cc.direct(a, b, start, length, conj)).max() < 1e-9


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors():
    x, h = torch.zeros(2, 16), torch.zeros(3)
    with pytest.raises(ValueError, match="mode"):
        cplx.fftconvolve(x, h, "circular")
    with pytest.raises(ValueError, match="0-d"):
        cplx.fftconvolve(x, torch.tensor(1.0))
    with pytest.raises(ValueError, match="empty"):
        cplx.fftconvolve(torch.zeros(2, 0), h)
    with pytest.raises(RuntimeError):
        cplx.fftconvolve(torch.zeros(2, 3, 16), torch.zeros(4, 3))
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.fftconvolve(x, h.double())
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.fftconvolve(Cplx(x, x.double()), h)
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.fftconvolve(x.half(), h.half())
    with pytest.raises(CplxAmdError, match="complex"):
        cplx.fftconvolve(torch.zeros(4, dtype=torch.complex64), h)
    with pytest.raises(CplxAmdError, match="2\\^22"):
        cplx.fftconvolve(torch.zeros(1, device="meta").expand((1 << 22),), torch.zeros(4097, device="meta"))
    with pytest.raises(CplxAmdError, match="no CPU path"):             # there is no host path
        cplx.fftconvolve(x, h)
    with pytest.raises(TypeError):
        cplx.fftconvolve(x, h, "full", 3)                              # log_l is not part of the public signature
    with pytest.raises(CplxAmdError):
        hostconv.fftconvolve(x, h, "full", log_l=1)                    # 2^1 < 3 taps


# ---- the launchers reject before they launch -----------------------------------------------------------------------------
def _desc(**kw):
    d = _lib.FftConvDesc(a_len=100, k=5, c_len=104, start=0, a_es=1, b_es=1, runs=1, conj=0, log_l=0, reserved=0)
    d.size[0], d.a_stride[0], d.b_stride[0], d.y_stride[0] = 3, 100, 0, 104
    for key, v in kw.items():
        setattr(d, key, v)
    return d


@pytest.mark.parametrize("name", ["cplxamd_fftconv", "cplxamd_fftconv_wgrad"])
def test_launchers_reject_bad_arguments_without_a_launch(name):
    fn = getattr(_lib.load(), name)
    assert ctypes.sizeof(_lib.FftConvDesc) == 160
    p = ctypes.c_void_p(4096)                             # never dereferenced: every call below returns before a launch
    d = _desc()
    if name.endswith("wgrad"):
        d.y_stride[0] = 0
    ok = [p, None, p, None, p, None, ctypes.byref(d), _lib.F32, p, 1 << 30, None]
    for null in (0, 2, 4, 6, 8):                          # a_r, b_r, y_r, the descriptor, the workspace
        args = list(ok)
        args[null] = None
        assert fn(*args) == -1, null
    assert fn(*(ok[:7] + [99] + ok[8:])) == -1            # dtype
    assert fn(*(ok[:9] + [64] + ok[10:])) == -4           # a workspace that is too small
    bad = [dict(a_len=0), dict(k=0), dict(c_len=-1), dict(a_es=-1), dict(runs=4), dict(log_l=2), dict(log_l=14),
           dict(reserved=1), dict(k=4097)]
    if name.endswith("wgrad"):
        bad.append(dict(conj=1))
    else:
        bad.append(dict(conj=2))
    for kw in bad:
        d = _desc(**kw)
        args = list(ok)
        args[6] = ctypes.byref(d)
        assert fn(*args) == -1, kw
    d = _desc()
    d.size[0] = -3
    args = list(ok)
    args[6] = ctypes.byref(d)
    assert fn(*args) == -1
    d = _desc()
    d.size[0] = 0                                         # no rows: nothing to do
    args[6] = ctypes.byref(d)
    assert fn(*args) == 0


# ---- the integer cases are exact in float32 --------------------------------------------------------------------------
def test_integer_cases_have_headroom():
    for rows, a_len, k in cc.EXACT + cc.EXACT_BLOCKS:
        xr, xi, hr, hi = cc.exact_case(rows, a_len, k)
        assert float(torch.stack([t.abs().max() for t in (xr, xi, hr, hi)]).max()) <= 4
        x, h = torch.complex(xr, xi), torch.complex(hr, hi)
        for mode in cc.MODES:
            ref = cc.integer_reference(x, h, mode)
            assert float(max(ref.real.abs().max(), ref.imag.abs().max())) < 2 ** 24
            assert torch.equal(ref.real, ref.real.round()) and torch.equal(ref.imag, ref.imag.round())
            assert float((ref - cc.reference(x, h, mode)).abs().max()) < 1e-9       # both references agree
        p = hostconv.plan(a_len, k, 0, a_len + k - 1, rows, 1, log_l=cc.EXACT_LOG_L)
        assert p["L"] == 4
        # the weight gradient of the shared filter sums rows x blocks products of spectra
        assert cc.partial_sum_bound(rows * p["wgrad_blocks"], p["L"]) < 2 ** 24
