"""The host side of cplx.czt / zoom_fft / czt_points (cplxmodule_amd/czt.py, cplxamd_czt_plan, cplxamd_czt's argument
checks): no GPU.  The plan at the seams, every argument error and the contour guard raised with no device, scipy's
parameter mapping, and the tests' own reference functions (czt_cases.py) against numbers recorded from scipy
(tests/golden/czt_scipy.npz, scripts/gen_czt_golden.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import czt_cases as cc

from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import czt as hostczt
from cplxmodule_amd._lib import CplxAmdError


# ---- the plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
def test_plan_paths_and_packing_at_the_seams(dtype):
    for (n, m), (path, vpw) in cc.PLAN.items():
        got = hostczt.plan(n, m, 3, dtype)
        assert got[:2] == (path, vpw), (n, m, got)
        assert vpw == cc.vectors_per_workgroup(n, m)
        assert hostczt.transform_size(n, m) == cc.transform_size(n, m)


@pytest.mark.parametrize("dtype,cs", [(torch.float32, 8), (torch.bfloat16, 8), (torch.float64, 16)], ids=["f32", "bf16", "f64"])
def test_plan_workspace_bytes(dtype, cs):
    al = lambda b: (b + 255) & ~255  # noqa: E731
    for (n, m), (path, _) in cc.PLAN.items():
        M = cc.transform_size(n, m)
        tables = 2 * al(M * cs) + al(n * cs) + al(m * cs)          # twiddles, B-hat, opening, closing
        for vectors in (0, 1, 3, 100000):
            want = tables
            if path == "workspace":                               # two buffers of GL vectors, within 256 MiB
                GL = max(1, min((256 << 20) // (2 * M * cs), max(vectors, 1), 65535))
                want += 2 * al(GL * M * cs)
            assert hostczt.plan(n, m, vectors, dtype)[2] == want, (n, m, vectors)


def test_plan_rejects():
    L = _lib.load()
    assert L.cplxamd_czt_plan(0, 4, 1, _lib.F32, None, None) == -1
    assert L.cplxamd_czt_plan(4, 0, 1, _lib.F32, None, None) == -1
    assert L.cplxamd_czt_plan(4, 4, -1, _lib.F32, None, None) == -1
    assert L.cplxamd_czt_plan(4, 4, 1, _lib.F16, None, None) == -1
    assert L.cplxamd_czt_plan(1 << 21, (1 << 21) + 1, 1, _lib.F32, None, None) == 2      # n + m - 1 = 2^22: the last
    assert L.cplxamd_czt_plan(1 << 21, (1 << 21) + 2, 1, _lib.F32, None, None) == -3
    assert L.cplxamd_czt_plan((1 << 22) + 1, 1, 1, _lib.F64, None, None) == -3
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        hostczt.plan(1 << 21, (1 << 21) + 2, 1)


# ---- cplxamd_czt checks every argument before any launch ---------------------------------------------------------------
def _desc(**kw):
    d = _lib.CztDesc(n=4, m=5, x_es=1, y_es=1, scale=1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _czt(d, x_r=256, x_i=256, y_r=256, y_i=256, in_dtype=_lib.F32, out_dtype=_lib.F32, ws=256, ws_bytes=1 << 20):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return _lib.load().cplxamd_czt(p(x_r), p(x_i), p(y_r), p(y_i), ctypes.byref(d), in_dtype, out_dtype, p(ws), ws_bytes, None)


def test_cabi_rejects_without_a_gpu():
    assert _czt(_desc(), x_r=0) == -1
    assert _czt(_desc(), y_r=0) == -1
    assert _czt(_desc(), y_i=0) == -1
    assert _czt(_desc(), ws=0) == -1
    assert _lib.load().cplxamd_czt(*([ctypes.c_void_p(256)] * 4), None, 0, 0, ctypes.c_void_p(256), 1 << 20, None) == -1
    assert _czt(_desc(), in_dtype=_lib.F16, out_dtype=_lib.F16) == -1
    assert _czt(_desc(), in_dtype=_lib.F32, out_dtype=_lib.F64) == -1
    assert _czt(_desc(), in_dtype=_lib.F64, out_dtype=_lib.BF16) == -1
    for bad in (dict(n=0), dict(m=0), dict(x_es=-1), dict(y_es=0), dict(runs=4), dict(runs=-1), dict(flags=2),
                dict(w_log=math.inf), dict(w_turn=math.nan), dict(a_log=-math.inf), dict(a_turn=math.nan),
                dict(scale=math.nan)):
        assert _czt(_desc(**bad)) == -1, bad
    d = _desc(runs=1)
    d.size[0] = -1
    assert _czt(d) == -1
    assert _czt(_desc(n=1 << 21, m=(1 << 21) + 2)) == -3
    d = _desc(runs=2)
    d.size[0], d.size[1] = 1 << 20, 1 << 12                # 2^32 vectors
    assert _czt(d) == -3
    assert _czt(_desc(), ws_bytes=1023) == -4               # the plan of (4, 5) asks for 1024 bytes
    # zero vectors: nothing is launched (there is no GPU here), with and without the null imaginary plane
    d = _desc(runs=1)
    d.size[0] = 0
    assert _czt(d) == 0 and _czt(d, x_i=0) == 0


# ---- argument errors of the public functions, all raised with no device ------------------------------------------------
def _z(*shape, dtype=torch.float32):
    return Cplx(torch.zeros(*shape, dtype=dtype), torch.zeros(*shape, dtype=dtype))


def test_value_errors_in_scipys_words():
    with pytest.raises(ValueError, match=r"Invalid number of CZT output points \(0\) specified"):
        cplx.czt(_z(2, 8), 0)
    with pytest.raises(ValueError, match=r"Invalid number of CZT output points \(-3\) specified"):
        cplx.zoom_fft(_z(2, 8), 0.5, -3)
    with pytest.raises(ValueError, match=r"Invalid number of CZT output points \(2.5\) specified"):
        cplx.czt(torch.zeros(8), 2.5)
    with pytest.raises(ValueError, match=r"Invalid number of CZT data points \(0\) specified"):
        cplx.czt(_z(2, 0))
    with pytest.raises(ValueError, match="0-d"):
        cplx.czt(torch.tensor(1.0))
    with pytest.raises(ValueError, match="fn must be a scalar or 2-length sequence"):
        cplx.zoom_fft(_z(2, 8), (0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match=r"Invalid number of CZT output points \(0\) specified"):
        cplx.czt_points(0)


def test_cplxamd_errors_without_a_device():
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.czt(_z(2, 8))
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.zoom_fft(torch.zeros(2, 8), (0.1, 0.3), 4)
    with pytest.raises(CplxAmdError, match="float16"):
        cplx.czt(_z(2, 8, dtype=torch.float16))
    with pytest.raises(CplxAmdError, match="complex"):
        cplx.czt(torch.zeros(2, 8, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.czt([1.0, 2.0])
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.czt(Cplx(torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.float64)))
    with pytest.raises(CplxAmdError, match="`w` is a tensor"):
        cplx.czt(_z(2, 8), w=torch.tensor(1.0))
    with pytest.raises(CplxAmdError, match="`a` is a tensor"):
        cplx.czt(_z(2, 8), a=torch.tensor(1.0))
    with pytest.raises(CplxAmdError, match="`a` is a tensor"):
        cplx.czt_points(4, a=torch.tensor(1.0))
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.czt(torch.zeros(1, 3 << 20), 3 << 20, w=1j)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.zoom_fft(torch.zeros(1, 1 << 21), 0.5, (1 << 21) + 2)


def test_contour_guard():
    """D = |ln|w|| max(n, m)^2 / 2 + |ln|a|| n against ln 2^24 (float32, bf16) and ln 2^53 (float64), named in the error"""
    n, m = 1000, 24
    w = 0.01 ** (1.0 / (n * m))                             # |w|^{nm} = 0.01: scipy's float64 result is off by 1e24
    D = abs(math.log(w)) * n * n / 2
    assert hostczt.spread(n, m, math.log(w), 0.0) == pytest.approx(D) and D > 53 * math.log(2)
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        with pytest.raises(CplxAmdError, match=r"D = .* = 95\.9"):
            cplx.czt(torch.zeros(2, n, dtype=dtype), m, w)
    # between the two limits: float32 refuses, float64 goes on (to the device check)
    w = math.exp(2 * 20.0 / n ** 2)
    with pytest.raises(CplxAmdError, match="ln 2\\^24"):
        cplx.czt(torch.zeros(2, n), m, w)
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.czt(torch.zeros(2, n, dtype=torch.float64), m, w)
    # |a| alone
    with pytest.raises(CplxAmdError, match="ln 2\\^24"):
        cplx.czt(torch.zeros(2, 100), 10, None, math.exp(0.17))
    with pytest.raises(CplxAmdError, match="MI355X only"):
        cplx.czt(torch.zeros(2, 100), 10, None, math.exp(0.16))
    # the limits themselves
    assert hostczt.D_MAX[torch.float32] == hostczt.D_MAX[torch.bfloat16] == pytest.approx(16.635532)
    assert hostczt.D_MAX[torch.float64] == pytest.approx(36.736801)
    for name in ("spiral_in", "spiral_out"):
        for n, m in cc.SHAPES:
            assert cc.spread(name, n, m) <= cc.D_TEST + 1e-9


# ---- scipy's parameter mapping -----------------------------------------------------------------------------------------
def test_zoom_params_are_scipys_turn_fractions():
    assert hostczt.zoom_params(16, (0.2, 0.6), None, 2.0, False) == (16, -((0.6 - 0.2) / 2.0) / 16, 0.1)
    assert hostczt.zoom_params(16, 0.5, 8) == (8, -0.25 / 8, 0.0)
    m, w_turn, a_turn = hostczt.zoom_params(50, (100.0, 180.0), 64, 1000.0, True)
    assert (m, w_turn, a_turn) == (64, -((80.0 * 64) / (1000.0 * 63)) / 64, 0.1)
    assert hostczt.zoom_params(8, torch.tensor(0.5), 4)[1] == -0.25 / 4
    assert hostczt.zoom_params(8, np.array([0.25, 0.75]), 4) == (4, -0.25 / 4, 0.125)
    with pytest.raises(ValueError):
        hostczt.zoom_params(8, (), 4)


def test_polar_gives_log_modulus_and_turn_fraction():
    assert hostczt._polar(1 + 0j, "a", "czt") == (0.0, 0.0)
    lg, turn = hostczt._polar(2j, "a", "czt")
    assert lg == pytest.approx(math.log(2)) and turn == 0.25
    assert hostczt._polar(-0.5 + 0j, "a", "czt")[1] == 0.5
    with pytest.raises(ValueError):
        hostczt._polar(0j, "w", "czt")


def _args(arg):
    """a fixture row -> (kind, m, the four numbers the kernel would receive)"""
    kind, m = arg[0], int(arg[1])
    if kind == 0.0:
        w = None if np.isnan(arg[2]) else complex(arg[2], arg[3])
        w_log, w_turn = (0.0, -1.0 / m) if w is None else hostczt._polar(w, "w", "czt")
        return m, (w_log, w_turn) + hostczt._polar(complex(arg[4], arg[5]), "a", "czt")
    return m, None


def test_reference_functions_against_scipy(golden):
    g = golden("czt_scipy")
    for i in range(int(g["cases"])):
        x, arg, y = torch.from_numpy(g[f"x{i}"]), g[f"arg{i}"], torch.from_numpy(g[f"y{i}"])
        m, p = _args(arg)
        if p is None:
            f1, f2, fs, endpoint = arg[2:6]
            _, w_turn, a_turn = hostczt.zoom_params(x.shape[-1], (f1, f2), m, fs, bool(endpoint))
            p = (0.0, w_turn, 0.0, a_turn)
        assert y.shape == (2, m)
        # scipy's own chirps carry the rounding of pi k^2 scale / m: 1e-12 is far above it at these sizes
        assert cc.normwise(cc.direct(x, m, *p), y) < 1e-12, i
        assert cc.normwise(cc.bluestein(x, m, *p), y) < 1e-12, i


def test_czt_points_against_scipy(golden):
    g = golden("czt_scipy")
    for j in range(int(g["point_sets"])):
        arg, want = g[f"pts_arg{j}"], torch.from_numpy(g[f"pts{j}"])
        w = None if np.isnan(arg[1]) else complex(arg[1], arg[2])
        got = cplx.czt_points(int(arg[0]), w, complex(arg[3], arg[4]))
        assert got.dtype == torch.complex128 and got.shape == want.shape and not got.is_cuda
        assert float((got - want).abs().max()) < 1e-14 * float(want.abs().max())


def test_adjoint_reference_is_the_conjugate_transpose():
    n, m = 9, 6
    p = cc.contour_params("spiral_in", n, m)
    x, g = torch.randn(2, n, dtype=torch.complex128), torch.randn(2, m, dtype=torch.complex128)
    lhs = (cc.direct(x, m, *p) * g.conj()).sum()              # <K x, g> = <x, K^H g>
    rhs = (x * cc.adjoint(g, n, *p).conj()).sum()
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_exact_phase_reduction():
    """turns(theta, q) against exact rational arithmetic, where the plain product is off by up to 2^-11 turns (half an
    ulp of 2^43)"""
    from fractions import Fraction
    theta = -0.4871
    q = torch.tensor([(1 << 22) - 1, 4194301, 3000017, 12345], dtype=torch.int64) ** 2
    got = cc.turns(theta, q)
    naive = theta * q.double()
    naive = naive - torch.round(naive)
    worst = 0.0
    for v, nv, qi in zip(got.tolist(), naive.tolist(), q.tolist()):
        exact = Fraction(theta) * qi
        exact -= round(exact)
        assert abs(float(Fraction(v) - exact)) < 1e-15
        worst = max(worst, abs(float(Fraction(nv) - exact)))
    assert worst > 1e-4                                         # what the exact reduction is for


@pytest.mark.parametrize("n,m", [(1, 1), (5, 1), (3, 7), (100, 37), (37, 100), (512, 513), (1100, 1000)])
def test_bluestein_reference_against_the_direct_sum(n, m):
    """the reference of the two largest float32 cases, validated where the direct sum is cheap; and the drift table of
    the float64 bound, re-measured at the small sizes"""
    for name in cc.CONTOURS:
        p = cc.contour_params(name, n, m)
        if p is None:
            assert name == "zoom_endpoint" and m == 1
            continue
        re, im, ref, ref_real = cc.case(n, m, torch.float64, name)
        for z, want in ((cc.c128(re, im), ref), (cc.c128(re, torch.zeros_like(re)), ref_real)):
            err = cc.normwise(cc.bluestein(z, m, *p), want)
            assert err <= cc.f64_tol(), (name, err)


def test_f64_bound_is_four_times_the_measured_drift():
    assert set(cc.F64_DRIFT) == set(cc.SHAPES) - set(cc.F32_ONLY)
    assert cc.f64_tol() == 4.0 * 2.59e-15
