"""utils.spectrum and utils.window_view without a GPU: window_view against torch.unfold and the reference's fixture
(tests/golden/spectrum.npz, scripts/gen_spectrum_golden.py) with its errors, fftshift, the host band-to-bin resolution
against torch's own comparisons, the Welch plan (paths, workspace sizes, the 2^22 bound) as a pure host call, the
reference's exception types, and CplxAmdError for CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("cplxamd_welch_plan", "cplxamd_welch_fwd", "cplxamd_welch_bwd")


def _sp():
    from cplxmodule_amd.utils import spectrum
    return spectrum


def test_window_view_matches_unfold():
    from cplxmodule_amd.utils import window_view
    x = torch.randn(2, 3, 1024, 2, 2, dtype=torch.float64)
    dim, size, stride = 2, 5, 2
    v = window_view(x, dim, size, stride)
    assert v.data_ptr() == x.data_ptr()
    for i in range(v.shape[dim]):
        np.testing.assert_array_equal(v.select(dim, i).numpy(), x.narrow(dim, i * stride, size).movedim(dim, dim)
                                      .numpy())
    np.testing.assert_array_equal(window_view(x, dim, size, stride, at=-1).numpy(), x.unfold(dim, size, stride).numpy())
    y = x[:, 1:, 3:900].requires_grad_(False)                  # a non-contiguous view with a storage offset
    np.testing.assert_array_equal(window_view(y, 2, 7, 3, at=-1).numpy(), y.unfold(2, 7, 3).numpy())


def test_window_view_gradient_flows_into_x():
    from cplxmodule_amd.utils import window_view
    x = torch.randn(10, dtype=torch.float64, requires_grad=True)
    window_view(x, 0, 4, 2).sum().backward()
    np.testing.assert_array_equal(x.grad.numpy(), [1, 1, 2, 2, 2, 2, 2, 2, 1, 1])


def test_window_view_fixture(golden):
    from cplxmodule_amd.utils import window_view
    d = golden("spectrum")
    x = torch.from_numpy(d["wv_x"])
    for i, (dim, size, stride, at) in enumerate(d["wv_params"].tolist()):
        got = window_view(x, dim, size, stride, at=None if at == 99 else at)
        np.testing.assert_array_equal(got.numpy(), d[f"wv_{i}"])


def test_window_view_errors():
    from cplxmodule_amd.utils import window_view
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="positive"):
        window_view(x, 1, 0, 1)
    with pytest.raises(ValueError, match="nonnegative"):
        window_view(x, 1, 2, -1)
    with pytest.raises(ValueError, match="too short"):
        window_view(x, 1, 9, 1)
    with pytest.raises(ValueError, match="out of range"):
        window_view(x, 2, 2, 1)
    with pytest.raises(ValueError, match="out of range"):
        window_view(x, 1, 2, 1, at=3)


def test_fftshift(golden):
    sp = _sp()
    d = golden("spectrum")
    np.testing.assert_array_equal(sp.fftshift(torch.from_numpy(d["pw_density"]), dim=-1).numpy(), d["fftshift"])
    np.testing.assert_array_equal(sp.fftshift(torch.arange(35.0).reshape(5, 7), dim=0).numpy(), d["fftshift_odd"])
    for n in (1, 2, 7, 8):
        a = np.arange(3 * n, dtype=np.float64).reshape(3, n)
        np.testing.assert_array_equal(sp.fftshift(torch.from_numpy(a)).numpy(), np.fft.fftshift(a, axes=-1))
    from cplxmodule_amd import Cplx
    z = sp.fftshift(Cplx(torch.arange(5.0), -torch.arange(5.0)), dim=0)
    np.testing.assert_array_equal(z.real.numpy(), np.fft.fftshift(np.arange(5.0)))
    np.testing.assert_array_equal(z.imag.numpy(), -np.fft.fftshift(np.arange(5.0)))


def _nonzero_ranges(n, fs, bands, dtype):
    """the reference's selection: torch.nonzero(ff.gt(lo) & ff.lt(hi)) on fftshift(fftfreq) in `dtype`"""
    ff = torch.roll(torch.tensor(np.fft.fftfreq(n, 1.0 / fs), dtype=dtype), n // 2)
    out = []
    for lo, hi in bands:
        (idx,) = torch.nonzero(ff.gt(lo) & ff.lt(hi), as_tuple=True)
        out.append(idx.tolist())
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_band_bins_equal_the_nonzero_selection(golden, dtype):
    sp = _sp()
    d = golden("spectrum")
    cases = [(500, 1000.0, [tuple(b) for b in d["bands"].tolist()]), (4999, 1000.0, [(90.0, 110.0), (50.0, 70.0)])]
    rs = np.random.RandomState(3)
    for n in (1, 2, 7, 64, 1000, 4999):
        fs = float(rs.choice([1.0, 1000.0, 3.0e6, 7.0]))
        k = rs.randint(-n, n + 1, size=8) / n * fs / 2
        edges = [(float(a), float(b)) for a, b in zip(k[:4], k[4:])]                     # exact bin edges included
        edges += [(float(a) + 1e-9 * fs, float(b)) for a, b in zip(k[:4], k[4:])]
        edges += [(float(np.float32(a)), float(np.nextafter(np.float32(b), np.float32(0)))) for a, b in zip(k, k[::-1])]
        cases.append((n, fs, edges))
    for n, fs, bands in cases:
        want = _nonzero_ranges(n, fs, bands, dtype)
        got = sp._band_bins(n, fs, bands, dtype)
        assert [list(range(a, b)) for a, b in got] == want, (n, fs)


def test_band_powers_from_the_fixture_spectrum(golden):
    """host bins + narrow/sum/log10 on the reference's own (shifted) spectrum give its band powers"""
    sp = _sp()
    d = golden("spectrum")
    bands = [tuple(b) for b in d["bands"].tolist()]
    for form in ("cplx", "real"):
        px = torch.from_numpy(d[f"bp_{form}_px"])
        ch = torch.stack([px[..., a:b].sum(-1) for a, b in sp._band_bins(500, 1000.0, bands)], -1)
        np.testing.assert_allclose((10 * torch.log10(ch)).numpy(), d[f"bp_{form}"], rtol=1e-12)


EXPECTED = {1: ("direct", "direct"), 2: ("direct", "direct"), 500: ("bluestein", "bluestein"),
            1024: ("direct", "direct"), 4999: ("bluestein+four-step", "bluestein+four-step"),
            8192: ("direct", "direct"), 16384: ("direct", "four-step"),
            16385: ("bluestein+four-step", "bluestein+four-step"), 65536: ("four-step", "four-step"),
            1 << 22: ("four-step", "four-step")}


@pytest.mark.parametrize("n", sorted(EXPECTED))
def test_plan_paths_and_workspace(n):
    from cplxmodule_amd import spectrum as hs
    rows, S = 3, 5
    for dtype, want in zip((torch.float32, torch.float64), EXPECTED[n]):
        path, ws_f, ws_b = hs.plan(n, rows, S, dtype)
        assert path == want, (n, dtype)
        esz = 4 if dtype == torch.float32 else 8
        assert ws_f >= rows * n * esz and ws_b >= rows * S * n * 2 * esz
        assert ws_f % 256 == 0 and ws_b % 256 == 0
    assert hs.plan(n, rows, S, torch.bfloat16) == hs.plan(n, rows, S, torch.float32)


def test_plan_rejects_past_2_22():
    from cplxmodule_amd import spectrum as hs
    from cplxmodule_amd._lib import CplxAmdError, load
    with pytest.raises(CplxAmdError, match="2\\^22"):
        hs.plan((1 << 22) + 1, 1, 1)
    with pytest.raises(CplxAmdError):
        hs.plan(0, 1, 1)
    lib = load()
    assert lib.cplxamd_welch_plan((1 << 22) + 1, 1, 1, 0, None, None) == -1
    assert lib.cplxamd_welch_plan(64, 1, 1, 2, None, None) == -1                   # F16 is not a Welch dtype


def test_entry_points_declared_bound_and_validated():
    from cplxmodule_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cplxamd.h")).read(), flags=re.S)
    lib = _lib.load()
    assert lib.cplxamd_abi_version() == 25
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", src) and name in _lib.SIGNATURES and hasattr(lib, name)
    # every argument is checked before any launch: callable without a GPU
    p = ctypes.c_void_p(16)
    assert lib.cplxamd_welch_fwd(None, None, 1, 1, 1, 8, None, 8, 1, 0, 1.0, None, None, 0, 0, None) == -1
    assert lib.cplxamd_welch_fwd(p, p, 8, 1, 1, 8, p, 8, 1, 0, 1.0, p, p, 0, 0, None) == -4      # workspace too small
    assert lib.cplxamd_welch_fwd(p, p, 8, 1, 1, 7, p, 8, 1, 0, 1.0, p, p, 1 << 20, 0, None) == -1  # t < n
    assert lib.cplxamd_welch_fwd(p, p, 8, 1, 1, 8, p, 8, 0, 0, 1.0, p, p, 1 << 20, 0, None) == -1  # step 0
    assert lib.cplxamd_welch_fwd(p, p, 8, 1, 1, 8, p, 8, 1, 2, 1.0, p, p, 1 << 20, 0, None) == -1  # scaling
    assert lib.cplxamd_welch_bwd(p, p, 8, 1, 1, 8, p, 8, 1, 0, 1.0, None, p, p, 8, 1, p, 1 << 20, 0, None) == -1


def test_reference_exception_types():
    sp = _sp()
    x = torch.zeros(2, 100, dtype=torch.complex64)
    w = torch.ones(16)
    with pytest.raises(ValueError, match="scaling"):
        sp.pwelch(x, 1, w, scaling="psd")
    with pytest.raises(AssertionError):
        sp.pwelch(torch.zeros(2, 100), 1, w)
    with pytest.raises(AssertionError):
        sp.pwelch(x, 1, w, n_overlap=16)
    with pytest.raises(ValueError, match="too short"):
        sp.pwelch(x, 1, torch.ones(101))
    with pytest.raises(ValueError, match="out of range"):
        sp.pwelch(x, 2, w)
    with pytest.raises(AssertionError):
        sp.bandwidth_power(torch.zeros(2, 100, 3), 1.0, [(0, 1)])
    with pytest.raises(TypeError, match="list or a tuple"):
        sp.acpr_calc(torch.zeros(2, 100, 2), 1.0, 0.1, 0.1, acf=0.2, acb=0.1)
    with pytest.raises(TypeError, match="list or a tuple"):
        sp.acpr_calc(torch.zeros(2, 100, 2), 1.0, 0.1, 0.1, acf=[0.2], acb="0.1")


def test_cpu_tensors_raise():
    from cplxmodule_amd import Cplx
    from cplxmodule_amd._lib import CplxAmdError
    sp = _sp()
    x = torch.randn(2, 100, dtype=torch.complex64)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        sp.pwelch(x, 1, torch.hamming_window(16))
    with pytest.raises(CplxAmdError, match="no CPU path"):
        sp.pwelch(Cplx(x.real, x.imag), 1, torch.hamming_window(16))
    with pytest.raises(CplxAmdError, match="no CPU path"):
        sp.bandwidth_power(torch.view_as_real(x), 1.0, [(-0.1, 0.1)], nperseg=32)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        sp.acpr_calc(torch.view_as_real(x), 1.0, 0.1, 0.1, acf=[0.3], acb=0.1)
