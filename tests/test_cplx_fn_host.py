"""cplx's elementary functions and joining helpers without a GPU: the names exist, the joining helpers match numpy on CPU
`Cplx` (with the reference's error cases, its tests/test_cplx.py:630-657), the two new C entry points are declared, bound
and exported under ABI 25 and reject bad arguments before any launch, and the functions refuse CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")
JOINING = ("cat", "split", "chunk", "stack", "unbind", "take", "narrow", "squeeze", "unsqueeze")
NEW_EXPORTS = ("cplxamd_cplx_fn_fwd", "cplxamd_cplx_fn_bwd")


def _close(z, a):
    np.testing.assert_allclose(z.real.numpy() + 1j * z.imag.numpy(), a, rtol=1e-12, atol=0)


@pytest.fixture
def rs():
    return np.random.RandomState(0)


def test_the_17_names_exist():
    from cplxmodule_amd import cplx
    for name in FUNCTIONS + JOINING:
        assert callable(getattr(cplx, name)), name


def test_cat_stack_match_numpy(rs):
    from cplxmodule_amd import cplx
    with pytest.raises(RuntimeError, match="a non-empty"):
        cplx.stack([], dim=0)
    arrays = [rs.randn(5, 3, 7) + 1j * rs.randn(5, 3, 7) for _ in range(4)]
    tensors = [cplx.Cplx.from_numpy(a) for a in arrays]
    for n in (0, 1, 2, -1):
        _close(cplx.cat(tensors, dim=n), np.concatenate(arrays, axis=n))
    for n in (0, 1, 2, 3):
        _close(cplx.stack(tensors, dim=n), np.stack(arrays, axis=n))
    _close(cplx.cat(map(cplx.Cplx.from_numpy, arrays), dim=1), np.concatenate(arrays, axis=1))   # any iterable
    _close(cplx.stack(iter(tensors), dim=0), np.stack(arrays))
    mismatched = [rs.randn(3, 7) + 1j * rs.randn(3, 7), rs.randn(5, 7) + 1j * rs.randn(5, 7)]
    for n in (0, 1, 2):
        with pytest.raises(RuntimeError, match="each tensor to be equal size"):
            cplx.stack(map(cplx.Cplx.from_numpy, mismatched), dim=n)
    with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
        cplx.cat(map(cplx.Cplx.from_numpy, mismatched), dim=1)


def test_split_chunk_unbind_match_numpy(rs):
    from cplxmodule_amd import cplx
    a = rs.randn(6, 4, 5) + 1j * rs.randn(6, 4, 5)
    p = cplx.Cplx.from_numpy(a)
    parts = cplx.split(p, 2, dim=0)
    assert isinstance(parts, tuple) and len(parts) == 3
    for got, ref in zip(parts, np.split(a, 3, axis=0)):
        _close(got, ref)
    parts = cplx.split(p, [1, 4], dim=2)
    for got, ref in zip(parts, (a[..., :1], a[..., 1:])):
        _close(got, ref)
    parts = cplx.chunk(p, 2, dim=1)
    assert len(parts) == 2
    for got, ref in zip(parts, np.array_split(a, 2, axis=1)):
        _close(got, ref)
    parts = cplx.unbind(p, dim=1)
    assert len(parts) == 4
    for k, got in enumerate(parts):
        _close(got, a[:, k])
    assert len(cplx.unbind(p)) == 6


def test_take_narrow_squeeze_unsqueeze_match_numpy(rs):
    from cplxmodule_amd import cplx
    a = rs.randn(3, 1, 5) + 1j * rs.randn(3, 1, 5)
    p = cplx.Cplx.from_numpy(a)
    idx = np.array([0, 4, 14, 7])
    _close(cplx.take(p, torch.from_numpy(idx)), np.take(a, idx))
    _close(cplx.narrow(p, 2, 1, 3), a[:, :, 1:4])
    _close(cplx.squeeze(p), a.squeeze())
    _close(cplx.squeeze(p, 1), a.squeeze(1))
    _close(cplx.squeeze(p, 0), a)
    _close(cplx.unsqueeze(p, 0), a[None])
    _close(cplx.unsqueeze(p, -1), a[..., None])
    with pytest.raises(RuntimeError):
        cplx.narrow(p, 2, 3, 5)


def test_new_exports_are_declared_bound_and_exported_under_abi_25():
    from cplxmodule_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cplxamd.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert "#define CPLXAMD_ABI_VERSION 25" in src and _lib.ABI_VERSION == 25
    enum = re.search(r"enum\s*\{\s*CPLXAMD_FN_EXP[^}]*\}", src).group(0)
    assert re.findall(r"CPLXAMD_FN_([A-Z]+)", enum) == [f.upper() for f in FUNCTIONS]
    assert [_lib.CPLX_FN[f] for f in FUNCTIONS] == list(range(8))
    lib = ctypes.CDLL(os.path.join(ROOT, "cplxmodule_amd", "libcplxamd.so"))
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert _lib.load().cplxamd_abi_version() == 25


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from cplxmodule_amd import _lib
    lib = _lib.load()
    fwd = lambda z, n, fn, dt: lib.cplxamd_cplx_fn_fwd(z, z, z, z, n, fn, dt, None)  # noqa: E731
    bwd = lambda z, n, fn, dt: lib.cplxamd_cplx_fn_bwd(z, z, z, z, z, z, n, fn, dt, None)  # noqa: E731
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: every case below is refused before a launch
    for call in (fwd, bwd):
        assert call(None, 16, 0, _lib.F32) == -1            # NULL with n > 0
        assert call(fake, -1, 0, _lib.F32) == -1            # n < 0
        assert call(fake, 16, 8, _lib.F32) == -1            # unknown function
        assert call(fake, 16, -1, _lib.BF16) == -1
        assert call(fake, 16, 7, _lib.F16) == -1            # dtype other than F32 / BF16
        assert call(fake, 16, 7, 3) == -1
        assert call(None, 0, 7, _lib.BF16) == 0             # nothing to do
    assert lib.cplxamd_cplx_fn_bwd(fake, fake, None, fake, fake, fake, 4, 0, _lib.F32, None) == -1


def test_functions_refuse_cpu_and_unsupported_tensors():
    from cplxmodule_amd import cplx
    from cplxmodule_amd._lib import CplxAmdError
    z = cplx.Cplx(torch.randn(4, 3), torch.randn(4, 3))
    for name in FUNCTIONS:
        with pytest.raises(CplxAmdError):
            getattr(cplx, name)(z)
    with pytest.raises(CplxAmdError):
        cplx.exp(z.to(torch.float64))          # float64 goes to f64.py, which runs on the device only
