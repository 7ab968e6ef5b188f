"""cplx.fft / ifft / fft2 / fftn without a GPU: the plan of csrc/fft.hip as a pure function, the argument handling of
cplxmodule_amd/fft.py, the shifts on CPU planes, and the C entry point's validation before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import fft_cases as fc
from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd._lib import CplxAmdError

EINVAL = -1


# ---- cplxamd_fft_plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(fc.PLAN_PATHS))
def test_plan_paths(n):
    for dtype, want in zip((torch.float32, torch.float64), fc.PLAN_PATHS[n]):
        path, vpw, ws = hostfft.plan(n, 3, dtype)
        assert path == want, (n, dtype, path)
        assert vpw == fc.vectors_per_workgroup(n), (n, vpw)
        assert ws > 0 and ws % 256 == 0
    # bf16 planes are computed in float32: the same plan
    assert hostfft.plan(n, 3, torch.bfloat16) == hostfft.plan(n, 3, torch.float32)


def test_plan_vectors_per_workgroup_is_2048_over_m():
    for n, m in ((8, 8), (64, 64), (100, 256), (512, 512), (513, 2048), (1024, 1024), (5, 16), (3, 8)):
        assert fc.transform_size(n) == m
        assert hostfft.plan(n, 1)[1] == (2048 // m if m <= 1024 else 1)
    for n in (1, 2, 4):                                   # below 8 points a thread holds a whole vector: 256 per workgroup
        assert hostfft.plan(n, 1)[1] == 256


def test_plan_workspace_grows_with_the_batch_only_through_the_workspace_paths():
    assert hostfft.plan(1024, 1)[2] == hostfft.plan(1024, 10 ** 6)[2]
    assert hostfft.plan(1 << 16, 1)[2] < hostfft.plan(1 << 16, 64)[2]
    assert hostfft.plan(1 << 16, 10 ** 6)[2] <= (1 << 16) * 8 + 2 * (256 << 20) + 1024      # batches bounded as Welch's


def test_plan_rejects_bad_arguments():
    lib = _lib.load()
    vpw, ws = ctypes.c_int(0), ctypes.c_int64(0)
    for n, dtype in ((0, _lib.F32), ((1 << 22) + 1, _lib.F32), (64, _lib.F16), (64, 17), (-5, _lib.F64)):
        assert lib.cplxamd_fft_plan(n, 1, dtype, ctypes.byref(vpw), ctypes.byref(ws)) == EINVAL
    assert lib.cplxamd_fft_plan(64, -1, _lib.F32, None, None) == EINVAL
    assert lib.cplxamd_fft_plan(64, 1, _lib.F32, None, None) == 0         # nullable outputs
    with pytest.raises(CplxAmdError):
        hostfft.plan((1 << 22) + 1, 1)


# ---- the C entry point checks before it launches ---------------------------------------------------------------------
def test_no_gpu_arguments_are_rejected_not_crashed():
    lib = _lib.load()
    d = _lib.FftDesc(n=64, n_in=64, x_es=1, y_es=1, runs=1, inverse=0, scale=1.0)
    d.size[0], d.x_stride[0], d.y_stride[0] = 4, 64, 64
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    assert lib.cplxamd_fft(None, None, None, None, None, _lib.F32, _lib.F32, None, 0, None) == EINVAL
    assert lib.cplxamd_fft(p, p, p, p, None, _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(d), _lib.F32, _lib.F32, None, big, None) == EINVAL
    for pair in ((_lib.F32, _lib.F64), (_lib.F64, _lib.F32), (_lib.BF16, _lib.F64), (_lib.F16, _lib.F16), (_lib.F32, 9)):
        assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(d), pair[0], pair[1], p, big, None) == EINVAL
    for field, value in (("n", 0), ("n", (1 << 22) + 1), ("n_in", 0), ("n_in", 65), ("x_es", -1), ("y_es", 0), ("runs", 4),
                         ("runs", -1), ("inverse", 4), ("scale", float("nan")), ("scale", float("inf"))):
        bad = _lib.FftDesc.from_buffer_copy(d)
        setattr(bad, field, value)
        assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(bad), _lib.F32, _lib.F32, p, big, None) == EINVAL, field
    bad = _lib.FftDesc.from_buffer_copy(d)
    bad.size[0] = -1
    assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(bad), _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(d), _lib.F32, _lib.F32, p, 16, None) == -4          # workspace too small
    empty = _lib.FftDesc.from_buffer_copy(d)
    empty.size[0] = 0
    assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(empty), _lib.F32, _lib.F32, p, big, None) == 0      # no launch
    assert ctypes.sizeof(_lib.FftDesc) == 120


# ---- argument handling -----------------------------------------------------------------------------------------------
def _z(*shape, dtype=torch.float32):
    return Cplx(torch.zeros(*shape, dtype=dtype), torch.zeros(*shape, dtype=dtype))


@pytest.mark.parametrize("name, kwargs", [
    ("fft", dict(n=0)),
    ("ifft", dict(n=-3)),
    ("fft2", dict(s=(4, 0))),
    ("fft", dict(norm="both")),
    ("ifftn", dict(norm="orthonormal")),
    ("fft2", dict(dim=(-1, -1))),
    ("fftn", dict(dim=(0, 2, -1))),
    ("fftn", dict(s=(4, 4), dim=(0,))),
    ("fft2", dict(s=(4,))),
])
def test_argument_errors_are_torchs(name, kwargs):
    """n or an entry of s below 1, an unknown norm, repeated dims, s and dim of different lengths: RuntimeError, raised
    before the device is looked at -- and NOT the package's own error class"""
    with pytest.raises(RuntimeError) as e:
        getattr(cplx, name)(_z(2, 3, 4), **kwargs)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError):                     # torch raises on every one of them too
        getattr(torch.fft, name)(torch.zeros(2, 3, 4, dtype=torch.complex64), **kwargs)


def test_there_is_no_host_path():
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.fft(_z(4, 8))
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.fft(_z(4, 8, dtype=torch.float16))
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.fft2(Cplx(torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float64)))
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.fft(torch.zeros(4, 8))
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.ifftn(torch.zeros(4, 8, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.fft(_z(2, 8), n=(1 << 22) + 1)


def test_argument_rules_follow_torch():
    z = _z(5, 6, 7)
    assert hostfft._arguments(z, None, [-1], None, "fft") == [(2, 7)]
    assert hostfft._arguments(z, [9], [1], "ortho", "fft") == [(1, 9)]
    assert hostfft._arguments(z, None, (-2, -1), None, "fft2") == [(1, 6), (2, 7)]
    assert hostfft._arguments(z, None, None, None, "fftn") == [(0, 5), (1, 6), (2, 7)]
    assert hostfft._arguments(z, (3, 4), None, None, "fftn") == [(1, 3), (2, 4)]
    assert hostfft._arguments(z, (3, -1), (2, 0), "forward", "fftn") == [(2, 3), (0, 5)]
    for n, norm, inverse, want in ((8, None, False, 1.0), (8, "backward", True, 0.125), (8, "forward", False, 0.125),
                                   (8, "forward", True, 1.0), (16, "ortho", False, 0.25), (16, "ortho", True, 0.25)):
        assert hostfft._scale(n, norm, inverse) == want


def test_batch_runs_fuse_jointly():
    """contiguous, channels-last and transposed layouts need at most three runs; the innermost run has the smallest stride"""
    x = torch.empty(3, 4, 5, 6)
    for t in (x, x.contiguous(memory_format=torch.channels_last), x.permute(0, 2, 1, 3), x[:, :, ::2], x[:, :1].expand(3, 4, 5, 6)):
        for dim in range(4):
            shape, ys = hostfft._dense_like(t, dim, t.shape[dim])
            runs = hostfft._runs(shape, t.stride(), ys, dim)
            assert len(runs) <= 3
            assert np.prod([r[0] for r in runs]) == t.numel() // t.shape[dim]
            assert [r[2] for r in runs] == sorted((r[2] for r in runs), reverse=True)
    shape, ys = hostfft._dense_like(x, 3, 6)
    assert hostfft._runs(shape, x.stride(), ys, 3) == [[60, 6, 6]]
    cl = x.contiguous(memory_format=torch.channels_last)
    shape, ys = hostfft._dense_like(cl, 3, 6)
    assert tuple(ys) == cl.stride()
    assert hostfft._runs(shape, cl.stride(), ys, 3) == [[15, 24, 24], [4, 1, 1]]


@pytest.mark.parametrize("shape, dim", [((7,), None), ((4, 5), None), ((4, 5), 0), ((3, 4, 6), (0, 2)), ((2, 9), -1)])
def test_shifts_on_cpu_planes_equal_numpys(shape, dim):
    rs = np.random.RandomState(0)
    re, im = rs.randn(*shape).astype(np.float32), rs.randn(*shape).astype(np.float32)
    z = Cplx(torch.from_numpy(re), torch.from_numpy(im))
    for ours, theirs in ((cplx.fftshift, np.fft.fftshift), (cplx.ifftshift, np.fft.ifftshift)):
        got = ours(z, dim=dim)
        np.testing.assert_array_equal(got.real.numpy(), theirs(re, axes=dim))
        np.testing.assert_array_equal(got.imag.numpy(), theirs(im, axes=dim))
    back = cplx.ifftshift(cplx.fftshift(z, dim=dim), dim=dim)
    assert torch.equal(back.real, z.real) and torch.equal(back.imag, z.imag)
