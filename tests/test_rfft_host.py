"""cplx.rfft / irfft / rfft2 / rfftn / hfft / ihfft without a GPU: the plan of csrc/rfft.hip as a pure function (the
half-length route shows in it), the C entry point's validation before any launch, the argument handling and the output
shapes of cplxmodule_amd/rfft.py."""
import ctypes

import pytest
import torch

import fft_cases as fc
import rfft_cases as rc
from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd import rfft as hostrfft
from cplxmodule_amd._lib import CplxAmdError

EINVAL, EWS = -1, -4
C2R, WEIGHTED = 4, 8


# ---- cplxamd_rfft_plan -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(rc.PLAN))
def test_plan_runs_the_half_length_transform(n):
    p32, p64, cn, points = rc.PLAN[n]
    assert cn == rc.complex_length(n) and points == fc.transform_size(cn)
    for c2r in (False, True):
        for dtype, want in ((torch.float32, p32), (torch.float64, p64)):
            path, got_cn, got_points, vpw, ws = hostrfft.plan(n, 3, dtype, c2r)
            assert (path, got_cn, got_points) == (want, cn, points), (n, dtype, path, got_cn, got_points)
            assert vpw == fc.vectors_per_workgroup(cn), (n, vpw)
            assert ws > 0 and ws % 256 == 0
            # the complex transform's own workspace, plus the table e^{-2 pi i k/n}, k < n / 2, for an even n
            base = hostfft.plan(cn, 3, dtype)[2]
            assert ws > base if n % 2 == 0 else ws == base
        assert hostrfft.plan(n, 3, torch.bfloat16, c2r) == hostrfft.plan(n, 3, torch.float32, c2r)


def test_plan_packs_twice_the_vectors():
    for n in (2, 64, 2048):
        assert hostrfft.plan(n, 1)[0] == "direct" and hostrfft.plan(n, 1)[1] == n // 2
    assert hostrfft.plan(2048, 1)[3] == 2 and hostfft.plan(2048, 1)[1] == 1
    assert hostrfft.plan(64, 1)[3] == 64 and hostfft.plan(64, 1)[1] == 32
    assert hostrfft.plan(4096, 1)[3] == 1
    assert hostrfft.plan(200, 1)[3] == 8 and hostfft.plan(200, 1)[1] == 4       # Bluestein on 256, not 512, points
    # packed Bluestein reaches n = 1024 (n = 1000 runs 500 points on 1024) and ends there
    assert hostrfft.plan(1000, 1)[2:4] == (1024, 2) and hostrfft.plan(1026, 1)[2:4] == (2048, 1)


def test_plan_rejects_bad_arguments():
    lib = _lib.load()
    out = [ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)]
    refs = [ctypes.byref(o) for o in out]
    for n, dtype, c2r in ((0, _lib.F32, 0), ((1 << 22) + 1, _lib.F32, 0), (64, _lib.F16, 0), (64, 17, 1), (-5, _lib.F64, 1),
                          (64, _lib.F32, 2)):
        assert lib.cplxamd_rfft_plan(n, 1, dtype, c2r, *refs) == EINVAL
    assert lib.cplxamd_rfft_plan(64, -1, _lib.F32, 0, None, None, None, None) == EINVAL
    assert lib.cplxamd_rfft_plan(64, 1, _lib.F32, 0, None, None, None, None) == 0      # nullable outputs
    assert lib.cplxamd_rfft_plan(1 << 22, 1, _lib.F32, 1, *refs) == 1                  # accepted: four-step
    with pytest.raises(CplxAmdError):
        hostrfft.plan((1 << 22) + 1, 1)


# ---- the C entry point checks before it launches ---------------------------------------------------------------------
@pytest.mark.parametrize("direction", [0, C2R], ids=["r2c", "c2r"])
def test_no_gpu_arguments_are_rejected_not_crashed(direction):
    lib = _lib.load()
    n_in = 33 if direction else 64
    d = _lib.FftDesc(n=64, n_in=n_in, x_es=1, y_es=1, runs=1, inverse=direction, scale=1.0)
    d.size[0], d.x_stride[0], d.y_stride[0] = 4, 64, 64
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    ref = ctypes.byref(d)
    assert lib.cplxamd_rfft(None, None, None, None, None, _lib.F32, _lib.F32, None, 0, None) == EINVAL
    assert lib.cplxamd_rfft(None, p, p, p, ref, _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_rfft(p, p, None, p, ref, _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_rfft(p, p, p, p, None, _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_rfft(p, p, p, p, ref, _lib.F32, _lib.F32, None, big, None) == EINVAL
    # the plane a direction does not touch may be NULL, the one it does may not
    if direction:
        assert lib.cplxamd_rfft(p, None, p, p, ref, _lib.F32, _lib.F32, p, big, None) == EINVAL
        assert lib.cplxamd_rfft(p, p, p, None, ref, _lib.F32, _lib.F32, p, 16, None) == EWS
    else:
        assert lib.cplxamd_rfft(p, p, p, None, ref, _lib.F32, _lib.F32, p, big, None) == EINVAL
        assert lib.cplxamd_rfft(p, None, p, p, ref, _lib.F32, _lib.F32, p, 16, None) == EWS
    for pair in ((_lib.F32, _lib.F64), (_lib.F64, _lib.F32), (_lib.BF16, _lib.F64), (_lib.F64, _lib.BF16),
                 (_lib.F16, _lib.F16), (_lib.F16, _lib.F32), (_lib.F32, _lib.F16), (_lib.F32, 9), (-1, _lib.F32)):
        assert lib.cplxamd_rfft(p, p, p, p, ref, pair[0], pair[1], p, big, None) == EINVAL
    for field, value in (("n", 0), ("n", (1 << 22) + 1), ("n_in", 0), ("n_in", n_in + 1), ("x_es", -1), ("y_es", 0),
                         ("runs", 4), ("runs", -1), ("inverse", direction | 2), ("inverse", direction | 16),
                         ("inverse", direction | 32), ("scale", float("nan")), ("scale", float("inf"))):
        bad = _lib.FftDesc.from_buffer_copy(d)
        setattr(bad, field, value)
        assert lib.cplxamd_rfft(p, p, p, p, ctypes.byref(bad), _lib.F32, _lib.F32, p, big, None) == EINVAL, field
    bad = _lib.FftDesc.from_buffer_copy(d)
    bad.size[0] = -1
    assert lib.cplxamd_rfft(p, p, p, p, ctypes.byref(bad), _lib.F32, _lib.F32, p, big, None) == EINVAL
    assert lib.cplxamd_rfft(p, p, p, p, ref, _lib.F32, _lib.F32, p, 16, None) == EWS            # workspace too small
    for flags in (direction, direction | 1, direction | WEIGHTED, direction | 1 | WEIGHTED):
        empty = _lib.FftDesc.from_buffer_copy(d)
        empty.size[0], empty.inverse = 0, flags
        assert lib.cplxamd_rfft(p, p, p, p, ctypes.byref(empty), _lib.F32, _lib.F32, p, big, None) == 0    # no launch


def test_the_complex_entry_point_still_rejects_the_new_bits():
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bits in (4, 8, 5, 12):
        d = _lib.FftDesc(n=64, n_in=64, x_es=1, y_es=1, runs=1, inverse=bits, scale=1.0)
        d.size[0], d.x_stride[0], d.y_stride[0] = 4, 64, 64
        assert lib.cplxamd_fft(p, p, p, p, ctypes.byref(d), _lib.F32, _lib.F32, p, 1 << 30, None) == EINVAL


# ---- argument handling -----------------------------------------------------------------------------------------------
def _z(*shape, dtype=torch.float32):
    return Cplx(torch.zeros(*shape, dtype=dtype), torch.zeros(*shape, dtype=dtype))


def _input(name, *shape, dtype=torch.float32):
    """what cplx.<name> takes, and what torch.fft.<name> takes"""
    if name.startswith(("irfft", "hfft")):
        return _z(*shape, dtype=dtype), torch.zeros(*shape, dtype=torch.complex64)
    return torch.zeros(*shape, dtype=dtype), torch.zeros(*shape)


@pytest.mark.parametrize("name, kwargs, error", [
    ("rfft", dict(n=0), RuntimeError),
    ("rfft", dict(norm="both"), RuntimeError),
    ("rfft", dict(dim=3), IndexError),
    ("irfft", dict(n=0), RuntimeError),
    ("irfft", dict(n=-3), RuntimeError),
    ("irfft", dict(norm="orthonormal"), RuntimeError),
    ("irfft", dict(dim=-4), IndexError),
    ("rfft2", dict(s=(4, 0)), RuntimeError),
    ("rfft2", dict(dim=(-1, -1)), RuntimeError),
    ("rfft2", dict(norm="no"), RuntimeError),
    ("irfft2", dict(s=(4,)), RuntimeError),
    ("irfft2", dict(dim=(0, 0)), RuntimeError),
    ("irfft2", dict(dim=(0, 7)), IndexError),
    ("rfftn", dict(dim=(0, 2, -1)), RuntimeError),
    ("rfftn", dict(s=(4, 4, 4, 4)), RuntimeError),
    ("irfftn", dict(s=(4, 4), dim=(0,)), RuntimeError),
    ("irfftn", dict(s=(4, 0)), RuntimeError),
    ("hfft", dict(n=-3), RuntimeError),
    ("hfft", dict(norm="both"), RuntimeError),
    ("hfft", dict(dim=5), IndexError),
    ("ihfft", dict(n=0), RuntimeError),
    ("ihfft", dict(norm="both"), RuntimeError),
    ("ihfft", dict(dim=-5), IndexError),
])
def test_argument_errors_are_torchs(name, kwargs, error):
    """raised on CPU inputs, so before the device is looked at -- and NOT the package's own error class"""
    ours, theirs = _input(name, 2, 3, 4)
    with pytest.raises(error) as e:
        getattr(cplx, name)(ours, **kwargs)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(error):                            # torch raises the same type on every one of them
        getattr(torch.fft, name)(theirs, **kwargs)


@pytest.mark.parametrize("name", ["irfft", "irfft2", "irfftn", "hfft"])
def test_a_default_output_length_of_zero_is_torchs_error(name):
    ours, theirs = _input(name, 2, 3, 1)
    with pytest.raises(RuntimeError) as e:
        getattr(cplx, name)(ours)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError):
        getattr(torch.fft, name)(theirs)


def test_there_is_no_host_path():
    for name in ("rfft", "rfft2", "rfftn", "ihfft"):
        fn = getattr(cplx, name)
        with pytest.raises(CplxAmdError, match="no CPU path"):
            fn(torch.zeros(4, 8))
        with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
            fn(torch.zeros(4, 8, dtype=torch.float16))
        with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
            fn(_z(4, 8))
        with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
            fn(torch.zeros(4, 8, dtype=torch.complex64))
    for name in ("irfft", "irfft2", "irfftn", "hfft"):
        fn = getattr(cplx, name)
        with pytest.raises(CplxAmdError, match="no CPU path"):
            fn(_z(4, 8))
        with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
            fn(_z(4, 8, dtype=torch.float16))
        with pytest.raises(CplxAmdError, match="not a Cplx"):
            fn(torch.zeros(4, 8))
        with pytest.raises(CplxAmdError, match="not a Cplx"):
            fn(torch.zeros(4, 8, dtype=torch.complex64))
        with pytest.raises(CplxAmdError, match="different dtypes"):
            fn(Cplx(torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float64)))
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.rfft(torch.zeros(2, 8), n=(1 << 22) + 1)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.ihfft(torch.zeros(2, 8), n=(1 << 22) + 1)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.irfft(_z(2, 8), n=(1 << 22) + 2)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.hfft(_z(2, 8), n=(1 << 22) + 1)


SHAPE_CASES = [
    ("rfft", (5, 6, 7), dict()), ("rfft", (5, 6, 8), dict()), ("rfft", (5, 6, 7), dict(n=10)), ("rfft", (5, 6, 7), dict(n=4, dim=1)),
    ("ihfft", (5, 6, 7), dict()), ("ihfft", (5, 6, 7), dict(n=9, dim=0)),
    ("irfft", (5, 6, 7), dict()), ("irfft", (5, 6, 7), dict(n=9)), ("irfft", (5, 6, 7), dict(n=20, dim=1)),
    ("hfft", (5, 6, 7), dict()), ("hfft", (5, 6, 2), dict(n=3)),
    ("rfft2", (5, 6, 7), dict()), ("rfft2", (5, 6, 7), dict(s=(4, 9))), ("rfft2", (5, 6, 7), dict(dim=(2, 0))),
    ("irfft2", (5, 6, 7), dict()), ("irfft2", (5, 6, 7), dict(s=(4, 9))), ("irfft2", (5, 6, 7), dict(dim=(2, 0))),
    ("rfftn", (5, 6, 7), dict()), ("rfftn", (5, 6, 7), dict(s=(3, 8))), ("rfftn", (5, 6, 7), dict(dim=(0, 1))),
    ("rfftn", (5, 6, 7), dict(s=(9, 3), dim=(2, 1))),
    ("irfftn", (5, 6, 7), dict()), ("irfftn", (5, 6, 7), dict(s=(4, 5, 6))), ("irfftn", (5, 6, 7), dict(s=(3, 9))),
    ("irfftn", (5, 6, 7), dict(dim=(0, 2))), ("irfftn", (5, 6, 7), dict(dim=(2, 0))), ("irfftn", (5, 6, 7), dict(s=(8, 3), dim=(2, 1))),
]


@pytest.mark.parametrize("name, shape, kwargs", SHAPE_CASES)
def test_output_shapes_are_torchs(name, shape, kwargs):
    """shape logic only: no transform runs"""
    theirs = _input(name, *shape)[1]
    s = kwargs.get("s", None if "n" not in kwargs else [kwargs["n"]])
    assert hostrfft.output_shape(name, shape, s, kwargs.get("dim")) == tuple(getattr(torch.fft, name)(theirs, **kwargs).shape)


def test_argument_rules_and_scales():
    x = torch.zeros(5, 6, 8)
    assert hostrfft.arguments(x, None, [-1], None, "rfft", False) == [(2, 8)]
    assert hostrfft.arguments(x, None, [-1], None, "irfft", True) == [(2, 14)]
    assert hostrfft.arguments(x, [9], [1], "ortho", "irfft", True) == [(1, 9)]
    assert hostrfft.arguments(x, None, (-2, -1), None, "irfft2", True) == [(1, 6), (2, 14)]
    assert hostrfft.arguments(x, (3, 4), None, None, "irfftn", True) == [(1, 3), (2, 4)]
    assert hostrfft.arguments(x, None, (2, 0), None, "irfftn", True) == [(2, 8), (0, 8)]
