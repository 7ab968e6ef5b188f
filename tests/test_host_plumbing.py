"""The host plumbing between _lib and the autograd Functions, without a GPU: the per-stream scratch cache, the hints a
producer leaves on its output tensors, the dtype codes of the float64-capable planes."""
import pytest
import torch

from cplxmodule_amd import _lib, _runs, ops, spectrum

CPU = torch.device("cpu")


# ---- _lib.scratch ----------------------------------------------------------------------------------------------------
@pytest.fixture
def cache(monkeypatch):
    monkeypatch.setattr(_lib, "_scratch", {})


def test_scratch_grows_and_never_shrinks(cache):
    a = _lib.scratch("t", CPU, 1000)
    assert a.dtype == torch.uint8 and a.numel() == 1000
    assert _lib.scratch("t", CPU, 10) is a and _lib.scratch("t", CPU, 1000) is a
    b = _lib.scratch("t", CPU, 1001)
    assert b is not a and b.numel() == 1001
    assert _lib.scratch("t", CPU, 1000) is b


def test_scratch_floor(cache):
    floor = 1 << 16
    sizes = (0, 1, floor - 1, floor, floor + 1)
    for n in sizes:                                                # a first request: the floor, or what was asked
        assert _lib.scratch(f"first{n}", CPU, n, floor).numel() == max(n, floor)
    for n in sizes + sizes[::-1]:                                  # one tag, growing then not: never shorter than asked
        assert _lib.scratch("f", CPU, n, floor).numel() >= max(n, floor)
    for n in (0, 1, 63, 64, 65):                                   # no floor: exactly what the first request asked
        assert _lib.scratch(f"nofloor{n}", CPU, n).numel() == n


def test_scratch_tags_are_separate_buffers(cache):
    a, b = _lib.scratch("gemm", CPU, 256), _lib.scratch("gauss", CPU, 256)
    assert a is not b and a.data_ptr() != b.data_ptr()
    assert a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
    assert _lib.scratch("gemm", CPU, 256) is a and _lib.scratch("gauss", CPU, 256) is b


def test_scratch_is_per_stream(cache, monkeypatch):
    """One tag on two streams of one device: two buffers.  (No GPU here: the stream handle and the allocation of a
    "cuda" buffer are stood in for; the real thing is tests/test_gpu_linear.py.)"""
    stream = [0x1000]
    empty = torch.empty
    monkeypatch.setattr(_lib, "_current_stream_handle", lambda idx=None: stream[0])
    monkeypatch.setattr(torch, "empty", lambda n, dtype, device: empty(n, dtype=dtype))
    dev = torch.device("cuda", 0)
    a = _lib.scratch("t", dev, 128)
    stream[0] = 0x2000
    b = _lib.scratch("t", dev, 128)
    assert a is not b and a.data_ptr() != b.data_ptr()
    assert _lib.scratch("t", dev, 64) is b
    stream[0] = 0x1000
    assert _lib.scratch("t", dev, 64) is a
    assert _lib.scratch_key(dev) == ("cuda", 0, 0x1000)


# ---- the hints of ops.py ---------------------------------------------------------------------------------------------
NODE, OTHER_NODE = object(), object()
SHAPE = (2, 4, 3, 3)


def _colsum():
    sums = torch.zeros(SHAPE[1])
    return 1, (lambda t: ops.attach_colsum(t, sums)), ops.colsum_hint, (lambda got: got is sums)


def _scale():
    scale = torch.ones(2)
    return 2, (lambda tr, ti: ops.attach_scale(tr, ti, scale)), ops.scale_hint, (lambda got: got is scale)


def _wgrad():
    dw = (torch.zeros(4, 4), torch.ones(4, 4), NODE)
    return (2, (lambda tr, ti: ops.attach_wgrad(tr, ti, dw)), (lambda tr, ti: ops.wgrad_hint(tr, ti, NODE)),
            (lambda got: got is not None and len(got) == 2 and got[0] is dw[0] and got[1] is dw[1]))


def _moments():
    partials = torch.zeros(3 * SHAPE[1] * 5, dtype=torch.float64)
    return (2, (lambda tr, ti: ops.attach_moments(tr, ti, partials, 3)), ops.moments_hint,
            (lambda got: got is not None and len(got) == 2 and got[0] is partials and got[1] == 3))


KINDS = {"colsum": _colsum, "scale": _scale, "wgrad": _wgrad, "moments": _moments}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_hint_is_taken_back_only_from_the_same_unmodified_planes(kind):
    n, attach, hint, same = KINDS[kind]()
    fresh = lambda: tuple(torch.zeros(SHAPE) for _ in range(n))  # noqa: E731
    planes = fresh()
    assert hint(*planes) is None
    attach(*planes)
    assert same(hint(*planes)) and same(hint(*planes))                    # (taking it does not consume it)
    for k in range(n):                                                    # an in-place write to either plane
        planes = fresh()
        attach(*planes)
        planes[k].add_(1)
        assert hint(*planes) is None
        attach(*planes)                                                   # ... and left again after the write
        assert same(hint(*planes))
    planes = fresh()
    attach(*planes)
    assert hint(*(t.clone() for t in planes)) is None                     # equal values, other storage
    for k in range(n):
        assert hint(*(t.clone() if i == k else t for i, t in enumerate(planes))) is None
    assert hint(*(t.view(SHAPE[0] * SHAPE[1], 3, 3) for t in planes)) is None        # a reshaped view
    if n == 2:                                                            # planes of different shapes
        assert hint(planes[0], planes[1][:1]) is None
        assert hint(planes[0], planes[1].view(SHAPE[0] * SHAPE[1], 3, 3)) is None
        odd = (torch.zeros(SHAPE), torch.zeros(SHAPE)[:1])
        attach(*odd)
        assert hint(*odd) is None


def test_wgrad_hint_is_for_one_node():
    n, attach, hint, same = _wgrad()
    tr, ti = torch.zeros(SHAPE), torch.zeros(SHAPE)
    attach(tr, ti)
    assert ops.wgrad_hint(tr, ti, OTHER_NODE) is None and ops.wgrad_hint(tr, ti, None) is None
    assert same(ops.wgrad_hint(tr, ti, NODE))


def test_colsum_hint_wants_one_sum_per_channel():
    t = torch.zeros(SHAPE)
    ops.attach_colsum(t, torch.zeros(SHAPE[1] + 1))
    assert ops.colsum_hint(t) is None
    sums = torch.zeros(SHAPE[1])
    ops.attach_colsum(t, sums)
    assert ops.colsum_hint(t) is sums


def test_hints_of_different_kinds_do_not_meet():
    tr, ti = torch.zeros(SHAPE), torch.zeros(SHAPE)
    ops.attach_scale(tr, ti, torch.ones(2))
    assert ops.moments_hint(tr, ti) is None and ops.wgrad_hint(tr, ti, NODE) is None and ops.colsum_hint(tr) is None


# ---- the small copies ------------------------------------------------------------------------------------------------
def test_dtype_codes_and_their_messages():
    for fn in (_runs.code, spectrum._code):
        assert (fn(torch.float32), fn(torch.bfloat16), fn(torch.float64)) == (_lib.F32, _lib.BF16, _lib.F64)
    with pytest.raises(_lib.CplxAmdError) as e:
        _runs.code(torch.float16)
    assert str(e.value) == "fft: planes must be float32, bfloat16 or float64, got torch.float16"
    with pytest.raises(_lib.CplxAmdError) as e:
        spectrum._code(torch.int32)
    assert str(e.value) == ("Welch spectra take float32, bfloat16 or float64 planes (complex64 / complex128), got "
                            "torch.int32")


def test_al16_and_ntuple():
    assert _lib.al16(None) is None
    t = torch.zeros(64)
    while t.data_ptr() % 16:                                  # (torch aligns its allocations; be sure anyway)
        t = t[1:]
    assert _lib.al16(t) is t
    off = t[1:]
    moved = _lib.al16(off)
    assert moved is not off and moved.data_ptr() % 16 == 0 and torch.equal(moved, off)
    assert _lib.ntuple(3, 2) == (3, 3) and _lib.ntuple(1, 3) == (1, 1, 1)
    assert _lib.ntuple([1, 2], 2) == (1, 2) and _lib.ntuple((1, 2, 3), 3) == (1, 2, 3)
