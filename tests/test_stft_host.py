"""cplx.stft / istft without a GPU: the plan of csrc/stft.hip as a pure function, the kernels' index maps proved against
F.pad + unfold address by address, the C entry points' validation before any launch, the argument handling and the output
shapes of cplxmodule_amd/stft.py -- and every case of stft_cases.py through torch on the CPU, so that a bad case fails
here."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import fft_cases as fc
import stft_cases as sc
from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd import rfft as hostrfft
from cplxmodule_amd import stft as hoststft
from cplxmodule_amd._lib import CplxAmdError

EINVAL, ESHAPE, EWS = -1, -3, -4
ZERO, REFLECT = hoststft.PAD_ZERO, hoststft.PAD_REFLECT


# ---- cplxamd_stft_plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", sc.PLAN_LENGTHS)
def test_plan_is_the_real_transforms_plan_over_the_frames(n_fft):
    hop, T, rows = sc.path_geometry(n_fft)
    padded = T + 2 * (n_fft // 2)
    frames = torch.stft(torch.zeros(T, dtype=torch.float64), n_fft, hop, window=torch.ones(n_fft, dtype=torch.float64),
                        return_complex=True).shape[-1]
    for dtype, word in ((torch.float32, 4), (torch.float64, 8), (torch.bfloat16, 4)):
        p = hoststft.plan(n_fft, hop, padded, rows, T, dtype)
        path, cn, points, vpw, ws = hostrfft.plan(n_fft, rows * frames, dtype)
        assert (p["path"], p["complex_n"], p["points"], p["vectors_per_workgroup"]) == (path, cn, points, vpw)
        assert (p["path"], p["vectors_per_workgroup"]) == hostfft.plan(cn, rows * frames, dtype)[:2]
        assert p["frames"] == frames
        assert p["analysis_ws"] == ws and ws > 0 and ws % 256 == 0
        assert p["synthesis_ws"] > 0 and p["synthesis_ws"] % 256 == 0
        assert 1 <= p["rows_per_chunk"] <= rows
        assert p["synthesis_ws"] >= hostrfft.plan(n_fft, p["rows_per_chunk"] * frames, dtype, True)[4] + T * word + \
            p["rows_per_chunk"] * frames * n_fft * word
        # the full spectrum: the complex transform of n_fft points, and two planes of frames
        f = hoststft.plan(n_fft, hop, padded, rows, T, dtype, full=True)
        path, vpw, ws = hostfft.plan(n_fft, rows * frames, dtype)[:3]
        assert (f["path"], f["vectors_per_workgroup"], f["analysis_ws"], f["complex_n"], f["frames"]) == (path, vpw, ws, n_fft, frames)
        assert f["points"] == (n_fft if n_fft & (n_fft - 1) == 0 else 1 << (2 * n_fft - 2).bit_length())
        assert f["synthesis_ws"] % 256 == 0 and 1 <= f["rows_per_chunk"] <= rows
        assert f["synthesis_ws"] >= hostfft.plan(n_fft, f["rows_per_chunk"] * frames, dtype)[2] + T * word + \
            2 * f["rows_per_chunk"] * frames * n_fft * word


def test_plan_chunks_rows_under_the_cap_and_rejects_bad_arguments():
    # 4096 frames of 1024 float32 words are 16 MiB a row: 16 rows fill the 256 MiB cap
    p = hoststft.plan(1024, 256, 1024 + 4095 * 256, 64, 1 << 20, torch.float32)
    assert p["frames"] == 4096 and p["rows_per_chunk"] == 16
    assert hoststft.plan(1024, 256, 1024 + 4095 * 256, 64, 1 << 20, torch.float64)["rows_per_chunk"] == 8
    assert hoststft.plan(1024, 256, 1024 + 4095 * 256, 64, 1 << 20, torch.float32, full=True)["rows_per_chunk"] == 8   # two planes
    # one row larger than the cap takes what it needs
    big = hoststft.plan(1 << 14, 1 << 10, (1 << 14) + ((1 << 16) - 1) * (1 << 10), 2, 1 << 26, torch.float32)
    assert big["rows_per_chunk"] == 1 and big["synthesis_ws"] > (1 << 16) * (1 << 14) * 4
    lib = _lib.load()
    nul = [None] * 7
    for args in ((0, 1, 16, 1, 16, _lib.F32), ((1 << 22) + 1, 1, 1 << 23, 1, 16, _lib.F32), (16, 0, 16, 1, 16, _lib.F32),
                 (16, 4, 15, 1, 16, _lib.F32), (16, 4, 16, -1, 16, _lib.F32), (16, 4, 16, 1, -1, _lib.F32),
                 (16, 4, 16, 1, 16, _lib.F16), (16, 4, 16, 1, 16, 9)):
        assert lib.cplxamd_stft_plan(*args, 0, *nul) == EINVAL and lib.cplxamd_stft_plan(*args, 1, *nul) == EINVAL, args
    assert lib.cplxamd_stft_plan(16, 4, 16, 1, 16, _lib.F32, 0, *nul) == 0               # nullable outputs
    with pytest.raises(CplxAmdError):
        hoststft.plan(0, 1, 16, 1, 16)


# ---- the index maps, exhaustively ------------------------------------------------------------------------------------------
# (center=False on 9 samples holds no frame of 16: torch rejects it, and so does cplx.stft)
MAPS = [(T, n, hop, mode) for T, n, hop in sc.MAP_CASES for mode in ("reflect", "constant", "none")
        if mode != "none" or T >= n]


@pytest.mark.parametrize("T, n_fft, hop, mode", MAPS)
def test_index_maps_are_pad_and_unfold(T, n_fft, hop, mode):
    pad = 0 if mode == "none" else n_fft // 2
    assert pad < T or mode != "reflect"
    # sample indices 1 .. T, so that constant padding (0) is told apart
    marks = torch.arange(1, T + 1, dtype=torch.float64)
    padded = F.pad(marks.view(1, 1, T), (pad, pad), mode="reflect" if mode == "reflect" else "constant").view(-1)
    want = padded.unfold(0, n_fft, hop).long() - 1                      # [frames, n_fft]; -1 is "zero"
    frames = want.shape[0]
    d = hoststft.descriptor(n_fft, hop, frames, T, pad, REFLECT if mode == "reflect" else ZERO)
    sources = {}
    for f in range(frames):
        for j in range(n_fft):
            i = hoststft.src_index(d, f, j)
            assert i == int(want[f, j]), (f, j, i)
            assert -1 <= i < T
            if i >= 0:
                sources.setdefault(i, []).append(f * hop + j)
    # the fold of t: exactly the padded positions that map to t (whether or not a frame covers them), ascending
    whole = {}
    for q in range(T + 2 * pad):
        i = int(padded[q]) - 1
        if i >= 0:
            whole.setdefault(i, []).append(q)
    for t in range(T):
        got = hoststft.fold_positions(d, t)
        assert got == whole[t], (t, got, whole[t])
        assert set(sources.get(t, [])) <= set(got)
        assert 1 <= len(got) <= 3
    # out of the descriptor: refused, not computed
    assert hoststft.src_index(d, frames, 0) == -2 and hoststft.src_index(d, 0, n_fft) == -2 and hoststft.src_index(d, -1, 0) == -2
    with pytest.raises(CplxAmdError):
        hoststft.fold_positions(d, T)


def test_a_reflect_pad_as_long_as_the_signal_is_refused_by_the_maps():
    d = hoststft.descriptor(16, 4, 3, 8, 8, REFLECT)
    assert hoststft.src_index(d, 0, 0) == -2
    with pytest.raises(CplxAmdError):
        hoststft.fold_positions(d, 0)


# ---- the C entry points check before they launch --------------------------------------------------------------------------
def _desc(p, **over):
    kw = dict(n_fft=64, hop=16, frames=5, length=64, pad=32, rows=4, sig_row_stride=64, sig_es=1, spec_row_stride=5 * 33,
              spec_frame_stride=33, spec_es=1, pad_mode=REFLECT, flags=0, window=p.value, envelope=None, scale=1.0)
    kw.update(over)
    return _lib.StftDesc(**kw)


@pytest.mark.parametrize("entry", ["cplxamd_stft", "cplxamd_istft"])
def test_no_gpu_arguments_are_rejected_not_crashed(entry):
    fn = getattr(_lib.load(), entry)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    ref = ctypes.byref(_desc(p))
    assert fn(None, None, None, None, _lib.F32, None, 0, None) == EINVAL
    assert fn(None, p, p, ref, _lib.F32, p, big, None) == EINVAL
    assert fn(p, None, p, ref, _lib.F32, p, big, None) == EINVAL
    assert fn(p, p, None, ref, _lib.F32, p, big, None) == EINVAL
    assert fn(p, p, p, None, _lib.F32, p, big, None) == EINVAL
    assert fn(p, p, p, ref, _lib.F32, None, big, None) == EINVAL
    for dtype in (_lib.F16, 9, -1):
        assert fn(p, p, p, ref, dtype, p, big, None) == EINVAL
    bad_fields = [("n_fft", 0), ("n_fft", (1 << 22) + 1), ("hop", 0), ("hop", -3), ("frames", -1), ("length", 0), ("pad", -1),
                  ("pad", 64), ("pad", (1 << 22) + 1), ("rows", -1), ("pad_mode", 2), ("pad_mode", -1), ("flags", 2), ("flags", 4),
                  ("flags", 32), ("flags", 16 | 8), ("sig_imag", p.value), ("window", None), ("scale", float("nan")), ("scale", float("inf")), ("sig_es", -1),
                  ("sig_row_stride", -1), ("spec_row_stride", -1), ("spec_es", -1), ("spec_frame_stride", -1)]
    bad_fields += [("spec_es", 0), ("spec_frame_stride", 0), ("envelope", p.value)] if entry == "cplxamd_stft" else [("sig_es", 0)]
    for field, value in bad_fields:
        assert fn(p, p, p, ctypes.byref(_desc(p, **{field: value})), _lib.F32, p, big, None) == EINVAL, field
    assert fn(p, p, p, ctypes.byref(_desc(p, rows=1 << 20, frames=1 << 20)), _lib.F32, p, big, None) == ESHAPE
    # offsets that would not fit 64 bits: (frames - 1) hop, and rows * length
    assert fn(p, p, p, ctypes.byref(_desc(p, rows=1, frames=1 << 30, hop=1 << 40)), _lib.F32, p, big, None) == ESHAPE
    assert fn(p, p, p, ctypes.byref(_desc(p, rows=1 << 30, frames=1, length=1 << 40)), _lib.F32, p, big, None) == ESHAPE
    assert fn(p, p, p, ref, _lib.F32, p, 16, None) == EWS                                  # workspace too small
    for flags in (0, 1, 8, 9, 16, 17):
        for mode in (ZERO, REFLECT):
            assert fn(p, p, p, ctypes.byref(_desc(p, rows=0, flags=flags, pad_mode=mode)), _lib.F32, p, big, None) == 0   # no launch
    if entry == "cplxamd_stft":
        assert fn(p, p, p, ctypes.byref(_desc(p, frames=0)), _lib.F32, p, big, None) == 0


# ---- argument handling -----------------------------------------------------------------------------------------------------
def _z(*shape, dtype=torch.float32):
    return Cplx(torch.zeros(*shape, dtype=dtype), torch.zeros(*shape, dtype=dtype))


@pytest.mark.parametrize("kwargs", [
    dict(n_fft=0), dict(n_fft=16, hop_length=0), dict(n_fft=16, win_length=17), dict(n_fft=16, win_length=0),
    dict(n_fft=16, window=torch.ones(15)), dict(n_fft=16, win_length=12, window=torch.ones(16)), dict(n_fft=80),
    dict(n_fft=200, center=False),
], ids=lambda kw: " ".join(f"{k}={v if not torch.is_tensor(v) else 'ones(%d)' % len(v)}" for k, v in kw.items()))
def test_stft_argument_errors_are_torchs(kwargs):
    """raised on CPU inputs, so before the device is looked at -- and NOT the package's own error class.  n_fft=80 on 40
    samples is the reflect pad that is not smaller than the signal."""
    with pytest.raises(RuntimeError) as e:
        cplx.stft(torch.zeros(2, 40), **kwargs)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(2, 40), return_complex=True, **kwargs)


def test_a_one_sided_spectrum_of_a_complex_signal_is_torchs_error():
    with pytest.raises(RuntimeError) as e:
        cplx.stft(_z(2, 40), 16, onesided=True)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(2, 40, dtype=torch.complex64), 16, onesided=True, return_complex=True)


@pytest.mark.parametrize("kwargs", [
    dict(n_fft=0), dict(n_fft=16, hop_length=0), dict(n_fft=16, win_length=17), dict(n_fft=16, window=torch.ones(15)),
    dict(n_fft=16, onesided=False), dict(n_fft=18), dict(n_fft=16, hop_length=8, win_length=4),
    dict(n_fft=16, return_complex=True),
], ids=lambda kw: " ".join(f"{k}={v if not torch.is_tensor(v) else 'ones(%d)' % len(v)}" for k, v in kw.items()))
def test_istft_argument_errors_are_torchs(kwargs):
    """onesided=False on a half spectrum, a spectrogram whose N does not match n_fft, hop_length > win_length, a complex
    result from a one-sided spectrum"""
    with pytest.raises(RuntimeError) as e:
        cplx.istft(_z(2, 9, 5), **kwargs)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError):
        torch.istft(torch.zeros(2, 9, 5, dtype=torch.complex64), **kwargs)


def test_there_is_no_host_path():
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.stft(torch.zeros(4, 64), 16)
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.stft(torch.zeros(4, 64, dtype=torch.float16), 16)
    with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
        cplx.stft(torch.zeros(4, 64, dtype=torch.complex64), 16)
    with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
        cplx.stft([1.0, 2.0], 16)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.stft(Cplx(torch.zeros(4, 64), torch.zeros(4, 64, dtype=torch.float64)), 16)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.stft(_z(4, 64), 16)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.stft(torch.zeros(1, (1 << 22) + 8), (1 << 22) + 2)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.istft(_z(4, 9, 5), 16)
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.istft(_z(4, 9, 5, dtype=torch.float16), 16)
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.istft(torch.zeros(4, 9, 5), 16)
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.istft(torch.zeros(4, 9, 5, dtype=torch.complex64), 16)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.istft(Cplx(torch.zeros(4, 9, 5), torch.zeros(4, 9, 5, dtype=torch.float64)), 16)
    with pytest.raises(CplxAmdError, match="exceeds 2\\^22"):
        cplx.istft(_z(1, (1 << 21) + 2, 2), (1 << 22) + 2)


@pytest.mark.parametrize("T, n_fft, hop, win_length, center, onesided, length", sc.SHAPE_CASES)
def test_output_shapes_are_torchs(T, n_fft, hop, win_length, center, onesided, length):
    """shape logic only: no transform runs"""
    win = torch.ones(win_length or n_fft, dtype=torch.float64)
    S = torch.stft(torch.zeros(3, T, dtype=torch.float64), n_fft, hop, win_length, win, center=center, onesided=onesided,
                   return_complex=True)
    assert hoststft.output_shape("stft", (3, T), n_fft, hop, win_length, center, onesided) == tuple(S.shape)
    assert hoststft.output_shape("stft", (2, 3, T), n_fft, hop, win_length, center, onesided) == (2,) + tuple(S.shape)
    assert hoststft.output_shape("stft", (T,), n_fft, hop, win_length, center, onesided) == tuple(S.shape[1:])
    back = torch.istft(S, n_fft, hop, win_length, win, center=center, onesided=onesided, length=length)
    assert hoststft.output_shape("istft", tuple(S.shape), n_fft, hop, win_length, center, onesided, length) == tuple(back.shape)


# ---- the cases of the GPU tests are good cases: torch takes every one of them on the CPU ------------------------------------
def test_every_path_case_passes_torch():
    for n_fft in sc.PATH_LENGTHS:
        x, win, S, xr, xi, y = sc.path_case(n_fft, torch.float32)
        hop, T, rows = sc.path_geometry(n_fft)
        assert 5 <= S.shape[-1] <= 9 and S.shape[:2] == (rows, n_fft // 2 + 1) and rows in (2, 3)
        assert y.shape[0] == rows and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("n", [16, 64])
def test_every_seam_case_passes_torch(n):
    for label, T, kw, kind, inverse in sc.seam_cases(n):
        win = sc.window(kind, kw.get("win_length", n))
        S = sc.ref_stft(torch.zeros(2, T), n, window=win, **kw)
        assert S.shape[-1] >= 1, label
        if inverse:                                        # NOLA holds, or torch raises here
            y = sc.ref_istft(S.real, S.imag, n, window=win, **sc.istft_kwargs(kw))
            assert y.shape[-1] >= 1, label
