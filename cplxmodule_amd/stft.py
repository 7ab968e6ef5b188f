"""Short-time Fourier transforms on the framed, windowed kernels of csrc/stft.hip: the argument handling, the launch glue
and the two autograd Functions behind cplx.stft / cplx.istft.

Two linear primitives (N = n_fft // 2 + 1; sg, w_k, c_k as in rfft.py; src / fold: the padding index map and its inverse
image, csrc/stft_impl.h):
    analysis   S[f][k] = scale [w_k] sum_j win[j] x[src(f hop + j)] e^{sg 2 pi i jk/n_fft}          signal -> plane pair
    synthesis  y[t] = e[t] sum_{p in fold(t)} sum_f (win[j] scale Re sum_k c_k X[f][k] e^{sg 2 pi i jk/n_fft})[j = p - f hop]
stft is analysis (sg -), istft synthesis (sg +, c = w, e = 1 / window envelope).  They are each other's adjoints: the
gradient of analysis is synthesis with the opposite sign, c = 1 exactly when the analysis was unweighted (for stft: NOT
istft), e = 1 and the fold of the forward's pad mode; the gradient of synthesis is analysis of e * g with the opposite
sign, weighted exactly when c = w, and the padding whose fold the synthesis used (for istft: zero padding).  Each
backward is the other Function, so derivatives of every order exist.

One launch of `cplxamd_stft` reads the signal where it lies (any sample stride, zero from `expand` included; the leading
dims as one row run, copied once, differentiably, when they do not collapse to one stride): reflect and constant padding,
framing and the window happen in the kernel's loader.  One launch of `cplxamd_istft` transforms into a workspace of
frames and gathers every output sample in a fixed order.  Workspaces come from torch's allocator; only istft's NOLA check
reads a device value on the host (`check_nola=False`: none).

The full spectrum (`full`: stft of a `Cplx` signal or with `onesided=False`, istft with `return_complex=True`) runs the same
two primitives on the complex kernels: N = n_fft, no w_k / c_k, no Re, signal and result are plane pairs.  A real signal
is a pair whose imaginary plane is None: it is never allocated or read, and its gradient is never written.  istft with
`onesided=False` and a real result reads the first n_fft // 2 + 1 bins of the full spectrum, as torch's does.

A spectrogram whose bins lie further apart than its frames (contiguous as [..., N, frames]) is copied once to the
frames-major order before synthesis: the transform's loads run along the bins, and with a stride they are uncoalesced
(scripts/bench_stft.py times both orders).
"""
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import code
from .fft import MAX_N, PATHS

FLAG_INVERSE, FLAG_WEIGHTED, FLAG_FULL = 1, 8, 16         # CPLXAMD_FFT_INVERSE, CPLXAMD_RFFT_WEIGHTED, CPLXAMD_STFT_FULL
PAD_ZERO, PAD_REFLECT = 0, 1                              # CPLXAMD_STFT_PAD_*
PAD_MODES = ("reflect", "constant", "replicate", "circular")


def plan(n_fft, hop, padded_length, rows, length, dtype=torch.float32, full=False):
    """{path, complex_n, points, vectors_per_workgroup, frames, rows_per_chunk, analysis_ws, synthesis_ws} of the
    transforms of `rows` signals whose padded length is `padded_length` (synthesis: outputs of `length` samples) -- a pure
    host call, no GPU needed.  `full`: the full spectrum on the complex transform of n_fft points."""
    cn, pts, fr, chunk, wa, wsyn = (ctypes.c_int64(0) for _ in range(6))
    vpw = ctypes.c_int(0)
    rc = _lib.load().cplxamd_stft_plan(int(n_fft), int(hop), int(padded_length), int(rows), int(length), code(dtype), int(bool(full)),
                                       ctypes.byref(cn), ctypes.byref(pts), ctypes.byref(vpw), ctypes.byref(fr),
                                       ctypes.byref(chunk), ctypes.byref(wa), ctypes.byref(wsyn))
    if rc < 0:
        raise CplxAmdError(f"stft: no plan for n_fft={n_fft}, hop={hop}, padded length {padded_length}, rows={rows} "
                           f"(n_fft must lie in [1, 2^22 = {MAX_N}] and not exceed the padded length)")
    return dict(path=PATHS[rc], complex_n=cn.value, points=pts.value, vectors_per_workgroup=vpw.value, frames=fr.value,
                rows_per_chunk=chunk.value, analysis_ws=wa.value, synthesis_ws=wsyn.value)


def descriptor(n_fft, hop, frames, length, pad, mode, rows=1, full=False):
    """a StftDesc with dense strides and no pointers: what cplxamd_stft_src / _fold need"""
    n = n_fft if full else n_fft // 2 + 1
    return _lib.StftDesc(n_fft=n_fft, hop=hop, frames=frames, length=length, pad=pad, rows=rows, sig_row_stride=length, sig_es=1,
                         spec_row_stride=frames * n, spec_frame_stride=n, spec_es=1, pad_mode=mode, flags=FLAG_FULL if full else 0,
                         scale=1.0)


def src_index(d, frame, j):
    """sample index of element j of frame `frame` under descriptor d, -1 for "zero" (the kernels' own index map)"""
    return _lib.load().cplxamd_stft_src(ctypes.byref(d), int(frame), int(j))


def fold_positions(d, t):
    """the padded positions that map to sample t under descriptor d, ascending (the kernels' own fold)"""
    out = (ctypes.c_int64 * 3)()
    c = _lib.load().cplxamd_stft_fold(ctypes.byref(d), int(t), out)
    if c < 0:
        raise CplxAmdError(f"stft: sample {t} is outside the descriptor")
    return list(out[:c])


def _row_run(t, keep):
    """the dims of t in front of its last `keep` as ONE run -> (rows, stride), or None when they do not collapse"""
    rows, stride = 1, 0
    for size, s in zip(reversed(t.shape[:t.dim() - keep]), reversed(t.stride()[:t.dim() - keep])):
        if size == 1:
            continue
        if rows > 1 and s != stride * rows:
            return None
        if rows == 1:
            stride = s
        rows *= size
    return rows, stride


def _flags(positive, weighted, full):
    return (FLAG_INVERSE if positive else 0) | (FLAG_WEIGHTED if weighted else 0) | (FLAG_FULL if full else 0)


class _Analysis(torch.autograd.Function):
    """(Sr, Si)[..., k, f] of a signal [..., T] (`xi`: its imaginary plane with x's strides, or None; full only) whose
    leading dims are one row run; the planes are dense as [..., frames, N] and returned transposed"""

    @staticmethod
    def forward(ctx, x, xi, win, meta):
        n_fft, hop, frames, pad, mode, positive, weighted, scale, full = meta
        ctx.meta = meta
        ctx.length = x.shape[-1]
        ctx.has_imag = xi is not None
        ctx.save_for_backward(win)
        lead, n = tuple(x.shape[:-1]), n_fft if full else n_fft // 2 + 1
        yr = torch.empty(lead + (frames, n), dtype=x.dtype, device=x.device)
        yi = torch.empty_like(yr)
        rows, rs = _row_run(x, 1)
        if yr.numel():
            d = _lib.StftDesc(n_fft=n_fft, hop=hop, frames=frames, length=x.shape[-1], pad=pad, rows=rows, sig_row_stride=rs,
                              sig_es=x.stride(-1), spec_row_stride=frames * n, spec_frame_stride=n, spec_es=1, pad_mode=mode,
                              flags=_flags(positive, weighted, full), window=win.data_ptr(), envelope=None,
                              sig_imag=None if xi is None else xi.data_ptr(), scale=scale)
            ws_bytes = plan(n_fft, hop, (frames - 1) * hop + n_fft, rows, x.shape[-1], x.dtype, full)["analysis_ws"]
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            call("cplxamd_stft", ptr(x), ptr(yr), ptr(yi), ctypes.byref(d), code(x.dtype), ptr(ws), ws_bytes, stream_ptr())
        return yr.transpose(-1, -2), yi.transpose(-1, -2)

    @staticmethod
    def backward(ctx, gr, gi):
        n_fft, hop, frames, pad, mode, positive, weighted, scale, full = ctx.meta
        win, = ctx.saved_tensors
        g = synthesis(gr, gi, win, None, n_fft, hop, ctx.length, pad, mode, not positive, weighted, scale, full, ctx.has_imag)
        return (g[0], g[1], None, None) if ctx.has_imag else (g, None, None, None)


class _Synthesis(torch.autograd.Function):
    """y[..., t], t < length, of planes [..., N, frames] that share one layout whose leading dims are one row run.  `ebuf`
    None: e = 1; else a buffer of length + 1 values that the launch fills with e and the envelope's minimum.  full with
    `imag`: the pair (y, its imaginary plane); full without: the real plane alone, the imaginary one is not formed"""

    @staticmethod
    def forward(ctx, pr, pi, win, ebuf, meta):
        n_fft, hop, length, pad, mode, positive, weighted, scale, full, imag = meta
        ctx.meta = meta
        ctx.frames = pr.shape[-1]
        ctx.save_for_backward(win, ebuf)
        y = torch.empty(tuple(pr.shape[:-2]) + (length,), dtype=pr.dtype, device=pr.device)
        yi = torch.empty_like(y) if imag else None
        rows, rs = _row_run(pr, 2)
        if y.numel():
            d = _lib.StftDesc(n_fft=n_fft, hop=hop, frames=pr.shape[-1], length=length, pad=pad, rows=rows, sig_row_stride=length,
                              sig_es=1, spec_row_stride=rs, spec_frame_stride=pr.stride(-1), spec_es=pr.stride(-2), pad_mode=mode,
                              flags=_flags(positive, weighted, full), window=win.data_ptr(),
                              envelope=None if ebuf is None else ebuf.data_ptr(), sig_imag=None if yi is None else yi.data_ptr(),
                              scale=scale)
            ws_bytes = plan(n_fft, hop, (pr.shape[-1] - 1) * hop + n_fft, rows, length, pr.dtype, full)["synthesis_ws"]
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pr.device)
            call("cplxamd_istft", ptr(pr), ptr(pi), ptr(y), ctypes.byref(d), code(pr.dtype), ptr(ws), ws_bytes, stream_ptr())
        return (y, yi) if imag else y

    @staticmethod
    def backward(ctx, g, gi=None):
        n_fft, hop, length, pad, mode, positive, weighted, scale, full, imag = ctx.meta
        win, ebuf = ctx.saved_tensors
        if ebuf is not None:
            g = (g * ebuf[:length]).to(g.dtype)
            gi = None if gi is None else (gi * ebuf[:length]).to(gi.dtype)
        dr, di = analysis(g, gi, win, n_fft, hop, ctx.frames, pad, mode, not positive, weighted, scale, full)
        return dr, di, None, None, None


def analysis(x, xi, win, n_fft, hop, frames, pad, mode, positive, weighted, scale, full=False):
    """the analysis primitive of a signal [..., T] (xi: its imaginary plane or None; full only) -> planes [..., N, frames]"""
    if _row_run(x, 1) is None or (xi is not None and xi.stride() != x.stride()):
        x = x.contiguous()                                # one differentiable copy
        xi = None if xi is None else xi.contiguous()
    return _Analysis.apply(x, xi, win, (n_fft, hop, frames, pad, mode, bool(positive), bool(weighted), float(scale), bool(full)))


def synthesis(pr, pi, win, ebuf, n_fft, hop, length, pad, mode, positive, weighted, scale, full=False, imag=False):
    """the synthesis primitive of planes [..., N, frames] of one dtype and shape -> a real tensor [..., length] (full with
    `imag`: the pair of planes of the complex result)"""
    strided_bins = pr.shape[-2] > 1 and pr.shape[-1] > 1 and pr.stride(-2) > pr.stride(-1) > 0
    if pr.stride() != pi.stride() or _row_run(pr, 2) is None or strided_bins:      # one differentiable copy, frames-major
        pr = pr.transpose(-1, -2).contiguous().transpose(-1, -2)
        pi = pi.transpose(-1, -2).contiguous().transpose(-1, -2)
    return _Synthesis.apply(pr, pi, win, ebuf, (n_fft, hop, length, pad, mode, bool(positive), bool(weighted), float(scale),
                                                bool(full), bool(imag)))


# ---- argument rules: torch.stft's and torch.istft's, with torch's exception types, before the device is looked at --------
def _framing(name, n_fft, hop_length, win_length, window):
    n_fft = int(n_fft)
    if n_fft < 1:
        raise RuntimeError(f"{name}: expected 0 < n_fft, but got n_fft={n_fft}")
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if hop < 1:
        raise RuntimeError(f"{name}: expected hop_length > 0, but got hop_length={hop}")
    win_length = n_fft if win_length is None else int(win_length)
    if not 0 < win_length <= n_fft:
        raise RuntimeError(f"{name}: expected 0 < win_length <= n_fft, but got win_length={win_length}")
    if window is not None:
        if not torch.is_tensor(window):
            raise TypeError(f"{name}: window must be a Tensor or None, got {type(window).__name__}")
        if window.dim() != 1 or window.shape[0] != win_length:
            raise RuntimeError(f"{name}: expected a 1D window tensor of size equal to win_length={win_length}, but got "
                               f"window with size {list(window.shape)}")
    return n_fft, hop, win_length


def _window(name, window, win_length, n_fft, compute, device):
    """the window in the compute type, centred in n_fft zeros"""
    if window is None:
        w = torch.ones(win_length, dtype=compute, device=device)
    else:
        if window.is_complex() or not window.is_floating_point():
            raise CplxAmdError(f"{name}: the window has dtype {window.dtype}; it must be a real floating tensor")
        if window.requires_grad:
            raise CplxAmdError(f"{name}: the window requires grad; it is a constant of the transform (detach it)")
        w = window.detach().to(compute)
    if win_length < n_fft:
        left = (n_fft - win_length) // 2
        w = F.pad(w, (left, n_fft - win_length - left))
    return w.contiguous()


def output_shape(name, shape, n_fft, hop_length=None, win_length=None, center=True, onesided=True, length=None):
    """the shape cplx.<name> gives an input of `shape` (argument rules only: nothing is transformed)"""
    n_fft, hop, _ = _framing(name, n_fft, hop_length, win_length, None)
    pad = n_fft // 2 if center else 0
    if name == "stft":
        padded = shape[-1] + 2 * pad
        if n_fft > padded:
            raise RuntimeError(f"stft: expected 0 < n_fft <= {padded}, but got n_fft={n_fft}")
        return tuple(shape[:-1]) + (n_fft // 2 + 1 if onesided else n_fft, 1 + (padded - n_fft) // hop)
    covered = n_fft + hop * (shape[-1] - 1)
    return tuple(shape[:-2]) + (covered - 2 * pad if length is None else int(length),)


def stft(input, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", normalized=False,
         onesided=None):
    from .cplx import Cplx
    is_cplx = isinstance(input, Cplx)
    if not is_cplx and (not torch.is_tensor(input) or input.is_complex()):
        raise CplxAmdError(f"stft: the input is a {type(input).__name__}"
                           f"{' of complex dtype' if torch.is_tensor(input) else ''}, not a real torch.Tensor")
    x = input.real if is_cplx else input
    n_fft, hop, win_length = _framing("stft", n_fft, hop_length, win_length, window)
    if x.dim() < 1:
        raise RuntimeError("stft: expected a tensor with at least one dimension")
    length = x.shape[-1]
    pad = n_fft // 2 if center else 0
    if center:
        if pad_mode not in PAD_MODES:
            raise NotImplementedError(f"stft: unknown pad_mode {pad_mode!r}")
        if pad_mode == "reflect" and pad >= length:
            raise RuntimeError(f"stft: padding size should be less than the corresponding input dimension, but got: padding "
                               f"({pad}, {pad}) at dimension {x.dim() - 1} of input {list(x.shape)}")
        if pad_mode == "circular" and pad > length:
            raise RuntimeError("stft: padding value causes wrapping around more than once")
    padded = length + 2 * pad
    if n_fft > padded:
        raise RuntimeError(f"stft: expected 0 < n_fft <= {padded}, but got n_fft={n_fft}")
    if is_cplx and onesided:
        raise RuntimeError("stft: cannot have onesided output if window or input is complex")
    onesided = (not is_cplx) if onesided is None else bool(onesided)
    if is_cplx and input.real.dtype != input.imag.dtype:
        raise CplxAmdError(f"stft: the planes have different dtypes: {input.real.dtype} and {input.imag.dtype}")
    code(x.dtype)
    if n_fft > MAX_N:
        raise CplxAmdError(f"stft: length {n_fft} exceeds 2^22 = {MAX_N}, the longest transform supported")
    xi = input.imag if is_cplx else None
    require_device(x, xi, window)
    compute = torch.float64 if x.dtype == torch.float64 else torch.float32
    win = _window("stft", window, win_length, n_fft, compute, x.device)
    mode = PAD_ZERO
    if center and pad_mode == "reflect":
        mode = PAD_REFLECT
    elif center and pad_mode != "constant":               # replicate, circular: one padded copy, then no padding
        def padded_copy(t):
            if not t.numel():                             # zero rows: nothing to pad, and a row count of -1 would be ambiguous
                return F.pad(t, (pad, pad))
            return F.pad(t.reshape(1, math.prod(t.shape[:-1]), length), (pad, pad), mode=pad_mode).reshape(*t.shape[:-1], padded)
        x, xi = padded_copy(x), None if xi is None else padded_copy(xi)
        pad = 0
    frames = 1 + (padded - n_fft) // hop
    scale = n_fft ** -0.5 if normalized else 1.0
    return Cplx(*analysis(x, xi, win, n_fft, hop, frames, pad, mode, False, False, scale, not onesided))


def istft(input, n_fft, hop_length=None, win_length=None, window=None, center=True, normalized=False, onesided=None,
          length=None, return_complex=False, *, check_nola=True):
    from .cplx import Cplx
    if not isinstance(input, Cplx):
        raise CplxAmdError(f"istft: the input is a {type(input).__name__}, not a Cplx (wrap planes with Cplx(re, im); "
                           "torch complex tensors are not taken)")
    pr, pi = input.real, input.imag
    n_fft, hop, win_length = _framing("istft", n_fft, hop_length, win_length, window)
    if hop > win_length:
        raise RuntimeError(f"istft: expected hop_length <= win_length, but got hop_length={hop}, win_length={win_length}")
    if pr.dim() < 2:
        raise RuntimeError("istft: expected a spectrogram with at least two dimensions [..., N, frames]")
    bins, frames = pr.shape[-2], pr.shape[-1]
    if frames < 1 or bins < 1:
        raise RuntimeError("istft: expected a non-empty spectrogram")
    onesided = (bins != n_fft) if onesided is None else bool(onesided)
    if onesided and bins != n_fft // 2 + 1:
        raise RuntimeError(f"istft: expected the frequency dimension (3rd to the last) of the input tensor to match "
                           f"n_fft / 2 + 1 = {n_fft // 2 + 1} when onesided=True, but got {bins}")
    if not onesided and bins != n_fft:
        raise RuntimeError(f"istft: expected the frequency dimension (3rd to the last) of the input tensor to match "
                           f"n_fft = {n_fft} when onesided=False, but got {bins}")
    if return_complex and onesided:
        raise RuntimeError("istft: cannot have onesided output if window or input is complex")
    pad = n_fft // 2 if center else 0
    covered = n_fft + hop * (frames - 1)
    out_length = covered - 2 * pad if length is None else int(length)
    if out_length < 1:
        raise RuntimeError(f"istft: the frames cover no output sample (output length {out_length})")
    if pr.dtype != pi.dtype:
        raise CplxAmdError(f"istft: the planes have different dtypes: {pr.dtype} and {pi.dtype}")
    code(pr.dtype)
    if n_fft > MAX_N:
        raise CplxAmdError(f"istft: length {n_fft} exceeds 2^22 = {MAX_N}, the longest transform supported")
    require_device(pr, pi, window)
    if not onesided and not return_complex:                                 # a real result reads the first half of a full spectrum, as torch's does
        pr, pi = pr.narrow(-2, 0, n_fft // 2 + 1), pi.narrow(-2, 0, n_fft // 2 + 1)
    compute = torch.float64 if pr.dtype == torch.float64 else torch.float32
    win = _window("istft", window, win_length, n_fft, compute, pr.device)
    if check_nola and pr.numel() and torch.cuda.is_current_stream_capturing():
        raise CplxAmdError("istft: the NOLA check reads a device value on the host, which a stream capture cannot do: pass "
                           "check_nola=False (and check the window once, outside the capture)")
    ebuf = torch.empty(out_length + 1, dtype=compute, device=pr.device)
    scale = (math.sqrt(n_fft) if normalized else 1.0) / n_fft
    y = synthesis(pr, pi, win, ebuf, n_fft, hop, out_length, pad, PAD_ZERO, True, not return_complex, scale, return_complex,
                  return_complex)
    if check_nola and pr.numel() and float(ebuf[out_length]) < 1e-11:
        raise RuntimeError("istft: window overlap add min: 1 (the window envelope falls below 1e-11 inside the output: "
                           "NOLA is violated)")
    return Cplx(*y) if return_complex else y
