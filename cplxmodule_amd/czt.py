"""Chirp-z transforms of planar `Cplx` tensors on the fused chirp-z kernel (csrc/czt.hip): the argument handling, the
contour guard, the launch glue and the autograd Function behind cplx.czt / zoom_fft / czt_points.

For every vector along the last dim, with host scalars w and a,

    y[k] = sum_{j < n} x[j] a^{-j} w^{jk},   k = 0 .. m - 1,

Bluestein's convolution of length n + m - 1 run at M = 2^ceil(log2(n + m - 1)) (at least 8): up to M = 8192 one launch
reads the n inputs and writes the m outputs of a vector, with nothing of length M in memory; up to M = 2^22 the
transform goes through the workspace.  The kernel is handed w and a as log-modulus and TURN FRACTION (arg / 2 pi): its
tables are built from those in float64 with exactly reduced phases.  `zoom_fft` passes the fractions it computes
(-scale / m, f1 / fs) as they are; `czt` takes them from the complex numbers it is given.

The leading dims are batch: they are sorted by stride and fused into at most three runs, jointly for the input and the
output (_runs.py; a sliced, `expand`ed or transposed input is read in place); planes that share no layout, or that need
more than three runs, are copied once, differentiably.  A real input is a null imaginary plane: no zero plane is built.

The transform is linear: its adjoint is the transform with n and m swapped, both turn fractions negated and the power of
a on the outputs (CPLXAMD_CZT_A_OUT), so the backward is the same Function applied to the incoming gradient.  It is
differentiable to any order in x; w and a are numbers and get no gradient.  The workspace comes from torch's caching
allocator and nothing reads a device value on the host: calls can be captured in a hipGraph.

Off the unit circle the three tables span a factor e^D, D = |ln|w|| max(n, m)^2 / 2 + |ln|a|| n, and the result loses
that much precision: the error follows eps e^D (a property of the algorithm: scipy's float64 czt returns a relative
error of 1e24 for n = 1000, m = 24, |w|^{nm} = 0.01).  Beyond D = ln 2^24 (float32, bfloat16) / ln 2^53 (float64) no
digit is correct and the call raises CplxAmdError; below, the result is what it is.
"""
import cmath
import ctypes
import functools
import math
import numbers

import torch

from . import _lib
from ._lib import CplxAmdError, call, ptr, require_device, stream_ptr
from ._runs import fill, fit_like, planes

code = functools.partial(_lib.plane_code, "czt: planes must be float32, bfloat16 or float64")
MAX_M = 1 << 22                       # CPLXAMD_WELCH_MAX_N: the longest convolution
PATHS = ("packed", "fused", "workspace")      # cplxamd_czt_plan's return codes
D_MAX = {torch.float32: 24 * math.log(2), torch.bfloat16: 24 * math.log(2), torch.float64: 53 * math.log(2)}


def transform_size(n, m):
    """M = 2^ceil(log2(n + m - 1)), at least 8"""
    M = 8
    while M < n + m - 1:
        M *= 2
    return M


def plan(n, m, vectors, dtype=torch.float32):
    """(path, vectors per workgroup, workspace bytes) of a transform of `vectors` vectors of n inputs and m outputs whose
    input planes have `dtype` -- a pure host call, no GPU needed.  Raises CplxAmdError when n + m - 1 exceeds 2^22."""
    vpw, ws = ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.load().cplxamd_czt_plan(int(n), int(m), int(vectors), code(dtype), ctypes.byref(vpw), ctypes.byref(ws))
    if rc == -3:
        raise CplxAmdError(f"czt: n + m - 1 = {n + m - 1} exceeds 2^22 = {MAX_M}, the longest convolution supported")
    if rc < 0:
        raise CplxAmdError(f"czt: invalid sizes n = {n}, m = {m}, vectors = {vectors}")
    return PATHS[rc], vpw.value, ws.value


def spread(n, m, w_log, a_log):
    """D: the log of the factor the tables of a contour span"""
    return abs(w_log) * max(n, m) ** 2 / 2 + abs(a_log) * n


def guard(n, m, w_log, a_log, dtype, name="czt"):
    D = spread(n, m, w_log, a_log)
    if not D <= D_MAX[dtype]:
        bits = 53 if dtype == torch.float64 else 24
        raise CplxAmdError(
            f"{name}: the contour leaves no correct digit: D = |ln|w|| max(n, m)^2 / 2 + |ln|a|| n = {D:.4g} exceeds "
            f"ln 2^{bits} = {D_MAX[dtype]:.4g} for {dtype} planes (the chirp-z algorithm loses a factor e^D of precision)")
    return D


class _Czt(torch.autograd.Function):
    """(yr, yi) = the chirp-z transform along the last dim of planes (pr, pi; pi may be None) that share one layout of
    at most three batch runs."""

    @staticmethod
    def forward(ctx, pr, pi, meta):
        m, w_log, w_turn, a_log, a_turn, a_out, batch, ys = meta
        n = pr.shape[-1]
        ctx.meta = (n, w_log, w_turn, a_log, a_turn, a_out)
        ctx.real = pi is None
        yr = torch.empty_strided(pr.shape[:-1] + (m,), ys, dtype=pr.dtype, device=pr.device)
        yi = torch.empty_like(yr)
        if yr.numel() == 0:
            return yr, yi
        d = _lib.CztDesc(n=n, m=m, x_es=pr.stride(-1), y_es=yr.stride(-1), flags=_lib.CZT_A_OUT if a_out else 0,
                         w_log=w_log, w_turn=w_turn, a_log=a_log, a_turn=a_turn, scale=1.0)
        vectors, _ = fill(d, batch, ("x_stride", "y_stride"))
        _, _, ws_bytes = plan(n, m, vectors, pr.dtype)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pr.device)
        call("cplxamd_czt", ptr(pr), ptr(pi), ptr(yr), ptr(yi), ctypes.byref(d), code(pr.dtype), code(pr.dtype),
             ptr(ws), ws_bytes, stream_ptr())
        return yr, yi

    @staticmethod
    def backward(ctx, gr, gi):
        n, w_log, w_turn, a_log, a_turn, a_out = ctx.meta
        dr, di = transform(gr, gi, n, w_log, -w_turn, a_log, -a_turn, not a_out)
        return dr, None if ctx.real else di, None


def transform(pr, pi, m, w_log, w_turn, a_log, a_turn, a_out=False):
    """the chirp-z transform along the last dim of planes pr, pi (None: zeros) -> planes [..., m] of the same dtype, in
    pr's memory order.  Differentiable to any order."""
    dim = pr.dim() - 1
    pr, pi, batch, ys = fit_like(pr, pi, dim, m)          # at most one differentiable copy
    return _Czt.apply(pr, pi, (int(m), float(w_log), float(w_turn), float(a_log), float(a_turn), bool(a_out), batch,
                               tuple(ys)))


def _number(v, name, fn):
    if torch.is_tensor(v):
        raise CplxAmdError(f"{fn}: `{name}` is a tensor; the contour parameters are Python numbers (they get no gradient)")
    if not isinstance(v, numbers.Number):
        raise CplxAmdError(f"{fn}: `{name}` is a {type(v).__name__}, not a number")
    return complex(v)


def _polar(z, name, fn):
    """(ln |z|, arg z / 2 pi) of a complex number"""
    if z == 0 or not cmath.isfinite(z):
        raise ValueError(f"{fn}: `{name}` = {z} has no finite logarithm")
    return math.log(abs(z)), math.atan2(z.imag, z.real) / (2 * math.pi)


def _sizes(pr, m, fn):
    """scipy's size rules for the plane pr -> (n, m).  ValueError in scipy's words, before the device is looked at."""
    shape = pr.shape
    if len(shape) == 0:
        raise ValueError(f"{fn}: the input has no dimension to transform (a 0-d input)")
    n = shape[-1]
    if n < 1:
        raise ValueError(f"Invalid number of CZT data points ({n}) specified. n must be positive and integer type.")
    if m is None:
        m = n
    elif isinstance(m, bool) or not isinstance(m, numbers.Integral) or m < 1:
        raise ValueError(f"Invalid number of CZT output points ({m}) specified. m must be positive and integer type.")
    return n, int(m)


def _checked(x, fn):
    from .cplx import Cplx
    if not isinstance(x, Cplx) and not torch.is_tensor(x):
        raise CplxAmdError(f"{fn}: the input is a {type(x).__name__}, not a Cplx or a real torch.Tensor")
    pr, pi = planes(x, "x", fn)
    code(pr.dtype)
    return pr, pi


def _run(pr, pi, n, m, w_log, w_turn, a_log, a_turn, fn):
    from .cplx import Cplx
    guard(n, m, w_log, a_log, pr.dtype, fn)
    if transform_size(n, m) > MAX_M:
        raise CplxAmdError(f"{fn}: n + m - 1 = {n + m - 1} exceeds 2^22 = {MAX_M}, the longest convolution supported")
    require_device(pr, pi)
    return Cplx(*transform(pr, pi, m, w_log, w_turn, a_log, a_turn))


def czt(x, m=None, w=None, a=1 + 0j):
    pr, pi = _checked(x, "czt")
    n, m = _sizes(pr, m, "czt")
    a = _number(a, "a", "czt")
    if w is not None:
        w = _number(w, "w", "czt")
    if w is None and a == 1 and m >= n and m & (m - 1) == 0 and pi is not None:   # a zero-padded power-of-two FFT
        from . import fft as _fft
        from .cplx import Cplx
        if m > _fft.MAX_N:
            raise CplxAmdError(f"czt: length {m} exceeds 2^22 = {MAX_M}, the longest transform supported")
        require_device(pr, pi)
        return Cplx(*_fft.transform(pr, pi, m, pr.dim() - 1, False, 1.0, pr.dtype))
    w_log, w_turn = (0.0, -1.0 / m) if w is None else _polar(w, "w", "czt")
    a_log, a_turn = _polar(a, "a", "czt")
    return _run(pr, pi, n, m, w_log, w_turn, a_log, a_turn, "czt")


def zoom_params(n, fn, m=None, fs=2, endpoint=False):
    """scipy's ZoomFFT mapping -> (m, w's turn fraction, a's turn fraction): w = e^{2 pi i w_turn}, a = e^{2 pi i a_turn}"""
    if m is None:
        m = n
    try:
        band = [float(v) for v in fn]
    except TypeError:                                     # a scalar: the band [0, fn]
        band = [float(fn)]
    if len(band) == 2:
        f1, f2 = band
    elif len(band) == 1:
        f1, f2 = 0.0, band[0]
    else:
        raise ValueError("fn must be a scalar or 2-length sequence")
    fs = float(fs)
    scale = ((f2 - f1) * m) / (fs * (m - 1)) if endpoint else (f2 - f1) / fs
    return m, -scale / m, f1 / fs


def zoom_fft(x, fn, m=None, fs=2, endpoint=False):
    pr, pi = _checked(x, "zoom_fft")
    n, m = _sizes(pr, m, "zoom_fft")
    m, w_turn, a_turn = zoom_params(n, fn, m, fs, endpoint)
    return _run(pr, pi, n, m, 0.0, w_turn, 0.0, a_turn, "zoom_fft")


def czt_points(m, w=None, a=1 + 0j):
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or m < 1:
        raise ValueError(f"Invalid number of CZT output points ({m}) specified. m must be positive and integer type.")
    a = _number(a, "a", "czt_points")
    k = torch.arange(m, dtype=torch.float64)
    if w is None:
        return a * torch.polar(torch.ones_like(k), 2 * math.pi * k / m)
    w = _number(w, "w", "czt_points")
    return a * torch.pow(torch.tensor(w, dtype=torch.complex128), -k)
