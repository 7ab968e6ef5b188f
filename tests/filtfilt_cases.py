"""Shared fixtures of the cplx.filtfilt / sosfiltfilt / lfilter_zi / sosfilt_zi tests (test_filtfilt_host.py,
test_gpu_filtfilt.py): the numpy oracle, the numpy emulation of the kernel's extension index map, the seam lists.

Oracle, in complex128 (or complex64 for the coverage condition): the extension of scipy's filtfilt(method="pad") ->
iir_cases.lfilter / sosfilt from the closed-form steady state scaled by the first sample -> reverse -> the same again ->
reverse -> trim.  Nothing is conjugated.  Bounds: iir_cases.py's (fft_cases.tol; integer cases compare with EQUAL).
"""
import functools
import os

import numpy as np

import iir_cases as ic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filtfilt_scipy.npz")
PADTYPES = ("odd", "even", "constant", None)
# the filters of the exact tests: their lfilter_zi is a Gaussian integer or half-integer (sum a != 0), so it is exact
EXACT_FILTERS = ("cos", "six", "three", "eight")
EXACT_CASCADES = ("two", "three")
MAP_CASES = ((2, 1), (7, 6), (64, 9), (4096, 27), (5000, 4999))
COVERAGE_N = ic.COVERAGE_N
COVERAGE_BOUND = ic.COVERAGE_BOUND


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def key(padtype):
    return "none" if padtype is None else padtype


# ---- the steady state of the unit step, in closed form ------------------------------------------------------------------
def lfilter_zi(b, a, dtype=np.complex128):
    """b, a 1-d or [R, n] -> zi [R, D] (1-d operands: [D])"""
    one = np.ndim(b) == 1 and np.ndim(a) == 1
    bb, aa, d = ic._coefs(b, a, max(np.atleast_2d(b).shape[0], np.atleast_2d(a).shape[0]), dtype)
    c = np.cumsum(bb[:, 1:] - aa[:, 1:] * bb[:, :1], axis=-1)
    if d == 0:
        zi = np.zeros((bb.shape[0], 0), dtype=dtype)
    else:
        z0 = c[:, -1:] / aa.sum(-1, keepdims=True)
        zi = np.cumsum(aa[:, :d], axis=-1) * z0 - np.concatenate([np.zeros_like(c[:, :1]), c[:, :-1]], -1)
    return (zi[0] if one else zi).astype(dtype)


def sosfilt_zi(sos, dtype=np.complex128):
    """sos [S, 6] -> zi [S, 2]"""
    sos = np.asarray(sos, dtype=dtype)
    zi = np.zeros((len(sos), 2), dtype=dtype)
    scale = 1.0
    for s, sec in enumerate(sos):
        zi[s] = scale * lfilter_zi(sec[:3], sec[3:], dtype)
        scale = scale * (sec[:3].sum() / sec[3:].sum())
    return zi


# ---- the extension ----------------------------------------------------------------------------------------------------------
def default_padlen(nb=None, na=None, sections=None):
    return 3 * (2 * sections + 1) if sections is not None else 3 * max(na, nb)


def extend(x, e, padtype):
    """x [R, N] -> [R, N + 2 e], with numpy slices as scipy's odd_ext / even_ext / const_ext"""
    x = np.asarray(x)
    if padtype is None or e == 0:
        return x
    n = x.shape[-1]
    assert e < n
    left, right = x[:, e:0:-1], x[:, n - 2:n - 2 - e:-1] if n - 2 - e >= 0 else x[:, n - 2::-1]
    if padtype == "even":
        return np.concatenate([left, x, right], -1)
    if padtype == "odd":
        return np.concatenate([2 * x[:, :1] - left, x, 2 * x[:, -1:] - right], -1)
    ones = np.ones((1, e), dtype=x.dtype)
    return np.concatenate([x[:, :1] * ones, x, x[:, -1:] * ones], -1)


def src(m, n, e, padtype):
    """the numpy emulation of the kernel's index map: (j, k), the sample being x[j] (k < 0), x[k] (j < 0) or 2 x[k] - x[j]"""
    i = m - e
    if 0 <= i < n:
        return i, -1
    k, j = (0, -i) if i < 0 else (n - 1, 2 * (n - 1) - i)
    if padtype == "constant":
        return -1, k
    return j, (k if padtype == "odd" else -1)


def from_map(x, e, padtype, index=src):
    """the extension of the rows x [R, N] built sample by sample from an index map"""
    n = x.shape[-1]
    out = np.zeros((x.shape[0], n + 2 * e), dtype=x.dtype)
    for m in range(n + 2 * e):
        j, k = index(m, n, e, padtype)
        out[:, m] = x[:, j] if k < 0 else (x[:, k] if j < 0 else 2 * x[:, k] - x[:, j])
    return out


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def _edge(padtype, padlen, default):
    return 0 if padtype is None else (default if padlen is None else padlen)


def filtfilt(b, a, x, padtype="odd", padlen=None, dtype=np.complex128):
    """x [R, N]; b, a 1-d or [R, n] -> y [R, N]; filtfilt.peak: the largest plane entry of any signal or state on the way"""
    x = np.asarray(x, dtype=dtype)
    e = _edge(padtype, padlen, default_padlen(np.shape(b)[-1], np.shape(a)[-1]))
    zi = np.atleast_2d(lfilter_zi(b, a, dtype))
    ext = extend(x, e, padtype).astype(dtype)
    peak = _peak(ext)
    y, _ = ic.lfilter(b, a, ext, zi * ext[:, :1], dtype)
    peak = max(peak, _peak(y), ic.lfilter.peak)
    y, _ = ic.lfilter(b, a, y[:, ::-1], zi * y[:, -1:], dtype)
    filtfilt.peak = max(peak, _peak(y), ic.lfilter.peak)
    return y[:, ::-1][:, e:e + x.shape[-1]]


def sosfiltfilt(sos, x, padtype="odd", padlen=None, dtype=np.complex128):
    """sos [S, 6]; x [R, N] -> y [R, N]"""
    x = np.asarray(x, dtype=dtype)
    sos = np.asarray(sos, dtype=dtype)
    e = _edge(padtype, padlen, default_padlen(sections=sos.shape[-2]))
    zi = sosfilt_zi(sos, dtype)[None]
    ext = extend(x, e, padtype).astype(dtype)
    y, _ = ic.sosfilt(sos, ext, zi * ext[:, :1, None], dtype)
    peak = max(_peak(ext), _peak(y))
    y, _ = ic.sosfilt(sos, y[:, ::-1], zi * y[:, -1:, None], dtype)
    sosfiltfilt.peak = max(peak, _peak(y))
    return y[:, ::-1][:, e:e + x.shape[-1]]


def _peak(z):
    return max(np.abs(z.real).max(), np.abs(z.imag).max()) if z.size else 0.0


def _many(one, x, e):
    """one(x, padtype, padlen) for every padtype -> ({padtype: y}, the largest peak); the three extensions of one length
    run stacked as rows of one call"""
    rows = x.shape[0]
    out, peak = {}, 0.0
    if e > 0:
        ext = np.concatenate([extend(x, e, p) for p in PADTYPES[:3]], 0)
        y = one(ext, None, 0)[:, e:e + x.shape[-1]]
        peak = one.peak
        for i, p in enumerate(PADTYPES[:3]):
            out[p] = y[i * rows:(i + 1) * rows]
    else:
        out["odd"] = one(x, None, 0)
        peak = one.peak
        out["even"] = out["constant"] = out["odd"]
    out[None] = one(x, None, 0)
    return out, max(peak, one.peak)


# ---- the integer cases of the exact GPU tests: data, references (computed once, shared, never written to) and peaks ------------
QUANTUM = {"eight": 0.25}                                 # a half-integer zi twice: multiples of 1 / 4; else integers
# (N, padlen) whose float32 arithmetic test_filtfilt_host.py's headroom assertion does NOT admit on this data (it asserts
# that too): two-pass outputs of the unit-circle filters grow with the extended length, the double poles of `three`
# fastest.  They run in float64 only, where every case is exact.
T3 = 3 * 4096 + 77
EXCLUDED = {("ba", "six"): {(5000, 4999)},
            ("ba", "three"): {(4071, None), (4072, None), (4073, None), (4096, None), (T3, None), (5000, 4999), (5003, None)},
            ("ba", "eight"): {(T3, None), (5000, 4999)},
            ("sos", "two"): {(T3, None), (5000, 4999)},
            ("sos", "three"): {(4053, None), (4054, None), (4055, None), (4096, None), (T3, None), (5000, 4999), (5003, None)}}
PADLENS = (0, 1, 64, 65)                                  # explicit values: none, one sample, the chunk seam
PADLEN_N = 200
LONG_EDGE = (5000, 4999)                                  # an extension longer than a tile
SPLIT_N = 5003
SPLIT_SEGMENTS = (2, 3, 7)
ROWS = 3


def exact_filter(kind, name):
    """("ba", name) -> (b, a); ("sos", name) -> sos [S, 6]"""
    return ic.int_sos(name) if kind == "sos" else ic.INT_FILTERS[name][:2]


def exact_edge(kind, name):
    f = exact_filter(kind, name)
    return default_padlen(sections=len(f)) if kind == "sos" else default_padlen(len(f[0]), len(f[1]))


def exact_cases(kind, name, float64=False):
    """(N, padlen) of the exact tests: the seams with the default padlen, the explicit padlens, the long edge; float32
    arithmetic (float32 and bfloat16 operands) takes those that its headroom admits"""
    e = exact_edge(kind, name)
    cases = [(n, None) for n in seam_lengths(e)] + [(PADLEN_N, p) for p in PADLENS] + [LONG_EDGE]
    return [c for c in cases if float64 or admitted(kind, name, c)]


def admitted(kind, name, case):
    return case not in EXCLUDED.get((kind, name), ())


def exact_signal(n):
    return ic.int_data((ROWS, n), n)


@functools.lru_cache(maxsize=None)
def exact_reference(kind, name, n, padlen):
    """({padtype: y [ROWS, N]}, peak) of the integer signal exact_signal(n) through the integer filter: complex128"""
    f = exact_filter(kind, name)
    e = exact_edge(kind, name) if padlen is None else padlen
    if kind == "sos":
        one = lambda x, p, q: sosfiltfilt(f, x, p, q)     # noqa: E731
        peak = lambda: sosfiltfilt.peak                   # noqa: E731
    else:
        one = lambda x, p, q: filtfilt(f[0], f[1], x, p, q)   # noqa: E731
        peak = lambda: filtfilt.peak                      # noqa: E731

    class Run:
        def __call__(self, x, p, q):
            y = one(x, p, q)
            self.peak = peak()
            return y
    out, top = _many(Run(), exact_signal(n), e)
    for y in out.values():
        y.setflags(write=False)
    return out, top


# ---- the seams -----------------------------------------------------------------------------------------------------------------
def seam_lengths(e, nmax=None):
    """N = e + 1; the chunk seam 63 .. 65 and the tile seam 4095 .. 4097 of the EXTENDED row (N + 2 e); one tile of signal;
    three tiles and a rest -- each at least e + 1"""
    ns = {e + 1, 4096, 3 * 4096 + 77}
    ns |= {t - 2 * e for t in (63, 64, 65, 4095, 4096, 4097)}
    return sorted(n for n in ns if n >= e + 1 and (nmax is None or n <= nmax))
