"""Shared fixtures of the cplx.lfilter / cplx.sosfilt tests (test_iir_host.py, test_gpu_iir.py): the filters, the
sequential numpy oracle, the numpy emulation of the kernel's chunk / tile / segment scheme and the bounds.

Oracle: the direct-form-II-transposed recurrence as a loop over the samples, in complex128 (or, for the coverage
condition of the Gaussian filters, in complex64):
    y[n] = b0 x[n] + z0,   z_i = b_{i+1} x[n] - a_{i+1} y[n] + z_{i+1}
Bounds: fft_cases.py's (float32 norm-wise 1e-5, float64 1e-11, bf16 per entry 2^-8 |ref| + 1e-5 max|ref| with no
violation allowed; the bf16 reference is formed from the rounded inputs).  Integer cases are compared with EQUAL.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iir_scipy.npz")
J = 1j

# ---- integer and Gaussian-integer filters whose impulse responses stay bounded or grow polynomially: name -> (b, a, N max)
# The sequential recurrence of the double integrator is exact up to N = 2048 (|y| <= 2 N^2 per plane).  The chunked scheme
# also multiplies states by its tables, whose entries reach chunk + 1 = 65 for this filter: D table-times-state products
# must stay below 2^24 (test_iir_host.py asserts it on the very data of the GPU tests), which holds up to N = 600.
INT_FILTERS = {
    "cumsum": ([1], [1, -1], None),
    "double": ([1], [1, -2, 1], 600),
    "rot": ([1, 2 * J], [1, -J], None),
    "cos": ([1, -1, 2], [1, 0, 1], None),
    "six": ([2, J], [1, -1, 1], None),
    "three": ([1, 0, -1, 3], [1, 1, 1], None),
    "four": ([1, 1], [1, 0, 0, 0, -1], None),
    "eight": ([1, -J, 2], [1, 0, 0, 0, 0, 0, 0, 0, 1], None),
}
# cascades of the biquads above (each padded to three taps)
INT_CASCADES = {"two": ("cos", "six"), "three": ("cos", "six", "three3")}
_BIQUADS = {"cos": ([1, -1, 2], [1, 0, 1]), "six": ([2, J, 0], [1, -1, 1]), "three3": ([1, 0, -1], [1, 1, 1])}

# the Gaussian filters: names of the designs recorded in the golden file (scripts/gen_iir_golden.py)
GAUSS_BA = ("butter2", "butter4", "butter6", "butter8", "cheby4", "ellip4", "dcblock", "cpole")
COVERAGE_N = 8192
COVERAGE_BOUND = 2.5e-6                                   # a quarter of the float32 tolerance


def seam_lengths(d, nmax=None):
    """1, D - 1, D, the chunk seams of float32 (64) and float64 (32), the tile seams (4096 / 2048), three tiles and a rest"""
    ns = {1, max(d - 1, 1), d, 31, 32, 33, 63, 64, 65, 500, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 77}
    return sorted(n for n in ns if nmax is None or n <= nmax)


def exact_case(name, n, rows=3):
    """(x [rows, n], zi [rows, D]) of the integer filter `name`: integers in [-4, 4] on both planes"""
    b, a, _ = INT_FILTERS[name]
    return int_data((rows, n), n), int_data((rows, max(len(a), len(b)) - 1), n + 1)


def int_sos(name):
    return np.array([list(_BIQUADS[k][0]) + list(_BIQUADS[k][1]) for k in INT_CASCADES[name]], dtype=np.complex128)


def int_data(shape, seed, real=False):
    """integers in [-4, 4] on both planes: complex128"""
    rs = np.random.RandomState(seed)
    re = rs.randint(-4, 5, shape).astype(np.float64)
    return re + 0j if real else re + J * rs.randint(-4, 5, shape)


def gauss_data(shape, seed, real=False):
    rs = np.random.RandomState(seed)
    re = rs.randn(*shape)
    return re + 0j if real else re + J * rs.randn(*shape)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def _coefs(b, a, rows, dtype):
    b, a = np.atleast_2d(np.asarray(b, dtype=dtype)), np.atleast_2d(np.asarray(a, dtype=dtype))
    d = max(b.shape[-1], a.shape[-1]) - 1
    a0 = a[:, :1]
    full = lambda t: np.broadcast_to(np.pad(t / a0, ((0, 0), (0, d + 1 - t.shape[-1]))), (rows, d + 1)).astype(dtype)  # noqa: E731
    return full(b), full(a), d


def lfilter(b, a, x, zi=None, dtype=np.complex128, reverse=False, conj=False):
    """x [R, N]; b, a 1-d or [R, n] (normalised by a[..., 0] here); zi [R, D] or None -> (y [R, N], zf [R, D])"""
    x = np.asarray(x, dtype=dtype)
    rows, n = x.shape
    b, a, d = _coefs(b, a, rows, dtype)
    if conj:
        b, a = np.conj(b), np.conj(a)
    z = np.zeros((rows, d + 1), dtype=dtype)
    if zi is not None:
        z[:, :d] = np.broadcast_to(np.asarray(zi, dtype=dtype), (rows, d))
    xs = x[:, ::-1] if reverse else x
    y = np.zeros((rows, n), dtype=dtype)
    peak = 0.0
    for t in range(n):
        xn = xs[:, t]
        yn = b[:, 0] * xn + z[:, 0]
        z[:, :d] = b[:, 1:] * xn[:, None] - a[:, 1:] * yn[:, None] + z[:, 1:]
        y[:, t] = yn
        if d:
            peak = max(peak, np.abs(z.real).max(), np.abs(z.imag).max())
    lfilter.peak = peak                                   # the largest state plane entry of the last call
    return (y[:, ::-1] if reverse else y), z[:, :d].copy()


def sosfilt(sos, x, zi=None, dtype=np.complex128, reverse=False, conj=False):
    """sos [S, 6] (or [R, S, 6]); zi [R, S, 2] or None -> (y, zf [R, S, 2]); reverse also reverses the section order"""
    sos = np.asarray(sos, dtype=dtype)
    s_count = sos.shape[-2]
    order = range(s_count - 1, -1, -1) if reverse else range(s_count)
    y = np.asarray(x, dtype=dtype)
    zf = np.zeros((y.shape[0], s_count, 2), dtype=dtype)
    for s in order:
        y, zf[:, s] = lfilter(sos[..., s, :3], sos[..., s, 3:], y, None if zi is None else np.asarray(zi)[:, s], dtype,
                              reverse, conj)
    return y, zf


# ---- the emulation of the kernel (csrc/iir.hip), from the plan's numbers alone ---------------------------------------------
def table_gain(a, chunk=64):
    """the largest entry (per plane) of the chunk tables of a normalised denominator"""
    zir, m = _tables(np.asarray(a, dtype=np.complex128), chunk, np.complex128)
    return max(np.abs(t.real).max() for t in (zir, m)) + max(np.abs(t.imag).max() for t in (zir, m))


def _tables(a, chunk, dtype):
    """zero-input responses zir [D, chunk] and the chunk transition M (column j: the final state from the unit state e_j)"""
    d = len(a) - 1
    zir = np.zeros((d, chunk), dtype=dtype)
    m = np.zeros((d, d), dtype=dtype)
    for j in range(d):
        z = np.zeros(d + 1, dtype=dtype)
        z[j] = 1
        for q in range(chunk):
            y = z[0]
            zir[j, q] = y
            z[:d] = z[1:] - a[1:] * y
        m[:, j] = z[:d]
    return zir, m


def _tile(x, b, a, carry, chunk, zir, pw, dtype):
    """one section over one tile of `len(x)` samples, chunk-parallel -> (y, the carried state after the tile)"""
    d, cnt = len(a) - 1, len(x)
    nl = -(-cnt // chunk)
    xs = np.zeros((nl, chunk), dtype=dtype)
    xs.reshape(-1)[:cnt] = x
    nv = np.clip(cnt - np.arange(nl) * chunk, 0, chunk)
    z = np.zeros((nl, d + 1), dtype=dtype)
    z[0, :d] = carry                                      # lane 0 runs from the carried state
    ys = np.zeros((nl, chunk), dtype=dtype)
    for q in range(chunk):                                # 1. every lane its chunk, from zero state
        live = q < nv
        yn = b[0] * xs[:, q] + z[:, 0]
        new = b[None, 1:] * xs[:, q, None] - a[None, 1:] * yn[:, None] + z[:, 1:]
        z[live, :d] = new[live]
        ys[live, q] = yn[live]
    local = z[:, :d].copy()
    p = local.copy()
    for c in range(1, nl):                                # 2. the states at the chunk ends, in order: P_c = M P_{c-1} + s_c
        p[c] = np.array([local[c, i] + np.sum(pw[i, :] * p[c - 1]) for i in range(d)], dtype=dtype)
    for c in range(1, nl):                                # 3. the zero-input response of the entering state
        for q in range(nv[c]):
            ys[c, q] = ys[c, q] + np.sum(zir[:, q] * p[c - 1])
    last = nl - 1
    final = p[last]
    if last > 0 and nv[last] < chunk:                     # 4. a part chunk ends the tile
        e = np.zeros(d + 1, dtype=dtype)
        e[:d] = p[last - 1]
        for _ in range(nv[last]):
            y0 = e[0]
            e[:d] = e[1:] - a[1:] * y0
        final = local[last] + e[:d]
    return ys.reshape(-1)[:cnt], final.astype(dtype)


def _segment(x, secs, zi, chunk, tile, dtype):
    """the cascade over one segment, tile by tile -> (y, final states [S, D])"""
    d = len(secs[0][1]) - 1
    carry = np.zeros((len(secs), d), dtype=dtype) if zi is None else np.array(zi, dtype=dtype).reshape(len(secs), d)
    tabs = [_tables(a, chunk, dtype) for _, a in secs]
    y = np.zeros(len(x), dtype=dtype)
    for t0 in range(0, len(x), tile):
        cur = np.asarray(x[t0:t0 + tile], dtype=dtype)
        for s, (b, a) in enumerate(secs):
            cur, carry[s] = _tile(cur, b, a, carry[s], chunk, *tabs[s], dtype)
        y[t0:t0 + tile] = cur
    return y, carry


def emulate(x, secs, zi, plan, reverse=False, conj=False, dtype=np.complex64):
    """One row through the kernel's scheme with the numbers of `plan` (chunk, tile, segments, seg_len): secs is a list of
    normalised (b [D + 1], a [D + 1]); zi [S, D] or None -> (y [N], zf [S, D]).  More than one segment runs the split
    path's launches: segment-final states from zero state, the transition from unit states on null input, the scan, the
    run from the true entering states."""
    chunk, tile, segs, seg_len = plan["chunk"], plan["tile"], plan["segments"], plan["seg_len"]
    secs = [(np.asarray(b, dtype=dtype), np.asarray(a, dtype=dtype)) for b, a in secs]
    if conj:
        secs = [(np.conj(b), np.conj(a)) for b, a in secs]
    x = np.asarray(x, dtype=dtype)
    xs = x[::-1] if reverse else x
    n, s_count, d = len(xs), len(secs), len(secs[0][1]) - 1
    if segs == 1:
        y, zf = _segment(xs, secs, zi, chunk, tile, dtype)
        return (y[::-1] if reverse else y), zf
    w = s_count * d
    cut = [xs[k * seg_len:(k + 1) * seg_len] for k in range(segs)]
    z = [_segment(c, secs, None, chunk, tile, dtype)[1].reshape(w) for c in cut]
    m = np.zeros((w, w), dtype=dtype)                     # m[j]: the final state from the unit state e_j
    for j in range(w):
        unit = np.zeros(w, dtype=dtype)
        unit[j] = 1
        m[j] = _segment(np.zeros(seg_len, dtype=dtype), secs, unit.reshape(s_count, d), chunk, tile, dtype)[1].reshape(w)
    enter = [np.zeros(w, dtype=dtype) if zi is None else np.array(zi, dtype=dtype).reshape(w)]
    for k in range(segs - 1):
        enter.append(np.array([z[k][i] + np.sum(m[:, i] * enter[k]) for i in range(w)], dtype=dtype))
    out = [_segment(c, secs, e.reshape(s_count, d), chunk, tile, dtype) for c, e in zip(cut, enter)]
    y = np.concatenate([o[0] for o in out])
    return (y[::-1] if reverse else y), out[-1][1]


def pad_section(b, a, dtype=np.complex128):
    """(b, a) normalised and zero-padded to a common D + 1"""
    bb, aa, _ = _coefs(b, a, 1, dtype)
    return bb[0], aa[0]
