"""Shared fixtures of the cplx.upfirdn / cplx.resample_poly tests (test_upfirdn_host.py, test_gpu_upfirdn.py): case
lists, the naive numpy oracle of both primitives, the numpy emulation of the kernels' tile geometry, the filter design and
the bounds.

Oracle: the definitions as loops in complex128 (xu is x upsampled by `up`, zero elsewhere and outside the row):
    P1 conv  y[n] = sum_k h[k] xu[n down + off - k]          P1 corr  y[n] = sum_k conj(h[k]) xu[n down + off + k]
    P2       y[k] = sum_n conj(au[n down + off - k]) c[n]
Bounds: fft_cases.py's (float32 norm-wise 1e-5, float64 1e-11, bf16 per entry 2^-8 |ref| + 1e-5 max|ref| with no violation
allowed; the bf16 reference is formed from the rounded inputs).
"""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upfirdn_scipy.npz")

RATES = [(1, 1), (1, 2), (2, 1), (3, 2), (2, 3), (7, 5), (4, 6), (160, 147)]
# the small cases of the golden file: scipy.signal.upfirdn (N, K, up, down) and resample_poly (N, up, down)
GOLDEN_UPFIRDN = [(50, 7, 1, 1), (50, 7, 1, 2), (37, 5, 2, 1), (50, 11, 3, 2), (37, 9, 2, 3), (41, 13, 7, 5), (23, 8, 4, 6),
                  (20, 300, 160, 147), (1, 4, 3, 2), (9, 1, 5, 4)]
GOLDEN_RESAMPLE = [(50, 3, 2), (37, 2, 3), (64, 160, 147), (100, 1, 4), (11, 5, 1), (23, 4, 6), (1, 3, 2)]
GOLDEN_WINDOW = [(40, 3, 2, 12), (40, 2, 5, 31)]          # resample_poly with an array of K taps: (N, up, down, K)
GOLDEN_FIRWIN = [(3, 2), (2, 3), (160, 147), (1, 4), (5, 1)]

# ---- the plan: (N, K, up, down, dtype, x complex, h complex) -> (T, tiles, tiles per workgroup, span, jseg, segs) ---------
# The rule: T = min(1024, length), halved (in multiples of 64) down to 64 while the staged span
# ((T - 1) down + up - 1) / up + ceil(K / up) and the min(up, K) ceil(K / up) taps exceed 76 KiB; rows of one tile are packed.
PLAN_TABLE = {
    (65536, 3201, 160, 147, "f32", True, False): (1024, 70, 1, 961, 21, 1),     # the 160/147 conversion of the benchmark
    (65536, 161, 1, 8, "f32", True, False): (1024, 9, 1, 8345, 161, 1),         # decimation by 8: 70 KiB of samples
    (65536, 1281, 1, 64, "f32", True, False): (64, 17, 1, 5313, 1281, 1),        # a heavy decimation: a smaller tile
    (65536, 1281, 1, 64, "f64", True, True): (64, 17, 1, 4304, 272, 5),          # ... and, in float64, segments
    (65536, 81, 4, 1, "f32", True, False): (1024, 257, 1, 277, 21, 1),          # interpolation by 4
    (100, 21, 3, 2, "f32", True, True): (159, 1, 4, 113, 7, 1),                 # short rows: packed (4 rows given)
    (4096, 4096, 1, 1, "f64", True, True): (64, 128, 1, 2319, 2256, 2),          # the longest fused filter in float64
}

# the geometry emulation (host): K relative to up, N at the tile seam
def geometry_cases():
    out = []
    for up, down in RATES:
        for k in sorted({1, max(up - 1, 1), up, up + 1, 2 * up + 3}):
            for n in (1, 2, 29):
                out.append((n, k, up, down))
    return out


def length_upfirdn(n, k, up, down):
    return -(-((n - 1) * up + k) // down)


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def p1(x, h, up, down, off, length, conj=False):
    """P1 by its definition, one row: complex128 [length]"""
    x, h = np.asarray(x, dtype=np.complex128), np.asarray(h, dtype=np.complex128)
    y = np.zeros(length, dtype=np.complex128)
    k = np.arange(len(h))
    taps = np.conj(h) if conj else h
    for n in range(length):
        m = n * down + off + (k if conj else -k)          # the index into xu per tap
        i = m // up
        ok = (m % up == 0) & (i >= 0) & (i < len(x))
        y[n] = np.sum(taps[ok] * x[i[ok]])
    return y


def p2(a, c, up, down, off, k_taps):
    """P2 by its definition, one row: complex128 [k_taps]"""
    a, c = np.asarray(a, dtype=np.complex128), np.asarray(c, dtype=np.complex128)
    y = np.zeros(k_taps, dtype=np.complex128)
    n = np.arange(len(c))
    for k in range(k_taps):
        m = n * down + off - k
        i = m // up
        ok = (m % up == 0) & (i >= 0) & (i < len(a))
        y[k] = np.sum(np.conj(a[i[ok]]) * c[ok])
    return y


def rows_p1(x, h, up, down, off, length, conj=False):
    """P1 over 2-d x [R, N] with h [K] or [R, K] -> complex128 tensor [R, length]"""
    x, h = np.asarray(x), np.asarray(h)
    return torch.from_numpy(np.stack([p1(x[r], h if h.ndim == 1 else h[r], up, down, off, length, conj) for r in range(len(x))]))


def pad(i):
    return i + (i >> 4)


def emulate_p1(x, h, up, down, off, length, conj, p):
    """P1 exactly as the plan `p` lays it out, from its numbers alone: per tile and segment a span of x from ibase (zero
    outside the row) and the taps (j0 + j) up + ph at pad(ph jseg + j); every LDS index is checked against the planes'
    sizes, every output is written exactly once."""
    x, h = np.asarray(x, dtype=np.complex128), np.asarray(h, dtype=np.complex128)
    n_x, k_taps = len(x), len(h)
    T, span, phases, jseg, segs = p["T"], p["span"], p["phases"], p["jseg"], p["segs"]
    assert phases == min(up, k_taps) and segs == -(-(-(-k_taps // up)) // jseg) and p["tiles"] == -(-length // T)
    y = np.full(length, np.nan, dtype=np.complex128)
    for jt in range(p["tiles"]):
        n0 = jt * T
        left = min(T, length - n0)
        q0 = n0 * down + off
        if conj:
            i0 = -((-q0) // up)
            c0 = up - 1 - (i0 * up - q0)
        else:
            i0 = q0 // up
            c0 = q0 - i0 * up
        assert 0 <= c0 < up
        acc = np.zeros(left, dtype=np.complex128)
        for seg in range(segs):
            j0 = seg * jseg
            ibase = i0 + j0 if conj else i0 - (j0 + jseg - 1)
            xs = np.zeros(pad(span) + 1, dtype=np.complex128)
            for s in range(span):
                if 0 <= ibase + s < n_x:
                    xs[pad(s)] = x[ibase + s]
            hs = np.zeros(pad(phases * jseg) + 1, dtype=np.complex128)
            for e in range(phases * jseg):
                j, ph = divmod(e, phases)
                k = (j0 + j) * up + ph
                if k < k_taps:
                    hs[pad(ph * jseg + j)] = np.conj(h[k]) if conj else h[k]
            for m in range(left):
                di, rem = divmod(m * down + c0, up)
                ph = up - 1 - rem if conj else rem
                if ph >= k_taps:
                    continue
                jp = (k_taps - ph + up - 1) // up
                j = np.arange(j0, min(j0 + jseg, jp))     # ascending, as the kernel walks them
                if not len(j):
                    continue
                sx = di + (j - j0) if conj else di + jseg - 1 - (j - j0)
                at = ph * jseg + j - j0
                assert sx.min() >= 0 and sx.max() < span and at.min() >= 0 and at.max() < phases * jseg, "an LDS index outside its plane"
                acc[m] += np.sum(hs[at + (at >> 4)] * xs[sx + (sx >> 4)])
        assert not np.isfinite(y[n0:n0 + left]).any(), "an output written twice"
        y[n0:n0 + left] = acc
    assert np.isfinite(y).all(), "an output never written"
    return y


def emulate_p2(a, c, up, down, off, k_taps, p):
    """P2 as the plan lays it out: blocks of kb taps, tiles of Tn entries of c, a span of a from ibase; per tap the n of
    its residue class modulo up / g, stepped by up / g (and i by down / g); the span index is checked"""
    a, c = np.asarray(a, dtype=np.complex128), np.asarray(c, dtype=np.complex128)
    Tn, span, kb = p["wgrad_Tn"], p["wgrad_span"], p["wgrad_kb"]
    g = int(np.gcd(up, down))
    upg, downg = up // g, down // g
    inv = pow(downg, -1, upg) if upg > 1 else 0
    y = np.zeros(k_taps, dtype=np.complex128)
    assert p["wgrad_tiles"] == -(-len(c) // Tn) and p["wgrad_kblocks"] == -(-k_taps // kb)
    for kbi in range(p["wgrad_kblocks"]):
        k0, k1 = kbi * kb, min(k_taps, kbi * kb + kb)
        for jt in range(p["wgrad_tiles"]):
            n_lo = jt * Tn
            cnt = min(Tn, len(c) - n_lo)
            ibase = -((-(n_lo * down + off - (k1 - 1))) // up)
            for k in range(k0, k1):
                r = k - off
                if r % g:
                    continue
                nk = ((r // g) % upg) * inv % upg
                ik = (nk * down - r) // up
                assert ik * up == nk * down - r
                nq, nr = divmod(n_lo, upg)
                z = nq + (1 if nk < nr else 0)
                m, s = z * upg + nk - n_lo, ik + z * downg - ibase
                assert 0 <= m < upg
                ms = np.arange(m, cnt, upg)
                if not len(ms):
                    continue
                ss = s + downg * np.arange(len(ms))
                assert ss.min() >= 0 and ss.max() < span, "the span of a does not hold a sample the tile meets"
                ok = (ibase + ss >= 0) & (ibase + ss < len(a))
                y[k] += np.sum(np.conj(a[ibase + ss[ok]]) * c[n_lo + ms[ok]])
    return y


# ---- the filter design --------------------------------------------------------------------------------------------------
def design(up, down, beta=5.0):
    """resample_poly's default filter for reduced rates, in numpy float64: fc sinc(fc (n - half)) kaiser, sum = up"""
    half = 10 * max(up, down)
    fc = 1.0 / max(up, down)
    h = fc * np.sinc(fc * (np.arange(2 * half + 1) - half)) * np.kaiser(2 * half + 1, beta)
    return h * (up / h.sum())


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_input(n, seed, cplx=True):
    """the inputs of the golden cases: reproducible without the file's generator"""
    rng = np.random.default_rng(seed)
    re = rng.standard_normal(n)
    return re + 1j * rng.standard_normal(n) if cplx else re


# ---- values --------------------------------------------------------------------------------------------------------------
def integers(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def gaussian(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.float64, generator=g).to(dtype)


def c128(x):
    """a Cplx, a pair of planes (the second may be None) or a real tensor -> complex128 on the CPU"""
    if torch.is_tensor(x):
        re, im = x, None
    elif isinstance(x, tuple):
        re, im = x
    else:
        re, im = x.real, x.imag
    re = re.detach().double().cpu()
    return torch.complex(re, torch.zeros_like(re) if im is None else im.detach().double().cpu())


# integer cases of the GPU tests: (rows, N, K, up, down).  Tiles hold 1024 outputs: the lengths below give 1023, 1024 and
# 1025 outputs (the tile seam) for the rates of RATES; rows of one tile are packed 1024 // length to a workgroup
def exact_cases():
    out = []
    for up, down in RATES:
        k = up + 2 if up < 100 else 2 * up + 5
        for length in (1023, 1024, 1025):
            # the least N whose output count reaches `length`, then trimmed by the check below
            n = max(1, -(-(length * down - k) // up) + 1)
            while length_upfirdn(n, k, up, down) > length and n > 1:
                n -= 1
            if length_upfirdn(n, k, up, down) == length:
                out.append((2, n, k, up, down))
    return out


# packed rows: 100 outputs per row -> T = 100, 10 rows per workgroup: 9, 10, 11 rows; and 2 workgroups + 1 row
PACKED = [(rows, 66, 4, 3, 2) for rows in (9, 10, 11, 21)]


@functools.lru_cache(maxsize=None)
def exact_case(rows, n, k, seed=0):
    """integer planes (xr, xi, hr, hi) in float64 on the CPU: x [rows, N], h [K] -- computed once, left unchanged"""
    s = seed + 7 * n + k
    return (integers((rows, n), s), integers((rows, n), s + 1), integers((k,), s + 2), integers((k,), s + 3))


def partial_sum_bound(terms, amax=4):
    """the largest magnitude a sum of `terms` complex products of integers up to amax can reach"""
    return 2 * terms * amax * amax
