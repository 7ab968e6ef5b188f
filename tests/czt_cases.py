"""Shared cases, reference and bounds of the chirp-z tests (test_czt_host.py, test_gpu_czt.py).

Reference: the direct sum y = x K in complex128 ON THE CPU, from the float64 of the values the kernel was actually given
(for bf16 planes: of the rounded values), K[j, k] = exp(ln|w| jk - ln|a| j) cis(2 pi (w_turn jk - a_turn j)).  The phase
is reduced from the same turn fractions the kernel receives, with the integer jk and a residual-exact product (Dekker's
two-product: no fma on the host), and K is built in chunks over k of at most 64 MB.  For the two largest float32 cases the
reference is a complex128 `torch.fft` Bluestein on the CPU (`bluestein`), which test_czt_host.py validates against the
direct sum at n, m <= 1100.

Bounds.  float32: norm-wise 1e-5, the repository's float32 bound (fft_cases.F32_TOL).  bf16: per entry of each plane
2^-8 |ref| + 1e-5 max|ref| of that plane, as fft_cases; only a plane whose reference is identically zero (the imaginary
plane of a real input at n = 1), which has no scale of its own, takes the largest modulus of the complex reference.
float64: complex128 Bluestein itself drifts from the direct sum, so the bound is measured: 4 x
the largest norm-wise error of `bluestein` against `direct` over every float64 test size and contour, on the CPU (the
kernel does the same arithmetic in the same precision, in a different order).  The measured values are F64_DRIFT below
(and profiles/czt_parity.txt); tests/test_czt_host.py re-measures the small sizes and holds them to the table.
"""
import functools
import math

import torch

from fft_cases import F32_TOL, c128, gaussian, normwise  # noqa: F401  (shared with the GPU tests)

# (n, m): the smallest that reach every branch; M = 2^ceil(log2(n + m - 1)) >= 8
SHAPES = ((1, 1), (1, 5), (5, 1),           # M clamps to 8
          (3, 7),
          (100, 37), (37, 100),             # n > m, n < m
          (512, 513),                       # n + m - 1 = 1024: the last packed M
          (513, 513),                       # 1025: the first one-vector M = 2048
          (5000, 3193),                     # 8192: the last fused
          (5000, 3194),                     # the first workspace M = 2^14; four-step in float64
          (16384, 16385))                   # float32 only: M = 2^15, four-step
F32_ONLY = ((16384, 16385),)
BLUESTEIN_REF = ((5000, 3194), (16384, 16385))          # float32 cases whose reference is `bluestein`
CONTOURS = ("default", "zoom", "zoom_endpoint", "spiral_in", "spiral_out")
D_TEST = 4.7                                # the bound of the spirals' D: 3.6 (w) + 1.0 (a) = 4.6

# cplxamd_czt_plan at the seams: (n, m) -> (path, vectors per workgroup), the same for float32 and float64
PLAN = {(1, 1): ("packed", 256), (5, 4): ("packed", 256), (5, 5): ("packed", 128), (3, 7): ("packed", 128),
        (100, 37): ("packed", 8), (512, 513): ("packed", 2), (513, 513): ("fused", 1), (5000, 3193): ("fused", 1),
        (5000, 3194): ("workspace", 1), (16384, 16385): ("workspace", 1), (1 << 21, 1 << 21): ("workspace", 1)}

# norm-wise error of the complex128 Bluestein against the direct sum, the largest over CONTOURS, per float64 test shape
# (measured on the CPU by scripts/gen_czt_golden.py --drift; see profiles/czt_parity.txt)
F64_DRIFT = {(1, 1): 0.0, (1, 5): 4.21e-16, (5, 1): 3.85e-16, (3, 7): 5.92e-16, (100, 37): 1.33e-15, (37, 100): 1.43e-15,
             (512, 513): 2.24e-15, (513, 513): 1.69e-15, (5000, 3193): 2.59e-15, (5000, 3194): 1.83e-15}
F64_MARGIN = 4.0                            # the bound: 4 x 2.59e-15 = 1.04e-14


def f64_tol():
    return F64_MARGIN * max(F64_DRIFT.values())


def transform_size(n, m):
    M = 8
    while M < n + m - 1:
        M *= 2
    return M


def vectors_per_workgroup(n, m):
    M = transform_size(n, m)
    return 1 if M > 1024 else min(256, 2048 // M)


def vector_counts(n, m):
    """1 vector, and a partly filled last packed workgroup (V + 1) or 3 vectors for the unpacked sizes"""
    v = vectors_per_workgroup(n, m)
    return (1, v + 1 if v > 1 else 3)


def contour(name, n, m):
    """-> (kind, arguments): ("czt", (w, a)) with complex numbers (None: the default w), or ("zoom", (fn, fs, endpoint))"""
    if name == "default":
        return "czt", (None, 1 + 0j)
    if name == "zoom":                                    # f1 / fs = 0.1, band 0.2
        return "zoom", ((0.2, 0.6), 2.0, False)
    if name == "zoom_endpoint":
        return "zoom", ((0.2, 0.6), 2.0, True)
    sign = 1.0 if name == "spiral_in" else -1.0           # |w| > 1 and the points a w^-k spiral inwards
    w_log = sign * 2 * 3.6 / max(n, m) ** 2
    a_log = sign * 1.0 / n
    w = complex(math.exp(w_log)) * complex(math.cos(-2 * math.pi * 0.7 / m), math.sin(-2 * math.pi * 0.7 / m))
    a = complex(math.exp(a_log)) * complex(math.cos(2 * math.pi * 0.05), math.sin(2 * math.pi * 0.05))
    return "czt", (w, a)


def contour_params(name, n, m):
    """(w_log, w_turn, a_log, a_turn): what the kernel receives for contour `name` (the host layer's own mapping, which
    test_czt_host.py checks against scipy's numbers)"""
    from cplxmodule_amd import czt as C
    kind, args = contour(name, n, m)
    if kind == "zoom":
        fn, fs, endpoint = args
        if endpoint and m == 1:
            return None                                   # scipy divides by m - 1
        _, w_turn, a_turn = C.zoom_params(n, fn, m, fs, endpoint)
        return 0.0, w_turn, 0.0, a_turn
    w, a = args
    w_log, w_turn = (0.0, -1.0 / m) if w is None else C._polar(w, "w", "czt")
    return (w_log, w_turn) + C._polar(a, "a", "czt")


def apply(name, x, m):
    """the public call for contour `name`"""
    from cplxmodule_amd import cplx
    kind, args = contour(name, x.shape[-1], m)
    if kind == "zoom":
        fn, fs, endpoint = args
        return cplx.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)
    return cplx.czt(x, m, *args)


# ---- exact phases ------------------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def turns(theta, q):
    """theta q mod 1 (in [-1/2, 1/2] plus a residual) for a double theta and a float64 tensor q of integers below 2^53:
    the rounded product and its exact residual (Dekker) are reduced separately"""
    q = q.double()
    p = theta * q
    th, tl = _split(torch.tensor(theta, dtype=torch.float64))
    qh, ql = _split(q)
    r = ((th * qh - p) + th * ql + tl * qh) + tl * ql
    return (p - torch.round(p)) + r


def cis_turns(t):
    a = 2 * math.pi * t
    return torch.complex(torch.cos(a), torch.sin(a))


def direct(z, m, w_log, w_turn, a_log, a_turn, chunk_bytes=64 << 20):
    """y[..., k] = sum_j z[..., j] a^-j w^{jk} for complex128 z [..., n], as the dense product, chunked over k"""
    n = z.shape[-1]
    j = torch.arange(n, dtype=torch.int64)
    aj = torch.exp(-a_log * j.double()) * cis_turns(-turns(a_turn, j))
    za = z.to(torch.complex128) * aj
    step = max(1, chunk_bytes // (16 * n))
    out = []
    for k0 in range(0, m, step):
        k = torch.arange(k0, min(m, k0 + step), dtype=torch.int64)
        jk = j[:, None] * k[None, :]
        K = cis_turns(turns(w_turn, jk))
        if w_log != 0.0:
            K = K * torch.exp(w_log * jk.double())
        out.append(za @ K)
    return torch.cat(out, dim=-1)


def _chirp(idx, s, w_log, w_turn):
    """w^{s i^2 / 2} for the int64 tensor idx (w_turn / 2 is exact)"""
    q = idx * idx
    v = cis_turns(s * turns(w_turn * 0.5, q))
    return v * torch.exp(s * w_log * q.double() / 2) if w_log != 0.0 else v


def bluestein(z, m, w_log, w_turn, a_log, a_turn):
    """the same transform by Bluestein's convolution in complex128 `torch.fft` at 2^ceil(log2(n + m - 1)): the chirp-z
    algorithm itself, in the reference's precision"""
    n = z.shape[-1]
    M = transform_size(n, m)
    j, k = torch.arange(n, dtype=torch.int64), torch.arange(m, dtype=torch.int64)
    opening = _chirp(j, 1.0, w_log, w_turn) * torch.exp(-a_log * j.double()) * cis_turns(-turns(a_turn, j))
    closing = _chirp(k, 1.0, w_log, w_turn)
    b = torch.zeros(M, dtype=torch.complex128)
    b[:m] = _chirp(k, -1.0, w_log, w_turn)
    if n > 1:
        i = torch.arange(1, n, dtype=torch.int64)
        b[M - i] = _chirp(i, -1.0, w_log, w_turn)
    A = torch.fft.fft(z.to(torch.complex128) * opening, M, dim=-1)
    return torch.fft.ifft(A * torch.fft.fft(b), dim=-1)[..., :m] * closing


@functools.lru_cache(maxsize=None)
def case(n, m, dtype, name, seed=0):
    """(re, im, reference of re + i im, reference of re alone) of max(vector_counts) Gaussian vectors (a test of fewer
    vectors takes the leading rows) -- one dense product for both, computed once, shared and left unchanged; None when
    the contour does not exist at this shape (zoom_endpoint at m = 1)"""
    p = contour_params(name, n, m)
    if p is None:
        return None
    rows = max(vector_counts(n, m))
    re, im = gaussian((rows, n), dtype, seed + 31 * n + m)
    z = torch.cat([c128(re, im), c128(re, torch.zeros_like(re))])
    ref = bluestein(z, m, *p) if dtype == torch.float32 and (n, m) in BLUESTEIN_REF else direct(z, m, *p)
    return re, im, ref[:rows], ref[rows:]


def adjoint(g, n, w_log, w_turn, a_log, a_turn):
    """the adjoint of the transform applied to complex128 g [..., m]: dx[j] = conj(a)^-j sum_k g[k] conj(w)^{jk}, j < n"""
    j = torch.arange(n, dtype=torch.int64)
    return direct(g, n, w_log, -w_turn, 0.0, 0.0) * torch.exp(-a_log * j.double()) * cis_turns(turns(a_turn, j))


def bf16_plane_violations(got, ref):
    """fft_cases.bf16_violations -- entries of a bf16 plane of `got` outside 2^-8 |ref| + 1e-5 max|ref| of that plane, and
    the worst ratio -- except that a plane whose reference is identically zero takes the largest modulus of the complex
    reference as its max|ref|"""
    worst, bad = 0.0, 0
    for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
        top = float(r.abs().max()) or float(ref.abs().max())
        ratio = (g.detach().double().cpu() - r).abs() / (2.0 ** -8 * r.abs() + F32_TOL * top)
        worst = max(worst, float(ratio.max()))
        bad += int((ratio > 1).sum())
    return bad, worst


def spread(name, n, m):
    w_log, _, a_log, _ = contour_params(name, n, m)
    return abs(w_log) * max(n, m) ** 2 / 2 + abs(a_log) * n
