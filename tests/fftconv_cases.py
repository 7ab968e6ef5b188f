"""Shared fixtures of the cplx.fftconvolve tests (test_fftconv_host.py, test_gpu_fftconv.py): case lists, references, the
numpy emulation of the kernels' overlap-save geometry and the bounds.

Reference: the full convolution in complex128 ON THE CPU by `torch.fft` at the exact length N + M - 1, from the float64 of
the values the kernel was actually given (for bf16 planes: of the rounded values), sliced by `mode`; for the integer
cases `numpy.convolve`.  Bounds: fft_cases.py's (float32 norm-wise 1e-5, float64 1e-11, bf16 per entry 2^-8 |ref| + 1e-5
max|ref| with no violation allowed).
"""
import functools

import numpy as np
import torch

MODES = ("full", "same", "valid")

# ---- the plan: (A, K, window) -> what cplxamd_fftconv_plan must answer ---------------------------------------------------
# The rule: L = the smallest power of two >= 4 K, at least 512, at most the power of two that holds
# min(A, length) + K - 1 and at most 8192; S = L - K + 1.  One block per row when L >= A + K - 1 and the window lies inside.
# (A, K, mode) -> (path, L, S, blocks per row, blocks per workgroup)
PLAN_TABLE = {
    (100, 1, "full"): ("fused", 128, 128, 1, 16),          # K = 1: a scaling, every entry of a block is an output
    (64, 64, "full"): ("fused", 128, 65, 1, 16),           # K = A in a single block of >= 2 A - 1 points
    (4096, 4096, "full"): ("fused", 8192, 4097, 1, 1),     # K = A = 4096: the largest fused filter, one 8192-point block
    (20000, 4096, "full"): ("fused", 8192, 4097, 6, 1),    # K = 4096: half of a block is overlap
    (20000, 4097, "full"): ("composed", 32768, 0, 0, 0),   # K = 4097: composed at 2^ceil(log2(A + K - 1))
    (100, 7, "full"): ("fused", 128, 122, 1, 16),          # a single block
    (1000, 33, "full"): ("fused", 512, 480, 3, 4),         # the shortest block the plan picks: four per workgroup
    (5000, 255, "full"): ("fused", 1024, 770, 7, 2),       # L = 4 K rounded up: the last packed length
    (5000, 257, "full"): ("fused", 2048, 1792, 3, 1),      # ... and the first with one block per workgroup
    (20000, 512, "same"): ("fused", 2048, 1537, 14, 1),
    (20000, 2048, "valid"): ("fused", 8192, 6145, 3, 1),
    (300, 5, "valid"): ("fused", 512, 508, 1, 4),          # the window caps L: 296 outputs + 4
    (5, 2, "full"): ("fused", 8, 7, 1, 256),               # below 8 points: one thread per block, 256 per workgroup
}

# every (N, M) of the geometry emulation (host) -- all modes, both operand orders
GEOMETRY = [(1, 1), (5, 1), (5, 2), (6, 3), (9, 4), (100, 7), (772, 2), (1000, 33), (479, 33), (480, 33), (481, 33), (959, 33),
            (960, 33), (961, 33), (5000, 255), (5000, 257), (4096, 4096), (9000, 4096), (64, 64), (300, 6)]
# the seams of the block stride for K = 33: L = 512, S = 480
SEAMS_K = 33
SEAMS_A = [479, 480, 481, 959, 960, 961]


def window(n, m, mode):
    """(start, length) of `mode` within the full convolution of N and M entries"""
    if mode == "full":
        return 0, n + m - 1
    if mode == "same":
        return (m - 1) // 2, n
    return min(n, m) - 1, max(n, m) - min(n, m) + 1


def emulate(a, b, start, length, conj, p):
    """P1 by overlap-save exactly as the plan `p` lays it out, in numpy (complex128): block j loads a[j S + in_shift + i],
    i < L (zero outside the row), its cyclic convolution with b (correlation: with conj(b), the other way round) is taken
    by FFT, and entry i goes to y[j S + ((i - out_lo) mod L)] where that is below min(n_valid, length - j S)."""
    L, S = p["L"], p["S"]
    H = np.fft.fft(np.concatenate([b, np.zeros(L - len(b))]).astype(np.complex128))
    if conj:
        H = np.conj(H)
    y = np.full(length, np.nan, dtype=np.complex128)
    for j in range(p["blocks"]):
        idx = j * S + p["in_shift"] + np.arange(L)
        ok = (idx >= 0) & (idx < len(a))
        x = np.where(ok, a[np.clip(idx, 0, len(a) - 1)], 0).astype(np.complex128)
        z = np.fft.ifft(np.fft.fft(x) * H)
        n = (np.arange(L) - p["out_lo"]) % L
        keep = n < min(p["n_valid"], length - j * S)
        assert not np.isfinite(y[j * S + n[keep]]).any(), "an output written twice"
        y[j * S + n[keep]] = z[keep]
    assert np.isfinite(y).all(), "an output never written"
    return y


def direct(a, b, start, length, conj):
    """P1 by its definition: y[n] = sum_m a[n + start - m] b[m], or sum_m a[n + start + m] conj(b[m])"""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    if conj:
        full = np.correlate(a, b, "full")                  # lag q at index q + K - 1
        off = len(b) - 1
    else:
        full = np.convolve(a, b)
        off = 0
    y = np.zeros(length, dtype=np.complex128)
    for n in range(length):
        q = n + start + off
        if 0 <= q < len(full):
            y[n] = full[q]
    return y


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


def reference(x, h, mode):
    """the convolution of complex128 tensors along the last dim (leading dims broadcast), sliced by `mode`"""
    n, m = x.shape[-1], h.shape[-1]
    full = torch.fft.ifft(torch.fft.fft(x, n + m - 1) * torch.fft.fft(h, n + m - 1))
    start, length = window(n, m, mode)
    return full[..., start:start + length]


def integer_reference(x, h, mode):
    """numpy.convolve row by row (2-d x, 1-d or 2-d h), sliced by `mode` -> complex128 tensor"""
    x, h = x.numpy(), h.numpy()
    rows = []
    for r in range(x.shape[0]):
        rows.append(np.convolve(x[r], h if h.ndim == 1 else h[r]))
    start, length = window(x.shape[-1], h.shape[-1], mode)
    return torch.from_numpy(np.stack(rows)[:, start:start + length])


# integer cases: (rows, A, K); log_l = 2, so L = 4 and every twiddle is +-1 or +-i.  772 = 3 * 258 - 2: 258 blocks per row
# at S = 3 (K = 2), 256 blocks per workgroup, so both workgroup boundaries fall inside a row and the last is partly filled
EXACT_LOG_L = 2
EXACT = [(1, 9, 1), (2, 9, 2), (2, 10, 3), (3, 11, 4), (3, 772, 2)]
# V - 1, V, V + 1 blocks in all at L = 4 (V = 256), K = 2, S = 3, full: blocks = ceil((A + 1) / 3)
EXACT_BLOCKS = [(1, 3 * 255 - 1, 2), (1, 3 * 256 - 1, 2), (1, 3 * 257 - 1, 2)]


@functools.lru_cache(maxsize=None)
def exact_case(rows, a_len, k, seed=0):
    """integer planes (xr, xi, hr, hi) in float64 on the CPU: x [rows, A], h [K] -- computed once, left unchanged"""
    s = seed + 7 * a_len + k
    return (integers((rows, a_len), s), integers((rows, a_len), s + 1), integers((k,), s + 2), integers((k,), s + 3))


def partial_sum_bound(blocks, L, amax=4):
    """the largest magnitude any intermediate of an integer case can reach: a spectrum entry is at most L max, a product
    of spectra L^2 max^2 (times 2 for the complex product), summed over at most `blocks` blocks in the weight gradient"""
    return 2 * blocks * L * L * amax * amax
