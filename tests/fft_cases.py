"""Shared fixtures of the Fourier-transform tests (test_fft_host.py, test_gpu_fft.py): case lists, the reference and the
bounds.

Reference: `torch.fft` in complex128 ON THE CPU, from the float64 of the values the kernel was actually given (for bf16
planes: of the rounded values).  Bounds: float32 norm-wise 1e-5 (the repository's float32 bound, what
test_gpu_spectrum.py asserts for |X|^2 on the same paths), float64 1e-11; bf16 per entry 2^-8 |ref| (half a bf16 ulp, the
most ONE rounding costs) + 1e-5 max|ref| (the float32 bound).
"""
import functools

import torch

F32_TOL, F64_TOL = 1e-5, 1e-11

# every path: packed direct / Bluestein, one vector per workgroup, through the workspace (four-step and Bluestein on it)
PATH_LENGTHS = (3, 5, 8, 64, 100, 512, 1000, 1024, 2048, 4097, 8192, 16384, 16385, 32768)
# cplxamd_fft_plan: n -> (path for float32, path for float64); float64's LDS limit is 8192 points
PLAN_PATHS = {1: ("direct", "direct"), 4: ("direct", "direct"), 1000: ("bluestein", "bluestein"),
              1024: ("direct", "direct"), 2048: ("direct", "direct"),
              4097: ("bluestein+four-step", "bluestein+four-step"), 8192: ("direct", "direct"),
              16384: ("direct", "four-step"), 16385: ("bluestein+four-step", "bluestein+four-step"),
              32768: ("four-step", "four-step"), 1 << 22: ("four-step", "four-step")}


def transform_size(n):
    """M: n for a power of two, else Bluestein's 2^ceil(log2(2n - 1))"""
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def vectors_per_workgroup(n):
    """what the packed kernel transforms per 256-thread workgroup: 2048 / M, 256 for M < 8 (one thread per vector), 1
    for the sizes that are not packed"""
    m = transform_size(n)
    return 1 if m > 1024 else min(256, 2048 // m)


def gaussian(shape, dtype, seed):
    """planes (re, im) on the CPU, rounded to `dtype`"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, dtype=torch.float64, generator=g).to(dtype),
            torch.randn(*shape, dtype=torch.float64, generator=g).to(dtype))


def integers(shape, dtype, seed, lo=-8, hi=8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi + 1, shape, generator=g).to(dtype), torch.randint(lo, hi + 1, shape, generator=g).to(dtype))


def c128(re, im):
    return torch.complex(re.detach().double().cpu(), im.detach().double().cpu())


def reference(re, im, fn, *args, **kwargs):
    """torch.fft.<fn> in complex128 on the CPU of the planes' values"""
    return getattr(torch.fft, fn)(c128(re, im), *args, **kwargs)


@functools.lru_cache(maxsize=None)
def path_case(n, vectors, dtype, seed=0):
    """(re, im, forward reference, inverse reference) of `vectors` Gaussian vectors of length n -- computed once, shared
    and left unchanged"""
    re, im = gaussian((vectors, n), dtype, seed + n)
    z = c128(re, im)
    return re, im, torch.fft.fft(z, dim=-1), torch.fft.ifft(z, dim=-1, norm="forward")


def normwise(got, ref):
    """norm-wise relative error of a Cplx (or a complex tensor) against a complex128 reference"""
    if not torch.is_tensor(got):
        got = c128(got.real, got.imag)
    got = got.detach().to(torch.complex128).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = torch.linalg.norm(ref.reshape(-1))
    return float(torch.linalg.norm((got - ref).reshape(-1)) / (den if den > 0 else 1.0))


def tol(dtype):
    return F64_TOL if dtype == torch.float64 else F32_TOL


def bf16_violations(got, ref):
    """entries of the bf16 planes of `got` outside 2^-8 |ref| + 1e-5 max|ref|, per plane; and the worst ratio"""
    worst, bad = 0.0, 0
    for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
        g = g.detach().double().cpu()
        bound = 2.0 ** -8 * r.abs() + F32_TOL * r.abs().max()
        ratio = (g - r).abs() / bound
        worst = max(worst, float(ratio.max()))
        bad += int((ratio > 1).sum())
    return bad, worst
