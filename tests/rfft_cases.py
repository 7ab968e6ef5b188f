"""Shared fixtures of the real-transform tests (test_rfft_host.py, test_gpu_rfft.py): case lists and cached inputs with
their references.  Reference and bounds are fft_cases.py's: `torch.fft` in complex128 / float64 ON THE CPU, from the values
the kernel was given; float32 1e-5 norm-wise, float64 1e-11, bf16 2^-8 |ref| + 1e-5 max|ref| per entry.
"""
import functools

import torch

import fft_cases as fc

# every path of the half-length route: packed direct / Bluestein (2 .. 2048), odd lengths on the full transform, one
# vector per workgroup (4096, 16384, 32768 in float32), through the workspace (4097, 8194, 65536; 32768 in float64)
PATH_LENGTHS = (2, 3, 5, 6, 8, 16, 64, 100, 101, 200, 224, 1000, 1024, 2000, 2048, 4096, 4097, 8194, 16384, 32768, 65536)

# cplxamd_rfft_plan: n -> (path for float32, path for float64, length of the complex transform, points run)
PLAN = {
    2: ("direct", "direct", 1, 1), 64: ("direct", "direct", 32, 32), 2048: ("direct", "direct", 1024, 1024),
    4096: ("direct", "direct", 2048, 2048), 200: ("bluestein", "bluestein", 100, 256),
    224: ("bluestein", "bluestein", 112, 256), 32768: ("direct", "four-step", 16384, 16384),
    8194: ("bluestein+four-step", "bluestein+four-step", 4097, 16384), 1 << 22: ("four-step", "four-step", 1 << 21, 1 << 21),
    1: ("direct", "direct", 1, 1), 3: ("bluestein", "bluestein", 3, 8), 101: ("bluestein", "bluestein", 101, 256),
}


def complex_length(n):
    """an even real length runs a complex transform of half the length, an odd one of the full length"""
    return n // 2 if n % 2 == 0 else n


def real_gaussian(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=torch.float64, generator=g).to(dtype)


def half_spectrum(shape, dtype, seed):
    """planes of a random half spectrum: the DC and Nyquist imaginary parts are NOT zero (the kernels must ignore them)"""
    return fc.gaussian(shape, dtype, seed)


@functools.lru_cache(maxsize=None)
def path_case(n, vectors, dtype, seed=0):
    """(x, rfft reference, Xr, Xi, irfft reference scaled by n) of `vectors` vectors of real length n -- computed once,
    shared and left unchanged"""
    x = real_gaussian((vectors, n), dtype, seed + n)
    xr, xi = half_spectrum((vectors, n // 2 + 1), dtype, seed + n + 1)
    return (x, torch.fft.rfft(x.double(), dim=-1), xr, xi, torch.fft.irfft(fc.c128(xr, xi), n=n, dim=-1, norm="forward"))


def real_normwise(got, ref):
    """norm-wise relative error of a real tensor against a float64 reference"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = torch.linalg.norm(ref.reshape(-1))
    return float(torch.linalg.norm((got - ref).reshape(-1)) / (den if den > 0 else 1.0))


def bf16_real_violations(got, ref):
    """entries of a bf16 real tensor outside 2^-8 |ref| + 1e-5 max|ref|; and the worst ratio"""
    bound = 2.0 ** -8 * ref.abs() + fc.F32_TOL * ref.abs().max()
    ratio = (got.detach().double().cpu() - ref).abs() / bound
    return int((ratio > 1).sum()), float(ratio.max())
