"""Shared fixtures of the short-time transform tests (test_stft_host.py, test_gpu_stft.py): case lists and cached inputs
with their references.  Reference and bounds are fft_cases.py's: `torch.stft` / `torch.istft` in float64 / complex128 ON THE
CPU, from the values the kernel was given; float32 1e-5 norm-wise, float64 1e-11, bf16 2^-8 |ref| + 1e-5 max|ref| per
entry.  Every istft case passes torch's NOLA check (test_stft_host.py runs them all through torch on the CPU): with
center=False the window has no small entry (0.5 + rand), because Hann's first sample is 0.
"""
import functools

import torch

import fft_cases as fc
import rfft_cases as rc

# every path of the underlying real transform: packed direct / Bluestein, odd lengths on the full transform, one vector
# per workgroup (4096), through the workspace (4097, 8194)
PATH_LENGTHS = (2, 3, 8, 16, 64, 100, 101, 400, 1024, 2048, 4096, 4097, 8194)
PLAN_LENGTHS = (2, 16, 64, 100, 400, 1024, 4096, 8194)

# (T, n_fft, hop) of the exhaustive index-map test
MAP_CASES = ((9, 16, 4), (50, 16, 4), (53, 16, 5), (50, 16, 1), (50, 16, 16), (50, 16, 20), (1, 1, 1))


def window(kind, win_length, seed=7):
    """float64 window on the CPU: None (rectangular), "hann" (periodic) or "rand" (0.5 + uniform: no small entry)"""
    if kind is None:
        return None
    if kind == "hann":
        return torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + win_length)
    return 0.5 + torch.rand(win_length, dtype=torch.float64, generator=g)


def _ones_if_none(win, n_fft, win_length):
    return torch.ones(win_length or n_fft, dtype=torch.float64) if win is None else win.double()


def ref_stft(x, n_fft, hop_length=None, win_length=None, window=None, **kw):
    """torch.stft in float64 on the CPU of the values of x [..., T] -> complex128 [..., N, frames]"""
    x = x.detach().double().cpu()
    lead = x.shape[:-1]
    out = torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop_length, win_length, _ones_if_none(window, n_fft, win_length),
                     return_complex=True, **kw)
    return out.reshape(*lead, *out.shape[-2:])


def ref_istft(re, im, n_fft, hop_length=None, win_length=None, window=None, **kw):
    """torch.istft in complex128 on the CPU of planes [..., N, frames] -> float64 [..., T]"""
    z = fc.c128(re, im)
    lead = z.shape[:-2]
    out = torch.istft(z.reshape(-1, *z.shape[-2:]), n_fft, hop_length, win_length, _ones_if_none(window, n_fft, win_length), **kw)
    return out.reshape(*lead, out.shape[-1])


def ref_stft_graph(x, n_fft, hop, win, **kw):
    """torch.stft of a float64 CPU tensor [..., T] that autograd follows"""
    lead = x.shape[:-1]
    out = torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop, kw.pop("win_length", None),
                     _ones_if_none(win, n_fft, None), return_complex=True, **kw)
    return out.reshape(*lead, *out.shape[-2:])


def ref_istft_graph(re, im, n_fft, hop, win, **kw):
    """torch.istft of float64 CPU planes [..., N, frames] that autograd follows"""
    z = torch.complex(re, im)
    lead = z.shape[:-2]
    out = torch.istft(z.reshape(-1, *z.shape[-2:]), n_fft, hop, None, _ones_if_none(win, n_fft, None), **kw)
    return out.reshape(*lead, out.shape[-1])


def path_geometry(n_fft):
    """(hop, T, rows) of the path cases: hop = max(1, n_fft // 4); 7 frames with center=True (8 at hop 1) and a ragged
    tail; 2 rows for an even n_fft, 3 for an odd one"""
    hop = max(1, n_fft // 4)
    return hop, 6 * hop + hop // 2 if hop > 1 else 7, 2 + n_fft % 2


@functools.lru_cache(maxsize=None)
def path_case(n_fft, dtype, seed=0):
    """(x, win, stft reference, Xr, Xi, istft reference) of the path case of n_fft -- computed once, shared, left
    unchanged.  The window is "rand": it passes NOLA for every hop <= n_fft."""
    hop, T, rows = path_geometry(n_fft)
    x = rc.real_gaussian((rows, T), dtype, seed + n_fft)
    win = window("rand", n_fft)
    S = ref_stft(x, n_fft, hop, window=win)
    xr, xi = rc.half_spectrum((rows, n_fft // 2 + 1, S.shape[-1]), dtype, seed + n_fft + 1)
    # (onesided=True is spelled out: at n_fft = 2 the half spectrum has n_fft entries and torch would take it for a full one)
    return x, win, S, xr, xi, ref_istft(xr, xi, n_fft, hop, window=win, onesided=True)


# framing seams, per n_fft in (16, 64): (label, T as a function of n_fft, stft / istft keywords, window kind, istft too?)
def seam_cases(n):
    return [
        ("ragged tail", 5 * n + 3, dict(hop_length=n // 4), "hann", True),
        ("hop 1", n + 9, dict(hop_length=1), "hann", True),
        ("hop n_fft", 4 * n + 5, dict(hop_length=n), "rand", True),
        ("hop beyond n_fft", 5 * n + 7, dict(hop_length=n + 4), "rand", False),
        ("shortest reflect", n // 2 + 1, dict(hop_length=n // 4), "hann", True),
        ("center=False", 4 * n + 3, dict(hop_length=n // 4, center=False), "rand", True),
        ("constant", 3 * n + 1, dict(hop_length=n // 4, pad_mode="constant"), "hann", True),
        ("replicate", 3 * n + 1, dict(hop_length=n // 4, pad_mode="replicate"), "hann", True),
        ("circular", 3 * n + 1, dict(hop_length=n // 4, pad_mode="circular"), "hann", True),
        ("win_length n_fft - 4", 3 * n + 2, dict(hop_length=n // 4, win_length=n - 4), "hann", True),
        ("odd win_length", 3 * n + 2, dict(hop_length=n // 8, win_length=n // 2 + 1), "hann", True),
        ("normalized", 3 * n + 2, dict(hop_length=n // 4, normalized=True), "hann", True),
        ("rectangular", 3 * n + 2, dict(hop_length=n // 2), None, True),
    ]


def istft_kwargs(kw):
    """the keywords of a stft case that istft takes too"""
    return {k: v for k, v in kw.items() if k != "pad_mode"}


# (T, n_fft, hop, win_length, center, onesided, length) of the shape test
SHAPE_CASES = [
    (100, 16, None, None, True, True, None), (100, 16, 4, None, True, True, None), (103, 16, 5, None, True, True, 90),
    (103, 16, 5, None, True, True, 120), (103, 16, 5, 12, True, True, 100), (64, 16, 16, None, False, True, None), (70, 17, 3, 9, True, True, 40),
    (9, 16, 4, None, True, True, None), (1, 1, 1, None, False, True, None), (1, 1, 1, None, True, True, 1), (200, 100, 25, None, True, True, 180),
]
