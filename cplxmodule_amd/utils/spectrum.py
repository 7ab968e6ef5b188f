"""Welch spectra, band power and ACPR (cplxmodule/utils/spectrum.py): pwelch, fftshift, bandwidth_power, acpr_calc.

pwelch runs on the fused HIP FFT kernels of csrc/spectrum.hip (cplxmodule_amd/spectrum.py); fftshift, the band sums and
the decibels are plane-wise torch plumbing.  Accepted inputs: torch complex64 / complex128 device tensors, `[..., T, 2]`
real device tensors (bandwidth_power and acpr_calc, as in the reference), and the package's `Cplx` with float32,
bfloat16 or float64 planes -- bf16 planes are read as bf16, computed in float32 and give float32 results (frequencies
included).  Deviations from the reference: CPU tensors raise CplxAmdError (no host path), and so does a window that
requires grad (no gradient with respect to the window).  Nothing synchronises with the device: the frequencies are
formed on the device and the band edges become bin ranges on the host from fs and n alone, so pwelch, bandwidth_power
and acpr_calc can be captured in a hipGraph.
"""
import numpy as np
import torch

from .. import spectrum as _sp
from ..cplx import Cplx
from .views import fix_dim

__all__ = ["pwelch", "fftshift", "bandwidth_power", "acpr_calc"]


def _planes(x):
    if isinstance(x, Cplx):
        return x.real, x.imag
    xv = torch.view_as_real(x.resolve_conj())
    return xv[..., 0], xv[..., 1]


def _fftfreq(n, fs, dtype, device):
    """np.fft.fftfreq(n, 1 / fs) as a `dtype` tensor formed on the device (numpy's float64 products, then rounded)"""
    k = torch.arange(n, dtype=torch.int64, device=device)
    k = torch.where(k < (n - 1) // 2 + 1, k, k - n)
    return (k.to(torch.float64) * (1.0 / (n * (1.0 / fs)))).to(dtype)


def _band_bins(n, fs, bands, dtype=torch.float64):
    """[(a, b)] per band (lo, hi): the bins a .. b - 1 of fftshift(fftfreq(n, 1 / fs)) in `dtype` that lie in the open
    interval (lo, hi), compared in `dtype` as torch compares a tensor with a Python number.  The reference selects them
    with torch.nonzero on the device; the shifted frequencies increase, so every selection is one contiguous range."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    k = np.arange(n)
    ff = np.roll((np.where(k < (n - 1) // 2 + 1, k, k - n) * (1.0 / (n * (1.0 / fs)))).astype(npd), n // 2)
    out = []
    for lo, hi in bands:
        sel = np.flatnonzero((ff > npd(lo)) & (ff < npd(hi)))
        out.append((int(sel[0]), int(sel[-1]) + 1) if sel.size else (0, 0))
    return out


def _welch(pr, pi, ndim, dim, window, fs, scaling, n_overlap):
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"Unrecognized `scaling` value {scaling}")
    dim = fix_dim(dim, ndim)
    n_window = len(window)
    if n_overlap is None:
        n_overlap = n_window // 2
    assert n_window > n_overlap
    # the errors of the reference's window_view(x, dim, n_window, n_window - n_overlap, at=-1)
    if n_window <= 0:
        raise ValueError("`size` must be a positive integer.")
    if pr.shape[dim] < n_window:
        raise ValueError(f"`x` at dim {dim} is too short ({pr.shape[dim]}) for this window size ({n_window}).")
    if not isinstance(window, torch.Tensor):
        window = torch.as_tensor(np.asarray(window), device=pr.device)
    fdt = _sp.compute_dtype(pr.dtype)                     # the frequencies keep x's real dtype, as in the reference
    pxx = _sp.welch(pr, pi, dim, window, fs, scaling, n_window - n_overlap)
    return _fftfreq(n_window, fs, fdt, pxx.device), pxx


def pwelch(x, dim, window, fs=1.0, scaling="density", n_overlap=None):
    r"""Power spectral density (or power spectrum) by Welch's method, as scipy.signal.welch with nfft=None,
    nperseg=None, detrend=False, return_onesided=False.

    x: complex device tensor or Cplx; dim: the time axis; window: 1-d tensor on x's device whose length is the segment
    length n; n_overlap: samples shared by consecutive segments (default n // 2).
    Returns (f, Pxx): the n fftfreq frequencies in x's real dtype and Pxx of shape x.shape without dim, n appended.
    Pxx has the dtype the reference's x * window promotes to: a float64 window with complex64 x (or float32 / bf16
    planes) gives a float64 Pxx, computed in float64.
    """
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"Unrecognized `scaling` value {scaling}")
    assert x.is_complex()
    pr, pi = _planes(x)
    return _welch(pr, pi, x.dim(), dim, window, fs, scaling, n_overlap)


def fftshift(x, dim=-1):
    r"""Shift the zero-frequency component to the centre of the spectrum (numpy.fft.fftshift along one dim)."""
    dim = fix_dim(dim, x.dim())
    if isinstance(x, Cplx):
        return Cplx(torch.roll(x.real, x.shape[dim] // 2, dim), torch.roll(x.imag, x.shape[dim] // 2, dim))
    return torch.roll(x, x.shape[dim] // 2, dim)


def bandwidth_power(x, fs, bands, dim=-2, n_overlap=None, nperseg=None, scaling="density"):
    r"""Total power of a batch of signals in each band (lo, hi), in decibels, from a Welch estimate with a Hamming
    window of nperseg samples (default: the whole signal).

    `dim` is resolved against x as given: for a `[..., T, 2]` real input the default -2 names T; for a complex tensor
    or a Cplx it names the axis before the last, as in the reference.
    Returns (f, Pxx, band_pwr): fftshift-ed frequencies and spectrum, and `(... x len(bands))` band powers.
    """
    dim = fix_dim(dim, x.dim())
    if isinstance(x, Cplx) or x.is_complex():
        pr, pi = _planes(x)
        shape = x.shape
    else:
        assert x.shape[-1] == 2
        pr, pi = x[..., 0], x[..., 1]
        shape = x.shape[:-1]
    if nperseg is None:
        nperseg = shape[dim]
    window = torch.hamming_window(nperseg, periodic=False, dtype=_sp.compute_dtype(pr.dtype), device=pr.device)
    ff, px = _welch(pr, pi, len(shape), dim, window, fs, scaling, n_overlap)
    ff, px = fftshift(ff), fftshift(px, dim=dim)
    if not bands:
        return ff, px, torch.empty(*px.shape[:dim], *px.shape[dim + 1:], 0, dtype=px.dtype, device=px.device)
    channel = [px.narrow(dim, a, b - a).sum(dim=dim) for a, b in _band_bins(nperseg, fs, bands, px.dtype)]
    return ff, px, 10 * torch.log10(torch.stack(channel, dim=-1))


def acpr_calc(signal, sample_rate, mcf, mcb, acf=None, acb=None, nperseg=None, dim=-2):
    r"""Total power (dB) in the main channel (centre mcf, bandwidth mcb) and in the adjacent channels (centres acf, a list
    or tuple; bandwidths acb, a number or a list / tuple), from a Welch power spectrum without overlap.

    Returns (main_channel_power (..., 1), adjacent_channel_power (..., len(acf))).
    """
    if acf is None or acb is None:
        acf, acb = [], []
    elif not isinstance(acf, (list, tuple)):
        raise TypeError("Adjacent Channel Frequency offests must be a list or a tuple.")
    if isinstance(acb, (int, float)):
        acb = type(acf)([acb] * len(acf))
    elif not isinstance(acb, (list, tuple)):
        raise TypeError("Adjacent Channel Bandwidth must be a list or a tuple.")
    bands = [(-0.5 * mcb + mcf, +0.5 * mcb + mcf)]
    for f, b in zip(acf, acb):
        bands.append((-0.5 * b + f, +0.5 * b + f))
    ff, px, channel = bandwidth_power(signal, sample_rate, bands, dim=dim, nperseg=nperseg, n_overlap=0,
                                      scaling="spectrum")
    return channel[..., :1], channel[..., 1:]
