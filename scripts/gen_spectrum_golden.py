"""Record tests/golden/spectrum.npz from the reference package's utils/spectrum.py and utils/views.py on the CPU, in
float64 (complex128).

    python scripts/gen_spectrum_golden.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

The signal is the reference test's (tests/test_spectrum.py:39-90): 2 x 4999 samples at fs = 1000 Hz, a 100 Hz cosine
plus 0.01 complex Gaussian noise, from a fixed seed.  Recorded: pwelch with a 500-point symmetric Hamming window
(density at overlap 300, spectrum at overlap 499) and scipy.signal.welch on the same settings, fftshift, bandwidth_power
on the complex and on the [..., T, 2] form, acpr_calc with the adjacent channels as a list and as one bandwidth, and
window_view cases in the style of the reference's tests/test_utils.py.  TEST INFRASTRUCTURE only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_l0_golden import import_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "spectrum.npz")
FS = 1000.0
BANDS = [(-150.0, -50.0), (50.0, 150.0), (90.0, 110.0), (-1.0, 1.0), (600.0, 700.0)]
# (dim, size, stride, at) on a [2, 3, 64, 2, 2] tensor; at = 99 stands for None
WINDOW_VIEWS = [(-3, 5, 2, 99), (-3, 5, 2, -1), (2, 7, 3, 0), (0, 1, 1, 99), (1, 3, 1, 2), (2, 64, 1, 99), (4, 2, 5, -1)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    from cplxmodule.utils.spectrum import acpr_calc, bandwidth_power, fftshift, pwelch
    from cplxmodule.utils.views import window_view
    from scipy.signal import welch
    rs = np.random.RandomState(20261016)
    tt = np.r_[: 5 * FS - 1] / FS
    x = np.cos(2 * np.pi * 100 * tt)[np.newaxis] + 0.01 * (rs.randn(2, len(tt)) + 1j * rs.randn(2, len(tt)))
    tx = torch.from_numpy(x)
    w = torch.hamming_window(500, periodic=False, dtype=torch.float64)
    d = {"x_re": x.real.copy(), "x_im": x.imag.copy(), "window": w.numpy()}
    for scaling, ov in (("density", 300), ("spectrum", 499)):
        f, p = pwelch(tx, 1, w, fs=FS, scaling=scaling, n_overlap=ov)
        d[f"pw_{scaling}_f"], d[f"pw_{scaling}"] = f.numpy(), p.numpy()
        _, sp = welch(x, fs=FS, axis=-1, window=w.numpy(), nfft=None, nperseg=None, scaling=scaling, noverlap=ov,
                      detrend=False, return_onesided=False)
        d[f"scipy_{scaling}"] = sp
    d["fftshift"] = fftshift(torch.from_numpy(d["pw_density"]), dim=-1).numpy()
    d["fftshift_odd"] = fftshift(torch.arange(35.0).reshape(5, 7), dim=0).numpy()
    xr = torch.from_numpy(np.stack([x.real, x.imag], axis=-1))              # [2, T, 2]
    d["bands"] = np.array(BANDS)
    f, p, c = bandwidth_power(tx, FS, BANDS, dim=-1, nperseg=500, n_overlap=250)
    d["bp_cplx_f"], d["bp_cplx_px"], d["bp_cplx"] = f.numpy(), p.numpy(), c.numpy()
    f, p, c = bandwidth_power(xr, FS, BANDS, dim=-2, nperseg=500, n_overlap=250, scaling="spectrum")
    d["bp_real_f"], d["bp_real_px"], d["bp_real"] = f.numpy(), p.numpy(), c.numpy()
    m, a = acpr_calc(xr, FS, 100.0, 20.0, acf=[60.0, 140.0, -100.0], acb=[20.0, 20.0, 10.0], nperseg=1000)
    d["acpr_list_main"], d["acpr_list_adj"] = m.numpy(), a.numpy()
    m, a = acpr_calc(xr, FS, 100.0, 20.0, acf=[60.0, 140.0], acb=15.0)                 # nperseg = T = 4999
    d["acpr_scalar_main"], d["acpr_scalar_adj"] = m.numpy(), a.numpy()
    wx = torch.from_numpy(rs.randn(2, 3, 64, 2, 2))
    d["wv_x"], d["wv_params"] = wx.numpy(), np.array(WINDOW_VIEWS)
    for i, (dim, size, stride, at) in enumerate(WINDOW_VIEWS):
        d[f"wv_{i}"] = window_view(wx, dim, size, stride, at=None if at == 99 else at).numpy().copy()
    total = sum(v.nbytes for v in d.values())
    np.savez_compressed(OUT, **d)
    assert os.path.getsize(OUT) < 900 * 1024, os.path.getsize(OUT)
    print(f"spectrum: {len(d)} arrays, {total / 1024:.1f} KiB uncompressed, {os.path.getsize(OUT) / 1024:.1f} KiB on disk")


if __name__ == "__main__":
    main()
