"""Writes tests/golden/iir_scipy.npz: scipy.signal.lfilter / sosfilt outputs in float64 / complex128 on short rows, with
and without zi, on real and complex data, together with the designed coefficients -- data only.  The tests read the file
and need no scipy.  Run from the repository root:  python scripts/gen_iir_golden.py
"""
import os

import numpy as np
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 96


def designs():
    yield "butter2", signal.butter(2, 0.2)
    yield "butter4", signal.butter(4, 0.25)
    yield "butter6", signal.butter(6, 0.3)
    yield "butter8", signal.butter(8, 0.4)
    yield "cheby4", signal.cheby1(4, 1, 0.3)
    yield "ellip4", signal.ellip(4, 1, 40, 0.3)
    yield "dcblock", (np.array([1.0, -1.0]), np.array([1.0, -0.995]))
    yield "cpole", (np.array([1.0 + 0j]), np.array([1.0, -0.9 * np.exp(0.7j)]))


def main():
    rs = np.random.RandomState(20)
    out = {}
    xr = rs.randn(2, N)
    xc = rs.randn(2, N) + 1j * rs.randn(2, N)
    out["x_real"], out["x_cplx"] = xr, xc
    for name, (b, a) in designs():
        d = max(len(a), len(b)) - 1
        zi = rs.randn(2, d) + 1j * rs.randn(2, d)
        out[f"{name}_b"], out[f"{name}_a"], out[f"{name}_zi"] = np.asarray(b), np.asarray(a), zi
        real = not (np.iscomplexobj(b) or np.iscomplexobj(a))
        for kind, x in (("real", xr), ("cplx", xc)):
            out[f"{name}_{kind}_y"] = signal.lfilter(b, a, x, axis=-1)
            z = zi.real if kind == "real" and real else zi
            out[f"{name}_{kind}_yz"], out[f"{name}_{kind}_zf"] = signal.lfilter(b, a, x, axis=-1, zi=z)
    sos = signal.butter(8, 0.3, output="sos")
    zi = rs.randn(2, sos.shape[0], 2) + 1j * rs.randn(2, sos.shape[0], 2)
    out["butter8sos_sos"], out["butter8sos_zi"] = sos, zi     # zi here: [rows, n_sections, 2]
    for kind, x in (("real", xr), ("cplx", xc)):
        out[f"butter8sos_{kind}_y"] = signal.sosfilt(sos, x, axis=-1)
        z = zi.real if kind == "real" else zi
        y, zf = signal.sosfilt(sos, x, axis=-1, zi=np.moveaxis(z, 1, 0))      # scipy: [n_sections, rows, 2]
        out[f"butter8sos_{kind}_yz"], out[f"butter8sos_{kind}_zf"] = y, np.moveaxis(zf, 0, 1)
    path = os.path.join(ROOT, "tests", "golden", "iir_scipy.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
