"""Writes tests/golden/upfirdn_scipy.npz: the outputs of scipy.signal.upfirdn, resample_poly and firwin for the small
cases of tests/upfirdn_cases.py (float64, at most a few hundred samples per case).  Needs scipy (the file was written with
scipy 1.15.3); the tests need only the file.  Inputs are tests/upfirdn_cases.golden_input(n, seed): Gaussian, reproducible.

    python scripts/gen_upfirdn_golden.py
"""
import os
import sys

import numpy as np
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import upfirdn_cases as uc  # noqa: E402


def main():
    out = {}
    for i, (n, k, up, down) in enumerate(uc.GOLDEN_UPFIRDN):
        x, h = uc.golden_input(n, 1000 + i), uc.golden_input(k, 2000 + i)
        out[f"upfirdn_{n}_{k}_{up}_{down}"] = scipy.signal.upfirdn(h, x, up, down)
        out[f"upfirdn_real_{n}_{k}_{up}_{down}"] = scipy.signal.upfirdn(h.real, x.real, up, down)
    for i, (n, up, down) in enumerate(uc.GOLDEN_RESAMPLE):
        x = uc.golden_input(n, 3000 + i)
        out[f"resample_{n}_{up}_{down}"] = scipy.signal.resample_poly(x, up, down)
        out[f"resample_real_{n}_{up}_{down}"] = scipy.signal.resample_poly(x.real, up, down)
    for i, (n, up, down, k) in enumerate(uc.GOLDEN_WINDOW):
        x, w = uc.golden_input(n, 4000 + i), uc.golden_input(k, 5000 + i, cplx=False)
        out[f"window_{n}_{up}_{down}_{k}"] = scipy.signal.resample_poly(x, up, down, window=w)
    for up, down in uc.GOLDEN_FIRWIN:
        m = max(up, down)
        out[f"firwin_{up}_{down}"] = scipy.signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    np.savez_compressed(uc.GOLDEN, **out)
    print(f"wrote {uc.GOLDEN}: {len(out)} arrays, {os.path.getsize(uc.GOLDEN)} bytes (scipy {scipy.__version__})")


if __name__ == "__main__":
    main()
