#!/usr/bin/env python
"""Record tests/golden/czt_scipy.npz from scipy.signal.czt / zoom_fft / czt_points (scipy 1.15), and measure the drift
of the tests' complex128 Bluestein against the direct sum (`--drift`, the table F64_DRIFT of tests/czt_cases.py).

The fixture holds short float64 cases: for every case i the input `x{i}` (complex128 [2, n]), the arguments as numbers
(`arg{i}`: kind, m, then w and a as re / im pairs -- NaN for the default w -- or f1, f2, fs, endpoint) and scipy's result
`y{i}`; for every point set j `pts_arg{j}` (m, w, a) and `pts{j}`.  The tests read it without scipy.

    python scripts/gen_czt_golden.py            # writes the fixture
    python scripts/gen_czt_golden.py --drift    # prints the drift table (no scipy needed)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "czt_scipy.npz")
CZT, ZOOM = 0.0, 1.0
nan = float("nan")


def golden():
    from scipy import signal
    rs = np.random.RandomState(20)
    out, i = {}, 0
    czt_cases = [(7, 7, None, 1 + 0j), (7, 12, None, 1 + 0j), (12, 5, None, 1 + 0j), (33, 20, np.exp(-2j * np.pi * 0.013), 1 + 0j),
                 (33, 20, 1.001 * np.exp(-2j * np.pi * 0.02), 0.98 * np.exp(2j * np.pi * 0.11)),
                 (64, 90, 0.9995 * np.exp(-2j * np.pi / 301), 1.02 * np.exp(-2j * np.pi * 0.3)), (1, 4, None, 0.5j)]
    for n, m, w, a in czt_cases:
        x = rs.randn(2, n) + 1j * rs.randn(2, n)
        out[f"x{i}"] = x
        wv = (nan, nan) if w is None else (complex(w).real, complex(w).imag)
        out[f"arg{i}"] = np.array([CZT, m, *wv, complex(a).real, complex(a).imag])
        out[f"y{i}"] = signal.czt(x, m, w, a)
        i += 1
    zoom_cases = [(16, (0.2, 0.6), 16, 2.0, False), (16, (0.2, 0.6), 9, 2.0, True), (50, 0.5, 31, 2.0, False),
                  (50, (100.0, 180.0), 64, 1000.0, True), (9, (-0.3, 0.3), 5, 2.0, False)]
    for n, fn, m, fs, endpoint in zoom_cases:
        x = rs.randn(2, n) + 1j * rs.randn(2, n)
        f1, f2 = (0.0, fn) if np.size(fn) == 1 else fn
        out[f"x{i}"] = x
        out[f"arg{i}"] = np.array([ZOOM, m, f1, f2, fs, float(endpoint)])
        out[f"y{i}"] = signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint)
        i += 1
    out["cases"] = np.array(i)
    pts = [(8, None, 1 + 0j), (5, None, 0.5 - 0.5j), (6, 0.99 * np.exp(-2j * np.pi / 13), 1 + 0j), (1, 1j, 2 + 0j)]
    for j, (m, w, a) in enumerate(pts):
        wv = (nan, nan) if w is None else (complex(w).real, complex(w).imag)
        out[f"pts_arg{j}"] = np.array([m, *wv, complex(a).real, complex(a).imag])
        out[f"pts{j}"] = signal.czt_points(m, w, a)
    out["point_sets"] = np.array(len(pts))
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


def drift():
    import czt_cases as C
    for n, m in C.SHAPES:
        if (n, m) in C.F32_ONLY:
            continue
        worst = 0.0
        for name in C.CONTOURS:
            p = C.contour_params(name, n, m)
            if p is None:
                continue
            re, im, ref, ref_real = C.case(n, m, torch.float64, name)
            worst = max(worst, C.normwise(C.bluestein(C.c128(re, im), m, *p), ref),
                        C.normwise(C.bluestein(C.c128(re, torch.zeros_like(re)), m, *p), ref_real))
        print(f"    ({n}, {m}): {worst:.2e},", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drift", action="store_true")
    drift() if ap.parse_args().drift else golden()
