"""Time cplx_trabelsi_independent_ on an n x n float32 device weight next to the reference's route for the same Z: a
host numpy.linalg.svd(full_matrices=True) of it in complex128 (cplxmodule/nn/init.py:104-109).

    python scripts/init_bench.py [--n 4096] [--repeats 3] [--skip-svd]

Prints the Newton-Schulz step count, the initialiser's time (median of the repeats, after one warm-up call, device
synchronised) and the SVD's time.  There is no threshold: the numbers are for DESIGN.md section 14.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cplxmodule_amd import Cplx  # noqa: E402
from cplxmodule_amd.nn import init  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-svd", action="store_true")
    a = ap.parse_args()
    dev = "cuda"
    w = Cplx.empty(a.n, a.n, device=dev)
    torch.manual_seed(0)
    init.cplx_trabelsi_independent_(w)                       # warm-up: library load, allocator
    torch.cuda.synchronize()
    times = []
    for r in range(a.repeats):
        torch.manual_seed(1 + r)
        t0 = time.perf_counter()
        init.cplx_trabelsi_independent_(w)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the same Z as the last call drew, for the step count and for the SVD
    torch.manual_seed(a.repeats)
    z = torch.randn(2, a.n, a.n, device=dev)
    steps = init._polar_device(z[0], z[1])[3]
    m = w.real.double().cpu().numpy() + 1j * w.imag.double().cpu().numpy()
    g = m.conj().T @ m
    defect = np.abs(g / np.real(np.diag(g)).mean() - np.eye(a.n)).max()
    print(f"n = {a.n}: cplx_trabelsi_independent_ {np.median(times):.3f} s (median of {a.repeats}: "
          f"{', '.join(f'{t:.3f}' for t in times)}), {steps} Newton-Schulz steps, std {m.std():.6e} "
          f"(target {1 / np.sqrt(2 * a.n):.6e}), max |G / c - I| = {defect / 2.0 ** -24:.1f} u", flush=True)
    if not a.skip_svd:
        zc = z[0].double().cpu().numpy() + 1j * z[1].double().cpu().numpy()
        t0 = time.perf_counter()
        u, _, vh = np.linalg.svd(zc, compute_uv=True, full_matrices=True)
        t_svd = time.perf_counter() - t0
        err = np.abs(m * (np.sqrt(a.n) / np.linalg.norm(m)) - u @ vh).max()       # (a unitary matrix has ||.||_F = sqrt n)
        print(f"n = {a.n}: numpy.linalg.svd (complex128, host, {torch.get_num_threads()} threads) {t_svd:.1f} s = "
              f"{t_svd / np.median(times):.0f} x; max |M - U V^H| = {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
