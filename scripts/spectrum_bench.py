"""Welch spectra (csrc/spectrum.hip through cplxmodule_amd.utils.spectrum) next to the reference's torch spelling
(window_view -> * window -> torch.fft.fft -> abs^2 -> mean, cplxmodule/utils/spectrum.py:63-83, restated below) on the
same GPU.

    python scripts/spectrum_bench.py [--steps 10] [--shapes a,b,c]

Shapes: (a) 64 rows x 2^20 complex64 samples, Hamming 1024, overlap 512 (direct path); (b) acpr_calc on 256 x 2^16
samples with nperseg = T (four-step path); (c) the reference test's signal, 2 x 4999 samples, Hamming 500 at overlap 499
(Bluestein, 4500 segments per row).  HIP events around `steps` calls after a warm-up, forward and forward + backward;
each output is checked against the complex128 formula at the timed size first.  Run under `rocprofv3 --kernel-trace
--stats` for per-kernel times.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def ref_pxx(x, dim, window, fs=1.0, scaling="density", n_overlap=None):
    n = window.shape[0]
    n_overlap = n // 2 if n_overlap is None else n_overlap
    xw = x.unfold(dim, n, n - n_overlap) * window
    scale = fs * (window ** 2).sum() if scaling == "density" else window.sum() ** 2
    return (torch.fft.fft(xw, dim=-1).abs() ** 2).mean(dim=dim) / scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default="a,b,c")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spectrum_bench.py measures on the GPU"
    from cplxmodule_amd.utils import spectrum as sp
    from cplxmodule_amd import spectrum as hs
    gen = torch.Generator(device="cuda").manual_seed(0)
    shapes = {"a": (64, 1 << 20, 1024, 512), "b": (256, 1 << 16, 1 << 16, 0), "c": (2, 4999, 500, 499)}
    rows_out = []
    for key in args.shapes.split(","):
        rows, T, n, ov = shapes[key]
        x = torch.randn(rows, T, dtype=torch.complex64, device="cuda", generator=gen)
        w = torch.hamming_window(n, periodic=False, device="cuda")
        S = (T - n) // (n - ov) + 1
        path = hs.plan(n, rows, S)[0]
        _, p = sp.pwelch(x, 1, w, n_overlap=ov, scaling="spectrum")
        ref = ref_pxx(x.to(torch.complex128), 1, w.double(), n_overlap=ov, scaling="spectrum")
        err = float(torch.linalg.norm(p.double() - ref) / torch.linalg.norm(ref))
        del ref
        assert err < 1e-5, err
        xg = x.clone().requires_grad_(True)
        g = torch.randn(rows, n, device="cuda", generator=gen)

        with torch.no_grad():
            fwd = timed(lambda: sp.pwelch(x, 1, w, n_overlap=ov, scaling="spectrum"), args.steps)
            tfwd = timed(lambda: ref_pxx(x, 1, w, n_overlap=ov, scaling="spectrum"), args.steps)
        fb = timed(lambda: torch.autograd.grad((sp.pwelch(xg, 1, w, n_overlap=ov, scaling="spectrum")[1] * g).sum(),
                                               xg), args.steps)
        tfb = timed(lambda: torch.autograd.grad((ref_pxx(xg, 1, w, n_overlap=ov, scaling="spectrum") * g).sum(), xg),
                    args.steps)
        if key == "b":                                   # the acpr_calc call itself (its bands and decibels included)
            xr = torch.view_as_real(x)
            with torch.no_grad():
                acpr = timed(lambda: sp.acpr_calc(xr, 1.0, 0.0, 0.1, acf=[0.2, -0.2], acb=0.1, nperseg=T), args.steps)
        else:
            acpr = None
        read = rows * T * 8
        row = dict(shape=key, rows=rows, T=T, n=n, overlap=ov, segments=S, path=path, rel_err=err, fwd_ms=fwd,
                   fwd_bwd_ms=fb, torch_fwd_ms=tfwd, torch_fwd_bwd_ms=tfb, acpr_ms=acpr,
                   fwd_read_gbs=read / fwd / 1e6, speedup_fwd=tfwd / fwd, speedup_fwd_bwd=tfb / fb)
        rows_out.append(row)
        print(f"({key}) rows {rows} T {T} n {n} ov {ov} S {S} [{path}]  fwd {fwd:.3f} ms ({read / fwd / 1e6:.0f} GB/s "
              f"of x)  f+b {fb:.3f} ms  | torch fwd {tfwd:.3f} ms  f+b {tfb:.3f} ms  | x{tfwd / fwd:.2f} fwd, "
              f"x{tfb / fb:.2f} f+b  rel err {err:.1e}" + (f"  acpr_calc {acpr:.3f} ms" if acpr else ""), flush=True)
        del x, xg, g
        torch.cuda.empty_cache()
    for r in rows_out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
