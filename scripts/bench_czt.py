"""Timings of cplx.zoom_fft (csrc/czt.hip) against two spellings of the same result that a user had before, one JSON
line per row and a table.

    python scripts/bench_czt.py [--warmup 3] [--iters 10] [--out profiles/czt_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native    cplx.zoom_fft: the table launches and one fused launch (M <= 8192), or the workspace path
  composed  the chirp composition on the package's public API as it was before cplx.czt: plane multiplies by the opening
            chirp, cplx.fft at M, a multiply by B-hat, cplx.ifft, a slice, a multiply by the closing chirp
  torch     torch.complex(re, im) -> the same composition in torch ops and torch.fft -> planes
Both yardsticks get their three tables for free (built once, outside the timed region); native builds its own in every
call.  bf16 planes are cast to float32 and back inside the yardsticks (neither has a once-rounded bf16 path).

Rows, float32 and bf16, forward only: [8192, 4096] -> 512 bins (M = 8192, fused), [256, 65536] -> 1024 bins (M = 2^17,
workspace), [4096, 1000] -> 1000 bins (M = 2048, fused).  `of_hbm_peak`: the bytes of the n inputs read once plus the m
outputs written once, over the call's time, as a share of the 8.0 TB/s HBM peak: an end-to-end share of the call.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402
from cplxmodule_amd import czt as hostczt  # noqa: E402

HBM_PEAK = 8.0e12
BAND, FS = (0.2, 0.6), 2.0
ROWS = [("zoom_8192x4096_512", (8192, 4096), 512), ("zoom_256x65536_1024", (256, 65536), 1024),
        ("zoom_4096x1000_1000", (4096, 1000), 1000)]


def time_variants(variants, warmup, iters):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(iters):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def chirp_tables(n, m):
    """(opening [n], B-hat [M], closing [m]) in complex64 on the device, from float64 phases reduced on the host"""
    _, w_turn, a_turn = hostczt.zoom_params(n, BAND, m, FS, False)
    M = hostczt.transform_size(n, m)
    i = torch.arange(max(n, m), dtype=torch.float64)
    half = torch.remainder(i * i * (w_turn / 2), 1.0)      # |product| < 2^20 at these sizes: 1e-10 turns, ample for complex64
    chirp = torch.polar(torch.ones_like(half), 2 * math.pi * half)
    opening = chirp[:n] * torch.polar(torch.ones(n, dtype=torch.float64), -2 * math.pi * torch.remainder(a_turn * i[:n], 1.0))
    b = torch.zeros(M, dtype=torch.complex128)
    b[:m] = chirp[:m].conj()
    b[M - n + 1:] = chirp[1:n].conj().flip(0)
    return tuple(t.to(torch.complex64).cuda() for t in (opening, torch.fft.fft(b) / M, chirp[:m]))


def cmul(ar, ai, b):
    return ar * b.real - ai * b.imag, ar * b.imag + ai * b.real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_czt.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag, shape, m in ROWS:
        n = shape[-1]
        M = hostczt.transform_size(n, m)
        path = hostczt.plan(n, m, shape[0])[0]
        opening, bhat, closing = chirp_tables(n, m)
        for dtype in (torch.float32, torch.bfloat16):
            xr, xi = (torch.randn(shape, device="cuda").to(dtype) for _ in range(2))

            def native():
                return cplx.zoom_fft(Cplx(xr, xi), BAND, m, fs=FS)

            def composed():
                ar, ai = cmul(xr.float(), xi.float(), opening)
                f = cplx.fft(Cplx(ar, ai), n=M)
                g = cplx.ifft(Cplx(*cmul(f.real, f.imag, bhat)), norm="forward")
                yr, yi = cmul(g.real[..., :m], g.imag[..., :m], closing)
                return Cplx(yr.to(dtype), yi.to(dtype))

            def torch_way():
                z = torch.complex(xr.float(), xi.float()) * opening
                y = torch.fft.ifft(torch.fft.fft(z, n=M) * bhat, norm="forward")[..., :m] * closing
                return Cplx(y.real.to(dtype).contiguous(), y.imag.to(dtype).contiguous())

            with torch.no_grad():
                y, ref = native(), torch_way()
                den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                err = float(torch.linalg.norm(torch.stack((y.real.float() - ref.real.float(),
                                                           y.imag.float() - ref.imag.float())).reshape(-1)) / den)
                del y, ref, den

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            moved = 2 * shape[0] * (n + m) * xr.element_size()
            times = time_variants({"native": no_grad(native), "composed": no_grad(composed), "torch": no_grad(torch_way)},
                                  args.warmup, args.iters)
            base = statistics.median(times["torch"])
            for variant, ts in times.items():
                med = statistics.median(ts)
                row = {"row": tag, "path": path, "dtype": str(dtype).replace("torch.", ""), "variant": variant,
                       "median_ms": round(med, 4), "min_ms": round(min(ts), 4), "ratio_to_torch": round(med / base, 3),
                       "gbytes_per_s": round(moved / med / 1e6, 1), "of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4),
                       "normwise_diff_to_torch": err}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xr, xi
            torch.cuda.empty_cache()
    lines = [f"cplx.zoom_fft against the chirp composition on cplx.fft and on torch.fft; forward; warm-up {args.warmup}, "
             f"{args.iters} timed calls per variant, alternating; HIP events",
             f"{'row':20} {'path':9} {'dtype':9} {'variant':8} {'median ms':>10} {'min ms':>9} {'x torch':>8} {'GB/s':>8} "
             f"{'of HBM peak':>12} {'diff to torch':>14}"]
    for r in rows:
        lines.append(f"{r['row']:20} {r['path']:9} {r['dtype']:9} {r['variant']:8} {r['median_ms']:10.4f} {r['min_ms']:9.4f} "
                     f"{r['ratio_to_torch']:8.3f} {r['gbytes_per_s']:8.1f} {r['of_hbm_peak']:12.4f} "
                     f"{r['normwise_diff_to_torch']:14.2e}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
