"""Timings of cplx.fft / cplx.fft2 (csrc/fft.hip) against what a user of planar tensors had before, one JSON line per
row and a table.

    python scripts/bench_fft.py [--warmup 3] [--iters 10] [--out profiles/fft_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native   this package: one launch per transformed dim, planes read and written where they lie
  torch    the yardstick, on the same device tensors: torch.complex(re, im) -> torch.fft -> .real / .imag made contiguous;
           for bf16 planes with the casts to float32 and back (torch has no complex bf16)
  one/wg   (packed row only) native with the packed kernel switched off (fft._ONE_PER_WORKGROUP): the same length on one
           workgroup per vector -- what the packing buys

Rows: fft over the last dim of [8192, 256] (packed) and [64, 65536] (four-step); fft2 of [32, 64, 256, 256], contiguous and
channels-last; fft2 of [32, 64, 224, 224] (Bluestein); each forward and forward + backward, float32 and bf16.
`of_hbm_peak`: the bytes of the planes read once plus written once (forward; twice that with the backward), over the call's
time, as a share of the 8.0 TB/s HBM peak: an end-to-end share of the call, not a kernel's -- a multi-dim transform moves
its intermediate as well, which this figure charges to the call.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402
from cplxmodule_amd import fft as hostfft  # noqa: E402

HBM_PEAK = 8.0e12
ROWS = [
    # tag, shape, function, layout, extra variants
    ("fft_8192x256", (8192, 256), "fft", "contiguous", True),
    ("fft_64x65536", (64, 65536), "fft", "contiguous", False),
    ("fft2_256_contig", (32, 64, 256, 256), "fft2", "contiguous", False),
    ("fft2_256_chlast", (32, 64, 256, 256), "fft2", "channels_last", False),
    ("fft2_224_blue", (32, 64, 224, 224), "fft2", "contiguous", False),
]


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


def one_per_workgroup(fn):
    def call():
        hostfft._ONE_PER_WORKGROUP = True
        try:
            return fn()
        finally:
            hostfft._ONE_PER_WORKGROUP = False
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fft.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag, shape, name, layout, packed in ROWS:
        for dtype in (torch.float32, torch.bfloat16):
            fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
            xr, xi = (torch.randn(shape, device="cuda").to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
                      for _ in range(2))

            def native():
                return getattr(cplx, name)(Cplx(xr, xi))

            def torch_way():
                z = torch.complex(xr.float(), xi.float()) if dtype == torch.bfloat16 else torch.complex(xr, xi)
                y = getattr(torch.fft, name)(z)
                return Cplx(y.real.to(dtype).contiguous(memory_format=fmt), y.imag.to(dtype).contiguous(memory_format=fmt))

            with torch.no_grad():
                y, ref = native(), torch_way()
                gr, gi = torch.randn_like(y.real), torch.randn_like(y.imag)
                den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                err = float(torch.linalg.norm(torch.stack((y.real.float() - ref.real.float(),
                                                           y.imag.float() - ref.imag.float())).reshape(-1)) / den)
                del y, ref, den

            def with_backward(fn):
                def call():
                    xr.grad = xi.grad = None
                    y = fn()
                    torch.autograd.backward((y.real, y.imag), (gr, gi))
                return call

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            nbytes = 4 * xr.numel() * xr.element_size()          # two planes read, two written
            for what, wrap, moved in (("fwd", no_grad, nbytes), ("fwd+bwd", with_backward, 2 * nbytes)):
                variants = {"native": wrap(native), "torch": wrap(torch_way)}
                if packed:
                    variants["one/wg"] = one_per_workgroup(wrap(native))
                times = time_variants(variants, args.warmup, args.iters)
                base = statistics.median(times["torch"])
                for variant, ts in times.items():
                    med = statistics.median(ts)
                    row = {"row": tag, "dtype": str(dtype).replace("torch.", ""), "what": what, "variant": variant,
                           "median_ms": round(med, 4), "min_ms": round(min(ts), 4), "ratio_to_torch": round(med / base, 3),
                           "gbytes_per_s": round(moved / med / 1e6, 1), "of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4),
                           "normwise_diff_to_torch": err}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del xr, xi, gr, gi
            torch.cuda.empty_cache()
    lines = [f"cplx.fft / fft2 against torch.complex -> torch.fft -> planes; warm-up {args.warmup}, {args.iters} timed calls per "
             "variant, alternating; HIP events",
             f"{'row':16} {'dtype':9} {'what':8} {'variant':7} {'median ms':>10} {'min ms':>9} {'x torch':>8} {'GB/s':>8} {'of HBM peak':>12}"]
    for r in rows:
        lines.append(f"{r['row']:16} {r['dtype']:9} {r['what']:8} {r['variant']:7} {r['median_ms']:10.4f} {r['min_ms']:9.4f} "
                     f"{r['ratio_to_torch']:8.3f} {r['gbytes_per_s']:8.1f} {r['of_hbm_peak']:12.4f}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
