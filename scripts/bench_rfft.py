"""Timings of cplx.rfft / cplx.rfft2 (csrc/rfft.hip) against the two ways a user of real tensors had before, one JSON line
per row and a table.

    python scripts/bench_rfft.py [--warmup 3] [--iters 10] [--out profiles/rfft_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native    this package's real transform: the half-length kernels, one real plane read, the half spectrum written
  complex   what the package offered before: cplx.fft* of Cplx(x, zeros_like(x)), narrowed to the half spectrum -- the zero
            plane is built inside the timed region, as a user had to
  torch     torch.fft.rfft* on the same device tensor -> .real / .imag made contiguous in the input's memory format; for
            bf16 with the casts to float32 and back (torch has no complex bf16)

Rows: rfft over the last dim of [8192, 256] (packed) and [64, 65536] (four-step); rfft2 of [32, 64, 256, 256] and of
[32, 64, 224, 224] (Bluestein on 112 points along the last dim), contiguous and channels-last; each forward and forward +
backward, float32 and bf16.  `x complex` and `x torch` are the native median over the other variant's: below 1 the native
call is faster.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402

from bench_fft import time_variants  # noqa: E402

ROWS = [
    # tag, shape, function, layout
    ("rfft_8192x256", (8192, 256), "rfft", "contiguous"),
    ("rfft_64x65536", (64, 65536), "rfft", "contiguous"),
    ("rfft2_256_contig", (32, 64, 256, 256), "rfft2", "contiguous"),
    ("rfft2_256_chlast", (32, 64, 256, 256), "rfft2", "channels_last"),
    ("rfft2_224_contig", (32, 64, 224, 224), "rfft2", "contiguous"),
    ("rfft2_224_chlast", (32, 64, 224, 224), "rfft2", "channels_last"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rfft.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag, shape, name, layout in ROWS:
        for dtype in (torch.float32, torch.bfloat16):
            fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
            x = torch.randn(shape, device="cuda").to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
            half = shape[-1] // 2 + 1

            def native():
                return getattr(cplx, name)(x)

            def complex_way():
                y = getattr(cplx, name[1:])(Cplx(x, torch.zeros_like(x)))
                return Cplx(y.real.narrow(-1, 0, half), y.imag.narrow(-1, 0, half))

            def torch_way():
                y = getattr(torch.fft, name)(x.float() if dtype == torch.bfloat16 else x)
                return Cplx(y.real.to(dtype).contiguous(memory_format=fmt), y.imag.to(dtype).contiguous(memory_format=fmt))

            with torch.no_grad():
                y, ref, old = native(), torch_way(), complex_way()
                gr, gi = torch.randn_like(y.real), torch.randn_like(y.imag)
                den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                err, err_old = (float(torch.linalg.norm(torch.stack((a.real.float() - ref.real.float(),
                                                                      a.imag.float() - ref.imag.float())).reshape(-1)) / den)
                                for a in (y, old))
                del y, ref, old, den

            def with_backward(fn):
                def call():
                    x.grad = None
                    out = fn()
                    torch.autograd.backward((out.real, out.imag), (gr, gi))
                return call

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            for what, wrap in (("fwd", no_grad), ("fwd+bwd", with_backward)):
                variants = {"native": wrap(native), "complex": wrap(complex_way), "torch": wrap(torch_way)}
                times = time_variants(variants, args.warmup, args.iters)
                med = {k: statistics.median(v) for k, v in times.items()}
                for variant, ts in times.items():
                    row = {"row": tag, "dtype": str(dtype).replace("torch.", ""), "what": what, "variant": variant,
                           "median_ms": round(med[variant], 4), "min_ms": round(min(ts), 4),
                           "native_over_complex": round(med["native"] / med["complex"], 3),
                           "native_over_torch": round(med["native"] / med["torch"], 3),
                           "normwise_diff_to_torch": err if variant == "native" else err_old if variant == "complex" else 0.0}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del x, gr, gi
            torch.cuda.empty_cache()
    lines = [f"cplx.rfft / rfft2 against cplx.fft* of (x, zeros) narrowed, and against torch.fft.rfft* -> planes; warm-up "
             f"{args.warmup}, {args.iters} timed calls per variant, alternating; HIP events",
             f"{'row':17} {'dtype':9} {'what':8} {'variant':8} {'median ms':>10} {'min ms':>9} {'x complex':>10} {'x torch':>8}"]
    for r in rows:
        ratios = (f"{r['native_over_complex']:10.3f} {r['native_over_torch']:8.3f}" if r["variant"] == "native" else "")
        lines.append(f"{r['row']:17} {r['dtype']:9} {r['what']:8} {r['variant']:8} {r['median_ms']:10.4f} {r['min_ms']:9.4f} {ratios}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
