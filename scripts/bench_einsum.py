"""Timings of cplx.einsum (csrc/einsum.hip) against what the package already had, one JSON line per row.

    python scripts/bench_einsum.py [--rows 1,2,3,4,5] [--warmup 5] [--iters 20]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls per variant with the
variants of a row ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  FLOP = 8 per
complex multiply-add; bf16 peak 2.5e15 FLOP/s, float32 matrix peak 157.3e12.  bf16 unless said.

  1  bmk,bkn->bmn  batch 64, M = N = K = 1024: the contraction kernel vs `p @ q` (the exact-float32 batched kernel,
     untouched by this change)
  2  bhqd,bhkd->bhqk  (8, 16, 1024, 128)
  3  bmk,bkn->nbm  vs row 1 followed by permute(2, 0, 1).contiguous() of both planes
  4  bsi,oi->bso  (8, 1024, 4096) x (4096, 4096) with CPLXAMD_EINSUM_GEMM = 1 (linear's GEMM family) and = 0 (this kernel)
  5  row 1 in float32
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402

PEAK = {torch.bfloat16: 2.5e15, torch.float32: 157.3e12}


def rand(shape, dtype):
    return Cplx(torch.randn(*shape, device="cuda").to(dtype), torch.randn(*shape, device="cuda").to(dtype))


def time_variants(variants, warmup, iters):
    """{name: fn} -> {name: [ms, ...]}, the variants alternating call by call"""
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


def report(row, what, macs, dtype, times, base=None):
    for name, ts in times.items():
        med, lo = statistics.median(ts), min(ts)
        d = {"row": row, "what": what, "variant": name, "dtype": str(dtype).replace("torch.", ""), "median_ms": round(med, 4),
             "min_ms": round(lo, 4), "tflops_median": round(8 * macs / med / 1e9, 1),
             "of_peak_median": round(8 * macs / (med * 1e-3) / PEAK[dtype], 4)}
        if base and name != base:
            d["ratio_to_" + base] = round(med / statistics.median(times[base]), 4)
        print(json.dumps(d), flush=True)


def env_call(value, fn):
    def call():
        os.environ["CPLXAMD_EINSUM_GEMM"] = value
        try:
            return fn()
        finally:
            os.environ.pop("CPLXAMD_EINSUM_GEMM", None)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2,3,4,5")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_einsum.py needs the GPU: a timing taken anywhere else says nothing")
    rows = {int(r) for r in args.rows.split(",")}
    torch.manual_seed(0)
    with torch.no_grad():
        for row, dtype in ((1, torch.bfloat16), (5, torch.float32)):
            if row in rows:
                p, q = rand((64, 1024, 1024), dtype), rand((64, 1024, 1024), dtype)
                t = time_variants({"matmul": lambda: p @ q, "einsum": lambda: cplx.einsum("bmk,bkn->bmn", p, q)},
                                  args.warmup, args.iters)
                report(row, "bmk,bkn->bmn 64x1024x1024x1024", 64 * 1024 ** 3, dtype, t, base="matmul")
                if row == 1 and 3 in rows:
                    def then_permute():
                        o = cplx.einsum("bmk,bkn->bmn", p, q)
                        return o.real.permute(2, 0, 1).contiguous(), o.imag.permute(2, 0, 1).contiguous()
                    t = time_variants({"einsum_then_permute": then_permute, "einsum_nbm": lambda: cplx.einsum("bmk,bkn->nbm", p, q)},
                                      args.warmup, args.iters)
                    report(3, "bmk,bkn->nbm 64x1024x1024x1024", 64 * 1024 ** 3, dtype, t, base="einsum_then_permute")
                del p, q
        if 2 in rows:
            qh, kh = rand((8, 16, 1024, 128), torch.bfloat16), rand((8, 16, 1024, 128), torch.bfloat16)
            t = time_variants({"einsum": lambda: cplx.einsum("bhqd,bhkd->bhqk", qh, kh)}, args.warmup, args.iters)
            report(2, "bhqd,bhkd->bhqk 8x16x1024x128", 8 * 16 * 1024 * 1024 * 128, torch.bfloat16, t)
            del qh, kh
        if 4 in rows:
            x, w = rand((8, 1024, 4096), torch.bfloat16), rand((4096, 4096), torch.bfloat16)
            fn = lambda: cplx.einsum("bsi,oi->bso", x, w)  # noqa: E731
            t = time_variants({"gemm_route": env_call("1", fn), "kernel_route": env_call("0", fn),
                               "linear": lambda: cplx.linear(x, w)}, args.warmup, args.iters)
            report(4, "bsi,oi->bso 8192x4096x4096", 8192 * 4096 * 4096, torch.bfloat16, t, base="gemm_route")


if __name__ == "__main__":
    main()
