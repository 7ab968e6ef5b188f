"""Timings of cplx.conv_transpose3d (csrc/conv3d.hip) on two decoder-like shapes, one JSON line per row and a table.

    python scripts/bench_conv_transpose3d.py [--warmup 3] [--iters 10] [--out profiles/conv_transpose3d_bench.txt]

B = 4, 64 -> 32 channels, 32^3 -> 64^3 voxels, with (a) kernel 2, stride 2 and (b) kernel 4, stride 2, padding 1; bf16 and
float32; forward, and forward + backward (all of dx, dw).  HIP events around single calls, `--warmup` untimed calls per
variant, then `--iters` timed calls with the variants of a row ALTERNATING in the same process on the same tensors; median
and minimum in milliseconds.  Variants:

  native   this package: the data-gradient kernel with stride phases (backward: forward kernel + split-K weight gradient)
  plain    the same kernel with the phases switched off (conv3d._PLAIN_DGRAD: every tap tested per voxel) -- what the
           phases save
  torch4   the reference's own formula on the same device tensors with torch's ops: four F.conv_transpose3d calls plus the
           two adds (cplx.conv_transposend_naive) -- what a user has without this layer

FLOP = 8 per complex multiply-add that the operator needs (structural zeros not counted); `of_f32_peak` is that rate over
the float32 matrix peak, 157.3e12 FLOP/s (the kernel multiplies in float32 whatever the storage type): an end-to-end share
of the call, not a kernel's.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx, conv3d  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
SHAPES = {
    "k2s2": dict(B=4, cin=64, cout=32, dhw=(32, 32, 32), k=2, stride=2, padding=0),
    "k4s2p1": dict(B=4, cin=64, cout=32, dhw=(32, 32, 32), k=4, stride=2, padding=1),
}


def useful_macs(s):
    """complex multiply-adds of the forward pass: every (input voxel, tap) pair that lands inside the output"""
    D = s["dhw"][0]
    out = (D - 1) * s["stride"] - 2 * s["padding"] + s["k"]
    per_dim = sum(1 for i in range(D) for t in range(s["k"]) if 0 <= i * s["stride"] - s["padding"] + t < out)
    return s["B"] * s["cin"] * s["cout"] * per_dim ** 3


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


def plain(fn):
    def call():
        conv3d._PLAIN_DGRAD = True
        try:
            return fn()
        finally:
            conv3d._PLAIN_DGRAD = False
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_transpose3d.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag, s in SHAPES.items():
        for dtype in (torch.bfloat16, torch.float32):
            kw = dict(stride=s["stride"], padding=s["padding"])
            xs, ws = (s["B"], s["cin"]) + s["dhw"], (s["cin"], s["cout"]) + (s["k"],) * 3
            t = [torch.randn(sh, device="cuda").to(dtype).requires_grad_(True) for sh in (xs, xs, ws, ws)]
            xr, xi, wr, wi = t

            def native():
                return cplx.conv_transpose3d(Cplx(xr, xi), Cplx(wr, wi), None, **kw)

            def torch4():
                ct = lambda u, w: F.conv_transpose3d(u, w, None, **kw)  # noqa: E731
                return Cplx(ct(xr, wr) - ct(xi, wi), ct(xr, wi) + ct(xi, wr))

            with torch.no_grad():
                y = native()
                ref = torch4()
                gr, gi = torch.randn_like(y.real), torch.randn_like(y.imag)
                err = max(float((y.real.float() - ref.real.float()).abs().max()), float((y.imag.float() - ref.imag.float()).abs().max()))
                scale = float(ref.real.float().abs().max())
                del y, ref

            def with_backward(fn):
                def call():
                    for p in t:
                        p.grad = None
                    y = fn()
                    torch.autograd.backward((y.real, y.imag), (gr, gi))
                return call

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            macs = useful_macs(s)
            for what, wrap, flop in (("fwd", no_grad, 8 * macs), ("fwd+bwd", with_backward, 3 * 8 * macs)):
                times = time_variants({"native": wrap(native), "plain": plain(wrap(native)), "torch4": wrap(torch4)},
                                      args.warmup, args.iters)
                base = statistics.median(times["torch4"])
                for name, ts in times.items():
                    med = statistics.median(ts)
                    row = {"shape": tag, "dtype": str(dtype).replace("torch.", ""), "what": what, "variant": name,
                           "median_ms": round(med, 3), "min_ms": round(min(ts), 3), "ratio_to_torch4": round(med / base, 3),
                           "tflops": round(flop / med / 1e9, 2), "of_f32_peak": round(flop / (med * 1e-3) / F32_MATRIX_PEAK, 4),
                           "max_abs_diff_to_torch4": err, "max_abs_ref": scale}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del t, xr, xi, wr, wi, gr, gi
            torch.cuda.empty_cache()
    lines = [f"cplx.conv_transpose3d, B = 4, 64 -> 32 channels, 32^3 -> 64^3; warm-up {args.warmup}, {args.iters} timed calls per "
             "variant, alternating; HIP events",
             f"{'shape':8} {'dtype':9} {'what':8} {'variant':7} {'median ms':>10} {'min ms':>9} {'x torch4':>9} {'TFLOP/s':>8} {'of f32 peak':>12}"]
    for r in rows:
        lines.append(f"{r['shape']:8} {r['dtype']:9} {r['what']:8} {r['variant']:7} {r['median_ms']:10.3f} {r['min_ms']:9.3f} "
                     f"{r['ratio_to_torch4']:9.3f} {r['tflops']:8.2f} {r['of_f32_peak']:12.4f}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
