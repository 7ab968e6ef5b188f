"""Timings of cplx.fftconvolve (csrc/fftconv.hip) against the two spellings a user of planar tensors had before, and
the block-length sweep behind the plan's rule; one JSON line per row and a table.

    python scripts/bench_fftconv.py [--warmup 3] [--iters 10] [--out profiles/fftconv_bench.txt] [--rows a,b,c,d]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native   cplx.fftconvolve
  former   the spelling through this package's transforms: n = the power of two >= N + K - 1,
           cplx.ifft(cplx.fft(x, n) * cplx.fft(h, n)) narrowed (a real operand gets its zero plane, as cplx.fft needs one;
           bf16 planes are cast to float32 before and back after, so that the intermediates are not rounded -- those
           casts are part of the timed baseline, as they are of `torch`)
  torch    torch.complex -> torch.fft.fft / ifft at the same n -> planes, on the same tensors (float32 casts for bf16)
  L=2^l    (fused rows) native with the block length forced through cplxmodule_amd.fftconv.fftconvolve(log_l=l): every
           length from half the plan's starting point (the smallest power of two >= 4 K) up to 8192

Rows: (a) Cplx [256, 65536] * one Cplx [64]; (b) Cplx [32, 64, 16384] * real [64, 1024] (a filter per channel);
(c) real [8, 256, 4096] * real [256, 4096], "full" narrowed to 4096; (d) Cplx [16, 65536] * Cplx [8192], the composed path;
each forward and forward + backward (gradients of both operands), float32 and bf16.  `--rows` may add (e) Cplx
[256, 65536] * one Cplx [8]: the sweep of a few-tap filter behind the plan's shortest block.
`of_hbm_peak`: the useful bytes -- operands read once plus the result written once (forward; with the backward also the
incoming gradient read and both gradients written) -- over the call's time, as a share of the 8.0 TB/s HBM peak.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402
from cplxmodule_amd import fftconv as hostconv  # noqa: E402

HBM_PEAK = 8.0e12
ROWS = {
    # tag: (x shape, x complex, h shape, h complex, narrowed length or None)
    "a": ((256, 65536), True, (64,), True, None),
    "b": ((32, 64, 16384), True, (64, 1024), False, None),
    "c": ((8, 256, 4096), False, (256, 4096), False, 4096),
    "d": ((16, 65536), True, (8192,), True, None),
    "e": ((256, 65536), True, (8,), True, None),          # few taps: the sweep behind the plan's shortest block
}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fftconv.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag in args.rows.split(","):
        xshape, xc, hshape, hc, keep = ROWS[tag]
        n, k = xshape[-1], hshape[-1]
        full = n + k - 1
        npow = 1 << (full - 1).bit_length()
        for dtype in (torch.float32, torch.bfloat16):
            def make(shape, is_complex):
                planes = [torch.randn(shape, device="cuda").to(dtype).requires_grad_(True) for _ in range(2 if is_complex else 1)]
                return planes

            xs, hs = make(xshape, xc), make(hshape, hc)
            leaves = xs + hs
            wide = torch.float32 if dtype == torch.bfloat16 else dtype

            def wrap(planes):
                return Cplx(*planes) if len(planes) == 2 else planes[0]

            def narrowed(y):
                if keep is None:
                    return y
                return y[..., :keep] if torch.is_tensor(y) else Cplx(y.real[..., :keep], y.imag[..., :keep])

            def native(log_l=None):
                return narrowed(hostconv.fftconvolve(wrap(xs), wrap(hs), "full", log_l=log_l))

            def lift(planes):
                re = planes[0].to(wide)
                return Cplx(re, torch.zeros_like(re) if len(planes) == 1 else planes[1].to(wide))

            def former():
                y = cplx.ifft(cplx.fft(lift(xs), npow) * cplx.fft(lift(hs), npow))
                y = narrowed(Cplx(y.real[..., :full].to(dtype), y.imag[..., :full].to(dtype)))
                return y if xc or hc else y.real

            def torch_way():
                def z(planes):
                    re = planes[0].to(wide)
                    return torch.complex(re, torch.zeros_like(re) if len(planes) == 1 else planes[1].to(wide))
                y = torch.fft.ifft(torch.fft.fft(z(xs), npow) * torch.fft.fft(z(hs), npow))[..., :full]
                y = narrowed(Cplx(y.real.to(dtype).contiguous(), y.imag.to(dtype).contiguous()))
                return y if xc or hc else y.real

            def outs(y):
                return (y,) if torch.is_tensor(y) else (y.real, y.imag)

            with torch.no_grad():
                y, ref = outs(native()), outs(torch_way())
                grads = [torch.randn_like(t) for t in y]
                den = torch.linalg.norm(torch.stack([t.float() for t in ref]).reshape(-1))
                err = float(torch.linalg.norm(torch.stack([a.float() - b.float() for a, b in zip(y, ref)]).reshape(-1)) / den)
                out_elems = sum(t.numel() for t in y)
                del y, ref, den

            def with_backward(fn):
                def call():
                    for t in leaves:
                        t.grad = None
                    torch.autograd.backward(outs(fn()), grads)
                return call

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            es = leaves[0].element_size()
            in_elems = sum(t.numel() for t in leaves)
            fwd_bytes = (in_elems + out_elems) * es
            p = hostconv.plan(n, k, 0, full, dtype=dtype)
            sweep = []
            if p["path"] == "fused" and not args.no_sweep:
                base = max((4 * k - 1).bit_length(), 1)
                sweep = [l for l in range(max(base - 1, (k - 1).bit_length(), 1), 14)]
            for what, wrapper, moved in (("fwd", no_grad, fwd_bytes), ("fwd+bwd", with_backward, 2 * fwd_bytes + in_elems * es)):
                variants = {"native": wrapper(native), "former": wrapper(former), "torch": wrapper(torch_way)}
                for l in sweep:
                    variants[f"L=2^{l}"] = wrapper(lambda l=l: native(l))
                times = time_variants(variants, args.warmup, args.iters)
                base_t, base_f = statistics.median(times["torch"]), statistics.median(times["former"])
                for variant, ts in times.items():
                    med = statistics.median(ts)
                    row = {"row": tag, "dtype": str(dtype).replace("torch.", ""), "what": what, "variant": variant,
                           "plan_L": p["L"] if p["path"] == "fused" else "composed", "median_ms": round(med, 4),
                           "min_ms": round(min(ts), 4), "ratio_to_former": round(med / base_f, 3),
                           "ratio_to_torch": round(med / base_t, 3), "gbytes_per_s": round(moved / med / 1e6, 1),
                           "of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4), "normwise_diff_to_torch": err}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del xs, hs, leaves, grads
            torch.cuda.empty_cache()
    lines = [f"cplx.fftconvolve against the former spelling (cplx.fft) and torch.complex -> torch.fft -> planes; warm-up {args.warmup}, "
             f"{args.iters} timed calls per variant, alternating; HIP events",
             f"{'row':4} {'dtype':9} {'what':8} {'variant':8} {'plan L':>8} {'median ms':>10} {'min ms':>9} {'x former':>9} {'x torch':>8} "
             f"{'GB/s':>8} {'of HBM peak':>12}"]
    for r in rows:
        lines.append(f"{r['row']:4} {r['dtype']:9} {r['what']:8} {r['variant']:8} {str(r['plan_L']):>8} {r['median_ms']:10.4f} "
                     f"{r['min_ms']:9.4f} {r['ratio_to_former']:9.3f} {r['ratio_to_torch']:8.3f} {r['gbytes_per_s']:8.1f} "
                     f"{r['of_hbm_peak']:12.4f}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
