"""Timings of cplx.upfirdn / cplx.resample_poly (csrc/upfirdn.hip) against the two spellings a user had before, one JSON
line per row and a table.

    python scripts/bench_upfirdn.py [--warmup 2] [--iters 10] [--out profiles/upfirdn_bench.txt] [--rows 256]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native    this package: one polyphase launch (forward), P1 and P2 launches (backward)
  stuffed   the spelling of the parent commit: torch zero-stuffing -> cplx.fftconvolve -> [off::down]
  conv1d    a torch composition on the planes: F.conv1d with stride `down` (up = 1) or F.conv_transpose1d with stride
            `up` and a strided slice, one call per pair of real planes (two for a real filter, four for a complex one)

Rows, float32 and bf16 `Cplx` signals of shape [rows, 65536] with a real filter: (b) decimation by 8 with 161 taps,
(c) interpolation by 4 with 81 taps, (a) resample_poly 160/147 (3201 taps), (d) forward + backward of (a) with a filter
that requires grad.  A variant whose call takes more than a second gets one warm-up and three timed calls (its median is of three); a variant
that fails (out of memory, a solver that declines) is recorded as such, not dropped.
`of_hbm_peak`: the bytes of the planes read once plus written once (twice that with the backward) over the call's time, as a
share of the 8.0 TB/s HBM peak.  `gcmadd_per_s`: outputs x ceil(K / up) complex multiply-adds over the call's time (forward
rows).  Rows where the native path is slower than a baseline are printed in bold (**).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx  # noqa: E402
from cplxmodule_amd import upfirdn as hostup  # noqa: E402

HBM_PEAK = 8.0e12
SLOW_S = 1.0
N = 65536
ROWS = [
    # tag, up, down, taps (None: resample_poly's design), backward
    ("b_decimate_8", 1, 8, 161, False),
    ("c_interp_4", 4, 1, 81, False),
    ("a_resample_160_147", 160, 147, None, False),
    ("d_resample_fwd_bwd", 160, 147, None, True),
]


def time_variants(variants, warmup, iters):
    alive = dict(variants)
    failed = {}
    slow = set()
    for name, fn in variants.items():
        try:
            for _ in range(warmup):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if time.perf_counter() - t0 > SLOW_S:         # a call of seconds: one warm-up, three timed calls
                    slow.add(name)
                    break
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
            failed[name] = str(e).splitlines()[0][:120]
            del alive[name]
            torch.cuda.empty_cache()
    times = {name: [] for name in alive}
    for it in range(iters):
        for name, fn in alive.items():
            if name in slow and it >= 3:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times, failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_upfirdn.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for tag, up, down, taps, backward in ROWS:
        for dtype in (torch.float32, torch.bfloat16):
            xr, xi = (torch.randn(args.rows, N, device="cuda").to(dtype).requires_grad_(backward) for _ in range(2))
            if taps is None:
                h = hostup.design(up, down, 5.0, dtype, "cuda").clone()
                off, length = (h.shape[-1] - 1) // 2, -(-N * up // down)
            else:
                h = (torch.randn(taps, device="cuda") / taps ** 0.5).to(dtype)
                off, length = 0, -(-((N - 1) * up + taps) // down)
            h.requires_grad_(backward)
            k = h.shape[-1]

            def native():
                yr, yi = hostup.conv(xr, xi, h[None], None, up, down, off, length, False, True)
                return Cplx(yr, yi)

            def stuffed():
                return Cplx(*hostup._composed(xr, xi, h, None, up, down, off, length))

            def conv1d():
                w = h.float() if dtype == torch.bfloat16 else h          # float32 arithmetic, as the kernel's
                out = []
                for p in (xr, xi):
                    p = (p.float() if dtype == torch.bfloat16 else p)[:, None]
                    if up == 1:
                        y = F.conv1d(F.pad(p, (k - 1, k - 1 + down)), w.flip(0)[None, None], stride=down)[:, 0, off:]
                    else:
                        y = F.conv_transpose1d(p, w[None, None], stride=up)[:, 0, off::down]
                    out.append(y[:, :length].to(dtype).contiguous())
                return Cplx(*out)

            def diff(y, ref):
                den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                return float(torch.linalg.norm(torch.stack((y.real.float() - ref.real.float(),
                                                            y.imag.float() - ref.imag.float())).reshape(-1)) / den)

            errs = {}
            with torch.no_grad():
                y = native()
                gr, gi = torch.randn_like(y.real), torch.randn_like(y.imag)
                for name, fn in (("stuffed", stuffed), ("conv1d", conv1d)):
                    try:
                        errs[name] = diff(fn(), y)
                    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                        errs[name] = str(e).splitlines()[0][:120]
                    torch.cuda.empty_cache()
                del y

            def with_backward(fn):
                def call():
                    xr.grad = xi.grad = h.grad = None
                    y = fn()
                    torch.autograd.backward((y.real, y.imag), (gr, gi))
                return call

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            wrap = with_backward if backward else no_grad
            moved = 2 * (args.rows * N + args.rows * length) * xr.element_size() * (2 if backward else 1)
            cmadds = args.rows * length * -(-k // up)
            times, failed = time_variants({"native": wrap(native), "stuffed": wrap(stuffed), "conv1d": wrap(conv1d)},
                                          args.warmup, args.iters)
            base = statistics.median(times["native"])
            for variant in ("native", "stuffed", "conv1d"):
                row = {"row": tag, "dtype": str(dtype).replace("torch.", ""), "what": "fwd+bwd" if backward else "fwd",
                       "variant": variant, "taps": k}
                if variant in times:
                    med = statistics.median(times[variant])
                    row.update(median_ms=round(med, 4), min_ms=round(min(times[variant]), 4), x_native=round(med / base, 3),
                               of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 4),
                               gcmadd_per_s=None if backward else round(cmadds / (med * 1e-3) / 1e9, 1),
                               normwise_diff_to_native=errs.get(variant))
                else:
                    row.update(failed=failed[variant])
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xr, xi, gr, gi, h
            torch.cuda.empty_cache()
    lines = [f"cplx.upfirdn / resample_poly on Cplx [{args.rows}, {N}] with a real filter against zero-stuffing -> cplx.fftconvolve "
             f"-> slice (stuffed) and F.conv1d / conv_transpose1d per plane (conv1d); warm-up {args.warmup}, {args.iters} timed "
             "calls per variant, alternating; HIP events.  x native: the variant's median over the native one's (** native loses)",
             f"{'row':20} {'dtype':9} {'what':8} {'variant':8} {'median ms':>10} {'min ms':>9} {'x native':>9} {'of HBM peak':>12} {'Gcmadd/s':>9}"]
    for r in rows:
        if "failed" in r:
            lines.append(f"{r['row']:20} {r['dtype']:9} {r['what']:8} {r['variant']:8} failed: {r['failed']}")
            continue
        bold = "**" if r["variant"] != "native" and r["x_native"] < 1 else ""
        rate = "" if r["gcmadd_per_s"] is None else f"{r['gcmadd_per_s']:9.1f}"
        lines.append(f"{bold}{r['row']:20} {r['dtype']:9} {r['what']:8} {r['variant']:8} {r['median_ms']:10.4f} {r['min_ms']:9.4f} "
                     f"{r['x_native']:9.3f} {r['of_hbm_peak']:12.4f} {rate:>9}{bold}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
