"""Timings of cplx.filtfilt / cplx.sosfiltfilt (csrc/filtfilt.hip) against the composition a user spelled before, one JSON
line per row and a table.

    python scripts/bench_filtfilt.py [--warmup 2] [--iters 10] [--out profiles/filtfilt_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  fused     cplx.filtfilt / cplx.sosfiltfilt as a user calls it: two passes of the extended kernel, one workspace
  composed  the public API without them: the odd extension with torch.cat of flipped slices, cplx.lfilter / cplx.sosfilt
            with zi = zi_unit * first sample, a flip, the same again, a flip and a slice.  zi_unit is computed ONCE outside
            the timed call (the user had to derive it; here it is cplx.lfilter_zi / sosfilt_zi)

Data: `Cplx` [256, 65536] and [1, 2^22] in float32, [256, 65536] in bfloat16.  Filters: a Butterworth biquad and a 4-section
Butterworth cascade (sosfiltfilt), an order-8 Butterworth (filtfilt); padtype "odd", the default padlen.  `of_hbm_peak`: the
bytes of the signal read once plus written once over the call's time, as a share of the 8.0 TB/s HBM peak -- an end-to-end
figure of the call, not a kernel's.  Rows where the fused call is slower than the composition are printed in bold (**).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_iir import FILTERS, HBM_PEAK, time_variants  # noqa: E402
from cplxmodule_amd import Cplx, cplx  # noqa: E402
from cplxmodule_amd import filtfilt as hostff  # noqa: E402

CASES = [((256, 65536), torch.float32), ((1, 1 << 22), torch.float32), ((256, 65536), torch.bfloat16)]
TAGS = ("biquad", "cascade_4", "lfilter_8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_filtfilt.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for shape, dtype in CASES:
        for tag in TAGS:
            kind, *coef = FILTERS[tag]
            xr, xi = (torch.randn(*shape, device="cuda").to(dtype) for _ in range(2))
            co = [c.to(dtype).cuda() for c in coef]
            sos = kind == "sosfilt"
            order, sections = (2, co[0].shape[0]) if sos else (co[1].shape[0] - 1, 1)
            edge = 3 * (2 * sections + 1) if sos else 3 * (order + 1)
            plan = hostff.plan(shape[1], edge, order, sections, shape[0], 1, dtype, True)
            zi = cplx.sosfilt_zi(co[0]) if sos else cplx.lfilter_zi(co[0], co[1])
            n = shape[1]

            def fused():
                x = Cplx(xr, xi)
                return cplx.sosfiltfilt(co[0], x) if sos else cplx.filtfilt(co[0], co[1], x)

            def ext(p):
                return torch.cat([2 * p[..., :1] - p[..., 1:edge + 1].flip(-1), p, 2 * p[..., -1:] - p[..., -edge - 1:-1].flip(-1)], -1)

            def once(pr, pi):
                first = (pr[..., :1], pi[..., :1]) if not sos else (pr[..., :1, None], pi[..., :1, None])
                z = Cplx(zi * first[0], zi * first[1])    # (a real unit state times the complex first sample)
                y, _ = cplx.sosfilt(co[0], Cplx(pr, pi), z) if sos else cplx.lfilter(co[0], co[1], Cplx(pr, pi), z)
                return y.real, y.imag

            def composed():
                yr, yi = once(ext(xr), ext(xi))
                yr, yi = once(yr.flip(-1), yi.flip(-1))
                return Cplx(yr.flip(-1)[..., edge:edge + n], yi.flip(-1)[..., edge:edge + n])

            def diff(y, ref):
                den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                return float(torch.linalg.norm(torch.stack((y.real.float() - ref.real.float(),
                                                            y.imag.float() - ref.imag.float())).reshape(-1)) / den)

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            variants = {"fused": no_grad(fused), "composed": no_grad(composed)}
            ref = variants["fused"]()
            errs = {name: diff(fn(), ref) for name, fn in variants.items()}
            del ref
            torch.cuda.empty_cache()
            moved = 2 * 2 * shape[0] * shape[1] * xr.element_size()
            times, failed = time_variants(variants, args.warmup, args.iters)
            base = statistics.median(times["fused"])
            for variant in variants:
                row = {"shape": list(shape), "filter": tag, "dtype": str(dtype).replace("torch.", ""), "variant": variant,
                       "path": plan["path"], "segments": plan["segments"], "padlen": edge}
                if variant in times:
                    med = statistics.median(times[variant])
                    row.update(median_ms=round(med, 4), min_ms=round(min(times[variant]), 4), x_fused=round(med / base, 3),
                               of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 4), normwise_diff_to_fused=errs.get(variant))
                else:
                    row.update(failed=failed[variant])
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xr, xi
            torch.cuda.empty_cache()
    lines = ["cplx.filtfilt / sosfiltfilt on Cplx signals (padtype odd, default padlen): the fused call (two passes of the extended "
             "kernel, one workspace) and the composition from the public API without it (torch.cat extension, two cplx.lfilter / "
             f"sosfilt calls with zi, three flips, a slice; zi_unit precomputed); warm-up {args.warmup}, {args.iters} timed calls per "
             "variant, alternating; HIP events.  x fused: the variant's median over the fused one's (** fused loses); of HBM "
             "peak: signal bytes read once + written once over the call's time / 8.0 TB/s",
             f"{'shape':14} {'filter':11} {'dtype':9} {'variant':9} {'path':6} {'segs':>5} {'median ms':>10} {'min ms':>9} "
             f"{'x fused':>8} {'of HBM peak':>12} {'diff to fused':>14}"]
    for r in rows:
        shape = "x".join(map(str, r["shape"]))
        if "failed" in r:
            lines.append(f"{shape:14} {r['filter']:11} {r['dtype']:9} {r['variant']:9} failed: {r['failed']}")
            continue
        bold = "**" if r["variant"] != "fused" and r["x_fused"] < 1 else ""
        lines.append(f"{bold}{shape:14} {r['filter']:11} {r['dtype']:9} {r['variant']:9} {r['path']:6} {r['segments']:>5} "
                     f"{r['median_ms']:10.4f} {r['min_ms']:9.4f} {r['x_fused']:8.3f} {r['of_hbm_peak']:12.4f} "
                     f"{r['normwise_diff_to_fused']:14.3g}{bold}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
