"""Timings of cplx.lfilter / cplx.sosfilt (csrc/iir.hip) against the spellings a user had before, one JSON line per row
and a table.

    python scripts/bench_iir.py [--warmup 2] [--iters 10] [--out profiles/iir_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  row       this package with the split path switched off: one launch, one workgroup per row
  split     this package with every row cut into segments (the plan's count for the shape, or 4 where the plan itself
            would not split): four launches
  planned   this package as a user calls it: the plan picks row or split
  cumsum    torch.cumsum on both planes (only for a = [1, -1], which it computes exactly)
  fftconv   cplx.fftconvolve with the impulse response truncated at 4096 taps: the only spelling available before, and
            APPROXIMATE (normwise_diff_to_planned says by how much; wrong for poles on the unit circle)

Data: `Cplx` [256, 65536] and [1, 2^22], float32 and bf16.  Filters: the integrator 1 / [1, -1], a Butterworth biquad, a
4-section Butterworth cascade (sosfilt) and an order-8 Butterworth lfilter; forward, and forward + backward with respect
to the signal.  `of_hbm_peak`: the bytes of the signal read once plus written once (twice that with the backward) over the
call's time, as a share of the 8.0 TB/s HBM peak -- an end-to-end figure of the call, not a kernel's.  Rows where the planned
path is slower than another variant are printed in bold (**).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402
from cplxmodule_amd import iir as hostiir  # noqa: E402

HBM_PEAK = 8.0e12
SLOW_S = 1.0
TAPS = 4096


def butter_sos(sections, wc):
    """Butterworth low-pass of order 2 * sections as biquads (bilinear transform, cut-off wc of Nyquist): float64 [S, 6]"""
    n, k = 2 * sections, math.tan(math.pi * wc / 2)
    out = []
    for m in range(sections):
        q = 2 * math.sin(math.pi * (2 * m + 1) / (2 * n))
        a0 = 1 + q * k + k * k
        out.append([k * k / a0, 2 * k * k / a0, k * k / a0, 1.0, 2 * (k * k - 1) / a0, (1 - q * k + k * k) / a0])
    return torch.tensor(out, dtype=torch.float64)


def expand_ba(sos):
    """the cascade as one (b, a): products of the sections' polynomials, float64"""
    b, a = torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    conv = lambda u, v: torch.nn.functional.conv1d(u[None, None], v.flip(0)[None, None], padding=len(v) - 1)[0, 0]  # noqa: E731
    for s in sos:
        b, a = conv(b, s[:3]), conv(a, s[3:])
    return b, a


FILTERS = {
    "integrator": ("lfilter", torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0, -1.0], dtype=torch.float64)),
    "biquad": ("sosfilt", butter_sos(1, 0.2)),
    "cascade_4": ("sosfilt", butter_sos(4, 0.3)),
    "lfilter_8": ("lfilter",) + expand_ba(butter_sos(4, 0.4)),
}


def time_variants(variants, warmup, iters):
    alive, failed, slow = dict(variants), {}, set()
    for name, fn in variants.items():
        try:
            for _ in range(warmup):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if time.perf_counter() - t0 > SLOW_S:     # a call of seconds: one warm-up, three timed calls
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_iir.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    rows = []
    for shape in ((256, 65536), (1, 1 << 22)):
        for tag, (kind, *coef) in FILTERS.items():
            for dtype in (torch.float32, torch.bfloat16):
                for backward in (False, True):
                    xr, xi = (torch.randn(*shape, device="cuda").to(dtype).requires_grad_(backward) for _ in range(2))
                    co = [c.to(dtype).cuda() for c in coef]
                    order, sections = (2, co[0].shape[0]) if kind == "sosfilt" else (co[1].shape[0] - 1, 1)
                    planned = hostiir.plan(shape[1], order, sections, shape[0], 1, dtype, True, 0)
                    segs = planned["segments"] if planned["path"] == "split" else 4

                    def native():
                        x = Cplx(xr, xi)
                        return cplx.sosfilt(co[0], x) if kind == "sosfilt" else cplx.lfilter(co[0], co[1], x)

                    def cumsum():
                        return Cplx(torch.cumsum(xr, -1), torch.cumsum(xi, -1))

                    # the impulse response, truncated: the filter run on a unit pulse in float64
                    pulse = torch.zeros(TAPS, dtype=torch.float64, device="cuda")
                    pulse[0] = 1
                    with torch.no_grad():
                        c64 = [c.double().cuda() for c in coef]
                        h = (cplx.sosfilt(c64[0], pulse) if kind == "sosfilt" else cplx.lfilter(c64[0], c64[1], pulse)).to(dtype)

                    def fftconv():
                        y = cplx.fftconvolve(Cplx(xr, xi), h)
                        return Cplx(y.real[..., :shape[1]], y.imag[..., :shape[1]])

                    def diff(y, ref):
                        den = torch.linalg.norm(torch.stack((ref.real.float(), ref.imag.float())).reshape(-1))
                        return float(torch.linalg.norm(torch.stack((y.real.float() - ref.real.float(),
                                                                    y.imag.float() - ref.imag.float())).reshape(-1)) / den)

                    variants = {"planned": native, "row": native, "split": native, "fftconv": fftconv}
                    force = {"planned": 0, "row": 1, "split": segs}           # hostiir._FORCE_SEGMENTS during the variant's call
                    if tag == "integrator":
                        variants["cumsum"] = cumsum

                    def forced(name, fn):
                        def call():
                            hostiir._FORCE_SEGMENTS = force.get(name, 0)
                            try:
                                return fn()
                            finally:
                                hostiir._FORCE_SEGMENTS = 0
                        return call

                    errs = {}
                    with torch.no_grad():
                        y = variants["planned"]()
                        gr, gi = torch.randn_like(y.real), torch.randn_like(y.imag)
                        for name, fn in variants.items():
                            try:
                                errs[name] = diff(forced(name, fn)(), y)
                            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                                errs[name] = str(e).splitlines()[0][:120]
                            torch.cuda.empty_cache()
                        del y

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

                    wrap = with_backward if backward else no_grad
                    moved = 2 * 2 * shape[0] * shape[1] * xr.element_size() * (2 if backward else 1)
                    times, failed = time_variants({k: forced(k, wrap(v)) for k, v in variants.items()}, args.warmup, args.iters)
                    base = statistics.median(times["planned"])
                    for variant in variants:
                        row = {"shape": list(shape), "filter": tag, "dtype": str(dtype).replace("torch.", ""),
                               "what": "fwd+bwd" if backward else "fwd", "variant": variant, "planned_path": planned["path"],
                               "segments": {"planned": planned["segments"], "row": 1, "split": segs}.get(variant)}
                        if variant in times:
                            med = statistics.median(times[variant])
                            row.update(median_ms=round(med, 4), min_ms=round(min(times[variant]), 4),
                                       x_planned=round(med / base, 3), of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 4),
                                       normwise_diff_to_planned=errs.get(variant))
                        else:
                            row.update(failed=failed[variant])
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                    del xr, xi, gr, gi
                    torch.cuda.empty_cache()
    lines = ["cplx.lfilter / sosfilt on Cplx signals: the plan's path (planned), one workgroup per row (row), every row cut into "
             "segments (split), torch.cumsum per plane (cumsum, the integrator only) and cplx.fftconvolve with the impulse "
             f"response truncated at {TAPS} taps (fftconv: APPROXIMATE, see diff); warm-up {args.warmup}, {args.iters} timed calls per "
             "variant, alternating; HIP events.  x planned: the variant's median over the planned one's (** planned loses); "
             "of HBM peak: signal bytes read once + written once (x 2 with the backward) over the call's time / 8.0 TB/s",
             f"{'shape':14} {'filter':11} {'dtype':9} {'what':8} {'variant':8} {'segs':>5} {'median ms':>10} {'min ms':>9} "
             f"{'x planned':>10} {'of HBM peak':>12} {'diff to planned':>16}"]
    for r in rows:
        shape = "x".join(map(str, r["shape"]))
        segs = "" if r["segments"] is None else str(r["segments"])
        if "failed" in r:
            lines.append(f"{shape:14} {r['filter']:11} {r['dtype']:9} {r['what']:8} {r['variant']:8} failed: {r['failed']}")
            continue
        bold = "**" if r["variant"] != "planned" and r["x_planned"] < 1 else ""
        d = r["normwise_diff_to_planned"]
        d = f"{d:16.3g}" if isinstance(d, float) else f"{str(d):>16}"
        lines.append(f"{bold}{shape:14} {r['filter']:11} {r['dtype']:9} {r['what']:8} {r['variant']:8} {segs:>5} {r['median_ms']:10.4f} "
                     f"{r['min_ms']:9.4f} {r['x_planned']:10.3f} {r['of_hbm_peak']:12.4f} {d}{bold}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
