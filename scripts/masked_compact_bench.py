"""Step times of the masked layers with the route on compacted operands off and on (cplxmodule_amd/compact.py), one
JSON line per row.

    python scripts/masked_compact_bench.py [--cases linear,conv] [--warmup 5] [--iters 50] [--fractions 1,0.75,0.5,0.25,0.125]

HIP events around one forward + backward, `--warmup` untimed steps per variant and shape, then `--iters` timed steps with
the variants ALTERNATING in the same process on the same tensors; medians in milliseconds.  Every timed step ends with a
synchronisation, so the steps are NOT back to back: each starts on an idle GPU and its time includes the host's launch
latency, which weighs more on the compacted route (it launches more kernels).  The variants of a row:

  dense, dense_again   the route off, timed twice: |dense - dense_again| / dense is the SPREAD a difference has to beat
  compact              the route on (max_live = 1: taken whenever the padded operands are smaller)

Cases, bf16 activations, dead rows and columns at seeded random positions, live fraction per side from --fractions:

  linear  CplxLinearMasked 4096 -> 4096, batch 8192
  conv    CplxConv2dMasked 256 -> 256, 3 x 3, padding 1, 64 x 64 images, batch 32, channels-last

Per row: the two step times, their ratio, the arithmetic ratio O' I' / (O I) of the padded operands, and the rate of the
gather of the input and the expand of the output timed on their own, against the HBM peak (8 TB/s spec; a float4 copy
reaches 6.3 TB/s).  compact.MAX_LIVE_FRACTION is set from this table: the largest arithmetic ratio at which `compact`
beats `dense` by more than the spread in BOTH cases.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, compact  # noqa: E402
from cplxmodule_amd.nn import masked  # noqa: E402

HBM_PEAK = 8.0e12


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


def structured_mask(shape, fraction, seed):
    g = torch.Generator().manual_seed(seed)
    O, C = shape[:2]
    m = torch.zeros(shape)
    rows = torch.randperm(O, generator=g)[:max(1, round(fraction * O))]
    cols = torch.randperm(C, generator=g)[:max(1, round(fraction * C))]
    m[rows[:, None], cols[None, :]] = 1
    return m


def build(case):
    dev, bf = "cuda", torch.bfloat16
    if case == "linear":
        layer = masked.CplxLinearMasked(4096, 4096).to(dev)
        x = [torch.randn(8192, 4096, device=dev).to(bf).requires_grad_(True) for _ in range(2)]
        return layer, x, -1
    layer = masked.CplxConv2dMasked(256, 256, 3, padding=1).to(dev)
    x = [torch.randn(32, 256, 64, 64, device=dev).to(bf).contiguous(memory_format=torch.channels_last).requires_grad_(True)
         for _ in range(2)]
    return layer, x, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="linear,conv")
    ap.add_argument("--fractions", default="1,0.75,0.5,0.25,0.125")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("masked_compact_bench.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    for case in args.cases.split(","):
        layer, x, dim = build(case)
        g = None
        for k, frac in enumerate(float(f) for f in args.fractions.split(",")):
            wshape = tuple(layer.weight.real.shape)
            layer.mask = structured_mask(wshape, frac, 10 + k)

            def step(on):
                def run():
                    nonlocal g
                    layer.compact = on
                    layer.zero_grad(set_to_none=True)
                    for t in x:
                        t.grad = None
                    y = layer(Cplx(*x))
                    if g is None:
                        g = [torch.randn_like(y.real), torch.randn_like(y.imag)]
                    torch.autograd.backward([y.real, y.imag], g)
                return run

            masked.compact_(layer, max_live=1.0)
            rep = masked.compaction(layer)[""]
            t = time_variants({"dense": step(False), "compact": step(True), "dense_again": step(False)}, args.warmup, args.iters)
            med = {n: statistics.median(v) for n, v in t.items()}
            row = {"case": case, "live_fraction_per_side": frac, "rows": rep["rows"], "cols": rep["cols"],
                   "route_taken": rep["active"], "dense_ms": round(med["dense"], 4), "dense_again_ms": round(med["dense_again"], 4),
                   "compact_ms": round(med["compact"], 4), "compact_over_dense": round(med["compact"] / med["dense"], 4),
                   "dense_spread": round(abs(med["dense"] - med["dense_again"]) / med["dense"], 4),
                   "arithmetic_ratio": round(rep["rows"][1] * rep["cols"][1] / (rep["rows"][2] * rep["cols"][2]), 4)}
            if rep["active"]:
                # the two activation-sized copies on their own: bytes read + bytes written over the median time
                plan = compact.plan_of(layer)
                with torch.no_grad():
                    xd = [v.detach() for v in x]
                    y = layer(Cplx(*xd))
                    yc = compact.gather(y.real, y.imag, plan.rows, dim)
                    tt = time_variants({"gather_x": lambda: compact.gather(xd[0], xd[1], plan.cols, dim),
                                        "expand_y": lambda: compact.expand(yc[0], yc[1], plan.inv_rows, dim)},
                                       args.warmup, args.iters)
                    xg = compact.gather(xd[0], xd[1], plan.cols, dim)
                    nbytes = {"gather_x": 2 * 2 * 2 * xg[0].numel(), "expand_y": 2 * 2 * (yc[0].numel() + y.real.numel())}
                for n, v in tt.items():
                    rate = nbytes[n] / (statistics.median(v) * 1e-3)
                    row[n + "_ms"] = round(statistics.median(v), 4)
                    row[n + "_GBps"] = round(rate / 1e9, 1)
                    row[n + "_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
                del y, yc, xg
            print(json.dumps(row), flush=True)
            g = None
        del layer, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
