"""Timings of cplx.stft / cplx.istft (csrc/stft.hip) against the two ways a user had before, one JSON line per row and a
table.

    python scripts/bench_stft.py [--warmup 3] [--iters 10] [--rows TAG,TAG] [--out profiles/stft_bench.txt]

HIP events around single calls, `--warmup` untimed calls per variant, then `--iters` timed calls with the variants of a row
ALTERNATING in the same process on the same tensors; median and minimum in milliseconds.  Variants:

  native    cplx.stft / cplx.istft: framing, reflect padding and window in the kernel's loader; the overlap-add as one
            gather pass
  unfold    the spelling this package offered before: cplx.rfft(F.pad(x).unfold(-1, n_fft, hop) * window) (the result is
            left frames-major: no transpose is charged), and cplx.irfft(X) * window -> F.fold -> / envelope (the envelope
            is computed once, outside the timed region)
  torch     torch.stft / torch.istft on the same device tensors -> planes made contiguous; for bf16 with the casts to
            float32 and back (torch has no complex bf16)
  bins-maj  istft only: the native call on a spectrogram that is contiguous as [..., N, frames] (what `.contiguous()` gives
            a model's output): the one frames-major copy of each plane that cplx.istft then makes is inside the time

Rows: real signals [64, 2^20] with n_fft 1024 / hop 256 (packed), [64, 2^18] with 400 / 160 (Bluestein) and [16, 2^20] with
16384 / 4096 (one vector per workgroup), and a Cplx signal [256, 65536] with 256 / 64 (the full spectrum on the packed
complex kernel; `unfold` is cplx.fft / cplx.ifft of the two planes); Hann, center=True, reflect; each forward and forward +
backward, float32 and bf16.
`GB/s` is the useful traffic of the native call -- the signal once plus both spectrogram planes once -- over its median
(the MI355X HBM peak is 8000 GB/s).  `x unfold` and `x torch` are the native median over the other variant's: below 1 the
native call is faster.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cplxmodule_amd import Cplx, cplx  # noqa: E402

from bench_fft import time_variants  # noqa: E402

ROWS = [
    # tag, rows, T, n_fft, hop, Cplx signal (full spectrum)
    ("1024_256", 64, 1 << 20, 1024, 256, False),
    ("400_160", 64, 1 << 18, 400, 160, False),
    ("c256_64", 256, 1 << 16, 256, 64, True),
    ("16384_4096", 16, 1 << 20, 16384, 4096, False),
]


def planes(t):
    """the planes of a Cplx, or the one plane of a real tensor, as a tuple"""
    return (t.real, t.imag) if isinstance(t, Cplx) else (t,)


def normwise(got, ref):
    g = torch.stack([p.float() for p in planes(got)])
    r = torch.stack([p.float() for p in planes(ref)])
    return float(torch.linalg.norm((g - r).reshape(-1)) / torch.linalg.norm(r.reshape(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stft.py needs the GPU: a timing taken anywhere else says nothing")
    torch.manual_seed(0)
    keep = None if args.rows is None else set(args.rows.split(","))
    rows = []
    for tag, nrows, T, n, hop, full in ROWS:
        if keep is not None and tag not in keep:
            continue
        for dtype in (torch.float32, torch.bfloat16):
            wide = torch.float32
            size = torch.finfo(dtype).bits // 8
            pad = n // 2
            win = torch.hann_window(n, device="cuda", dtype=wide)
            x = torch.randn(nrows, T, device="cuda").to(dtype).requires_grad_(True)
            xi = torch.randn(nrows, T, device="cuda").to(dtype).requires_grad_(True) if full else None
            frames = 1 + T // hop
            covered = n + hop * (frames - 1)
            env = F.fold((win * win).view(1, n, 1).expand(1, n, frames), (1, covered), (1, n), stride=(1, hop)).view(covered)
            env = env[pad:pad + T]

            def framed(t):
                return (F.pad(t.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1).unfold(-1, n, hop) * win).to(dtype)

            def stft_native():
                return cplx.stft(Cplx(x, xi) if full else x, n, hop, window=win)

            def stft_unfold():
                return cplx.fft(Cplx(framed(x), framed(xi))) if full else cplx.rfft(framed(x))

            def stft_torch():
                wide_x = x.float() if dtype == torch.bfloat16 else x
                if full:
                    wide_x = torch.complex(wide_x, xi.float() if dtype == torch.bfloat16 else xi)
                y = torch.stft(wide_x, n, hop, window=win, return_complex=True)
                return Cplx(y.real.to(dtype).contiguous(), y.imag.to(dtype).contiguous())

            with torch.no_grad():
                S = stft_native()
                ref = stft_torch()
                err_s = normwise(S, ref)
                del ref
            zr = S.real.detach().clone().requires_grad_(True)
            zi = S.imag.detach().clone().requires_grad_(True)
            del S
            with torch.no_grad():                              # the same values, contiguous as [rows, N, frames]
                kr, ki = zr.contiguous().requires_grad_(True), zi.contiguous().requires_grad_(True)

            def istft_native():
                return cplx.istft(Cplx(zr, zi), n, hop, window=win, length=T, return_complex=full, check_nola=False)

            def istft_bins_major():
                return cplx.istft(Cplx(kr, ki), n, hop, window=win, length=T, return_complex=full, check_nola=False)

            def folded(fr):                                    # [rows, frames, n] -> [rows, T]
                y = F.fold((fr * win).transpose(-1, -2), (1, covered), (1, n), stride=(1, hop)).view(nrows, covered)
                return (y[:, pad:pad + T] / env).to(dtype)

            def istft_unfold():
                z = Cplx(zr.transpose(-1, -2), zi.transpose(-1, -2))
                if full:
                    fr = cplx.ifft(z)
                    return Cplx(folded(fr.real), folded(fr.imag))
                return folded(cplx.irfft(z, n=n))

            def istft_torch():
                y = torch.istft(torch.complex(zr.float(), zi.float()), n, hop, window=win, length=T, return_complex=full)
                return Cplx(y.real.to(dtype), y.imag.to(dtype)) if full else y.to(dtype)

            with torch.no_grad():
                y, ref = istft_native(), istft_torch()
                err_i = normwise(y, ref)
                assert all(torch.equal(a, b) for a, b in zip(planes(y), planes(istft_bins_major())))
                gy = tuple(torch.randn_like(p) for p in planes(y))
                del y, ref
            gr, gi = torch.randn_like(zr), torch.randn_like(zi)
            bins = n if full else n // 2 + 1
            useful = ((2 if full else 1) * nrows * T + 2 * nrows * frames * bins) * size

            def no_grad(fn):
                def call():
                    with torch.no_grad():
                        return fn()
                return call

            def stft_backward(fn):
                def call():
                    x.grad = None
                    if full:
                        xi.grad = None
                    out = fn()
                    g = (gr, gi) if out.real.shape == gr.shape else (gr.transpose(-1, -2), gi.transpose(-1, -2))
                    torch.autograd.backward((out.real, out.imag), g)
                return call

            def istft_backward(fn):
                def call():
                    zr.grad = zi.grad = kr.grad = ki.grad = None
                    torch.autograd.backward(planes(fn()), gy)
                return call

            for fname, fns, err, wraps in (
                    ("stft", (stft_native, stft_unfold, stft_torch), err_s, (("fwd", no_grad), ("fwd+bwd", stft_backward))),
                    ("istft", (istft_native, istft_unfold, istft_torch, istft_bins_major), err_i, (("fwd", no_grad), ("fwd+bwd", istft_backward)))):
                for what, wrap in wraps:
                    variants = dict(zip(("native", "unfold", "torch", "bins-maj"), (wrap(f) for f in fns)))
                    times = time_variants(variants, args.warmup, args.iters)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    for variant, ts in times.items():
                        row = {"row": f"{fname}_{tag}", "dtype": str(dtype).replace("torch.", ""), "what": what, "variant": variant,
                               "median_ms": round(med[variant], 4), "min_ms": round(min(ts), 4),
                               "useful_gb_s": round((2 if what == "fwd+bwd" else 1) * useful / med[variant] / 1e6, 1),
                               "native_over_unfold": round(med["native"] / med["unfold"], 3),
                               "native_over_torch": round(med["native"] / med["torch"], 3),
                               "normwise_diff_to_torch": err if variant == "native" else 0.0}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
            del x, xi, zr, zi, kr, ki, gr, gi, gy, env
            torch.cuda.empty_cache()
    lines = [f"cplx.stft / istft against cplx.rfft of unfold * window (cplx.irfft * window -> F.fold), and against torch.stft / "
             f"istft -> planes; warm-up {args.warmup}, {args.iters} timed calls per variant, alternating; HIP events",
             f"{'row':18} {'dtype':9} {'what':8} {'variant':8} {'median ms':>10} {'min ms':>9} {'GB/s':>8} {'x unfold':>9} {'x torch':>8}"]
    for r in rows:
        ratios = (f"{r['native_over_unfold']:9.3f} {r['native_over_torch']:8.3f}" if r["variant"] == "native" else "")
        lines.append(f"{r['row']:18} {r['dtype']:9} {r['what']:8} {r['variant']:8} {r['median_ms']:10.4f} {r['min_ms']:9.4f} "
                     f"{r['useful_gb_s']:8.1f} {ratios}")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "a" if args.rows else "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
