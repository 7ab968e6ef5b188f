"""Times cplx.pfb_analysis, forward and forward + backward, against the composed route on the public API and writes
profiles/pfb_bench.txt.  Baselines (nothing is compared against the code under test): `composed` is
cplx.stft(x, n_fft=K, hop_length=hop, window=h, center=False)[..., ::P, :] made dense (the strided copy a user pays to go
on); `torch` is torch.stft on the complex tensor with the same slice and copy, float32 only.  HIP events around `reps`
calls, the variants alternating in one process, every shape warmed up, the median of `rounds`.  The useful bytes of a pass
are computed from the shapes (forward: both planes of x read, both of y written; the backward the same again) and shown
over the CALL time (launch glue included) as a share of the 6.3 TB/s a copy achieves."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx, pfb  # noqa: E402

ACHIEVABLE = 6.3e12


def fused(xr, xi, h, M, hop):
    y = cplx.pfb_analysis(Cplx(xr, xi), h, M, hop)
    return y.real, y.imag


def composed(xr, xi, h, M, hop):
    z = cplx.stft(Cplx(xr, xi), n_fft=h.numel(), hop_length=hop, window=h, center=False)[..., ::h.numel() // M, :]
    return z.real.contiguous(), z.imag.contiguous()


def torch_stft(xr, xi, h, M, hop):
    z = torch.stft(torch.complex(xr, xi), n_fft=h.numel(), hop_length=hop, window=h, center=False, return_complex=True,
                   onesided=False)[..., ::h.numel() // M, :].contiguous()
    return z.real, z.imag


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfb_bench.txt"))
    args = ap.parse_args()
    # (M, P, hop, rows, T): critically sampled at three sizes, hop = M / 2, and a K whose span takes the direct plan
    shapes = [(256, 8, 256, 64, 1 << 18), (1024, 8, 1024, 64, 1 << 18), (4096, 8, 4096, 64, 1 << 18),
              (1024, 8, 512, 64, 1 << 17), (1024, 32, 1024, 16, 1 << 18)]
    lines = [f"{torch.cuda.get_device_name(0)}; ms per CALL (HIP events around {args.reps} calls, launch glue included), median "
             f"of {args.rounds} rounds, variants alternating; GB/s = the useful bytes (x read and y written; forward + backward: "
             f"twice that) over the fused call time, against the {ACHIEVABLE / 1e12:.1f} TB/s a copy achieves; `composed` = "
             "cplx.stft + [..., ::P, :] + the dense copy, `torch` = torch.stft on the complex tensor likewise (float32 only)"]
    for (M, P, hop, rows, T), dtype in ((s, d) for s in shapes for d in (torch.float32, torch.bfloat16)):
        g = torch.Generator(device="cuda").manual_seed(0)
        xr, xi = (torch.randn(rows, T, device="cuda", generator=g).to(dtype).requires_grad_() for _ in range(2))
        h = torch.randn(P * M, device="cuda", generator=g)
        F = (T - P * M) // hop + 1
        p = pfb.plan(M, P, hop, F, rows)
        useful = 2 * xr.element_size() * (rows * T + rows * F * M)
        variants = {"fused": fused, "composed": composed}
        if dtype == torch.float32:
            variants["torch"] = torch_stft
        for mode in ("fwd", "fwd+bwd"):
            def job(fn):
                def step():
                    if mode == "fwd":
                        with torch.no_grad():
                            fn(xr, xi, h, M, hop)
                    else:
                        yr, yi = fn(xr, xi, h, M, hop)
                        torch.autograd.grad((yr.float() ** 2).sum() + (yi.float() ** 2).sum(), (xr, xi))
                return step
            jobs = {name: job(fn) for name, fn in variants.items()}
            times = {name: [] for name in jobs}
            for step in jobs.values():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            rate = useful * (2 if mode == "fwd+bwd" else 1) / (med["fused"] * 1e-3)
            lines.append(f"M={M:<5d} P={P:<3d} hop={hop:<5d} rows={rows:<3d} F={F:<5d} {str(dtype)[6:]:9s} {p['plan']:6s} "
                         f"tile={p['frames_per_tile']:<4d} {mode:8s} " + "  ".join(f"{n} {ms:8.3f} ms" for n, ms in med.items()) +
                         f"   composed/fused x{med['composed'] / med['fused']:6.2f}   fused {rate / 1e9:6.0f} GB/s "
                         f"({100 * rate / ACHIEVABLE:4.1f} % of achievable), min..max {min(times['fused']):.3f}.."
                         f"{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
