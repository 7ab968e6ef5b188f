"""Times cplx.layer_norm against the same formulas composed from torch ops on the device planes (the reference: nothing is
compared against the code under test), forward and forward + backward, and writes profiles/layer_norm_bench.txt.  HIP
events around `reps` calls, the variants alternating in one process, every shape warmed up, the median of `rounds`.
The bytes a pass must move are computed from the shapes (forward: 4 planes; backward: 6 planes plus the parameters); the
GB/s are those bytes over the CALL time (launch glue included), next to the 6.3 TB/s SURVEY counts as achievable."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx  # noqa: E402

ACHIEVABLE = 6.3e12


def fused(xr, xi, w, b, kind):
    o = cplx.layer_norm(Cplx(xr, xi), xr.shape[-1], w, b, kind=kind)
    return o.real, o.imag


def composed(xr, xi, w, b, kind, eps=1e-5):
    dtype = xr.dtype
    xr, xi = xr.float(), xi.float()
    cr, ci = xr - xr.mean(-1, keepdim=True), xi - xi.mean(-1, keepdim=True)
    if kind == "modulus":
        rstd = torch.rsqrt((cr * cr + ci * ci).mean(-1, keepdim=True) + eps)
        yr, yi = cr * rstd, ci * rstd
    else:
        a, d = (cr * cr).mean(-1, keepdim=True) + eps, (ci * ci).mean(-1, keepdim=True) + eps
        bb = (cr * ci).mean(-1, keepdim=True)
        s = torch.sqrt(a * d - bb * bb)
        t = s * torch.sqrt(a + d + 2 * s)
        p, q, r = (d + s) / t, -bb / t, (a + s) / t
        yr, yi = p * cr + q * ci, q * cr + r * ci
    return (w[0, 0] * yr + w[0, 1] * yi + b[0]).to(dtype), (w[1, 0] * yr + w[1, 1] * yi + b[1]).to(dtype)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_norm_bench.txt"))
    args = ap.parse_args()
    cases = [(64 * 2048, 512, torch.bfloat16, "whiten"), (64 * 2048, 512, torch.float32, "whiten"),
             (16 * 2048, 4096, torch.bfloat16, "whiten"), (16 * 2048, 4096, torch.float32, "whiten"),
             (64 * 2048, 512, torch.bfloat16, "modulus")]
    lines = [f"{torch.cuda.get_device_name(0)}; ms per CALL (HIP events around {args.reps} calls, launch glue included), "
             f"median of {args.rounds} rounds, variants alternating; GB/s = the bytes the pass must move (forward 4 planes; "
             f"forward + backward 10 planes + 2 x the parameters) over the call time; achievable {ACHIEVABLE / 1e12:.1f} TB/s"]
    for rows, N, dtype, kind in cases:
        xr = torch.randn(rows, N, device="cuda").to(dtype).requires_grad_(True)
        xi = torch.randn(rows, N, device="cuda").to(dtype).requires_grad_(True)
        w = torch.randn(2, 2, N, device="cuda").requires_grad_(True)
        b = torch.randn(2, N, device="cuda").requires_grad_(True)
        up = [torch.randn(rows, N, device="cuda").to(dtype) for _ in range(2)]
        plane = rows * N * xr.element_size()
        for mode in ("fwd", "fwd+bwd"):
            def job(fn):
                def step():
                    if mode == "fwd":
                        with torch.no_grad():
                            fn(xr, xi, w, b, kind)
                    else:
                        torch.autograd.grad(list(fn(xr, xi, w, b, kind)), [xr, xi, w, b], up)
                return step
            jobs = {"fused": job(fused), "composed": job(composed)}
            times = {name: [] for name in jobs}
            for step in jobs.values():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            moved = 4 * plane + 6 * N * 4 if mode == "fwd" else 10 * plane + 2 * 6 * N * 4
            rate = moved / (med["fused"] * 1e-3)
            lines.append(f"rows={rows} N={N} {str(dtype)[6:]:9s} {kind:8s} {mode:8s} " +
                         "  ".join(f"{name} {ms:8.3f} ms" for name, ms in med.items()) +
                         f"   x{med['composed'] / med['fused']:5.1f}   {moved / 2 ** 20:7.0f} MiB  fused {rate / 1e9:7.0f} GB/s "
                         f"({100 * rate / ACHIEVABLE:4.1f} % of achievable), min..max {min(times['fused']):.3f}..{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
