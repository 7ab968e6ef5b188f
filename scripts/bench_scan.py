"""Times cplx.linear_recurrence and cplx.cumsum against torch baselines on the device planes, forward and forward +
backward, and writes profiles/scan_bench.txt.  Baselines (nothing is compared against the code under test): the same
recurrence as ceil(log2 T) rounds of torch elementwise ops on the maps (P, s) (a Hillis-Steele scan along the time dim,
in float32, where the tensor lies); for cumsum, torch.cumsum on each plane.  HIP events around `reps` calls, the
variants alternating in one process, every shape warmed up, the median of `rounds`.  The useful bytes of a pass are
computed from the shapes (forward: a, x read and h written, 6 planes; cumsum: 4; the backward adds the adjoint's 6 and
da's 6) and shown over the CALL time (launch glue included) as a share of the 8 TB/s HBM peak."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx, scan  # noqa: E402

PEAK = 8.0e12


def fused(ar, ai, xr, xi, tr):
    v = (lambda t: t.transpose(-1, -2)) if tr else (lambda t: t)
    o = cplx.linear_recurrence(Cplx(v(ar), v(ai)), Cplx(v(xr), v(xi)))
    return o.real, o.imag


def rounds(ar, ai, xr, xi, tr):
    """h[t] = a[t] h[t-1] + x[t] by doubling: (P, s)[t] <- (P, s)[t] o (P, s)[t - d], d = 1, 2, 4 ..."""
    dim, dtype = (-2 if tr else -1), xr.dtype
    pr, pi, sr, si = ar.float(), ai.float(), xr.float(), xi.float()
    T, d = xr.shape[dim], 1
    while d < T:
        hi = lambda t: t.narrow(dim, d, T - d)        # noqa: E731
        lo = lambda t: t.narrow(dim, 0, T - d)        # noqa: E731
        keep = lambda t: t.narrow(dim, 0, d)          # noqa: E731
        nsr = hi(pr) * lo(sr) - hi(pi) * lo(si) + hi(sr)
        nsi = hi(pr) * lo(si) + hi(pi) * lo(sr) + hi(si)
        npr, npi = hi(pr) * lo(pr) - hi(pi) * lo(pi), hi(pr) * lo(pi) + hi(pi) * lo(pr)
        pr, pi, sr, si = (torch.cat([keep(o), n], dim) for o, n in ((pr, npr), (pi, npi), (sr, nsr), (si, nsi)))
        d *= 2
    return tuple(t.to(dtype).transpose(-1, -2) if tr else t.to(dtype) for t in (sr, si))


def fused_cumsum(ar, ai, xr, xi, tr):
    o = cplx.cumsum(Cplx(xr, xi))
    return o.real, o.imag


def torch_cumsum(ar, ai, xr, xi, tr):
    return torch.cumsum(xr, -1), torch.cumsum(xi, -1)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench.txt"))
    args = ap.parse_args()
    pairs = {"recurrence": (fused, rounds), "cumsum": (fused_cumsum, torch_cumsum)}
    cases = [(op, shape, tr, dtype) for op in pairs for dtype in (torch.float32, torch.bfloat16)
             for shape, tr in (((256, 65536), False), ((1, 1 << 22), False), ((8, 4096, 1024), True))
             if not (op == "cumsum" and tr)]
    lines = [f"{torch.cuda.get_device_name(0)}; ms per CALL (HIP events around {args.reps} calls, launch glue included), median "
             f"of {args.rounds} rounds, variants alternating; GB/s = the useful bytes (recurrence: forward 6 planes, forward + "
             f"backward 18; cumsum: 4 and 8) over the call time; HBM peak {PEAK / 1e12:.0f} TB/s; `torch` = log2 T rounds of "
             "elementwise ops (recurrence) or torch.cumsum per plane (cumsum)"]
    for op, shape, tr, dtype in cases:
        g = torch.Generator(device="cuda").manual_seed(0)
        r = 0.8 + 0.2 * torch.rand(shape, device="cuda", generator=g)
        th = 6.2831853 * torch.rand(shape, device="cuda", generator=g)
        ar, ai = ((r * f(th)).to(dtype).requires_grad_(op == "recurrence") for f in (torch.cos, torch.sin))
        xr, xi = (torch.randn(shape, device="cuda", generator=g).to(dtype).requires_grad_() for _ in range(2))
        up = [torch.randn(shape, device="cuda", generator=g).to(dtype) for _ in range(2)]
        up = [u.transpose(-1, -2) for u in up] if tr else up
        T, rows = (shape[-2], shape[0]) if tr else (shape[-1], shape[0])
        p = scan.plan(T, rows, shape[-1] if tr else None, dtype)
        leaves = [ar, ai, xr, xi] if op == "recurrence" else [xr, xi]
        plane = xr.numel() * xr.element_size()
        for mode in ("fwd", "fwd+bwd"):
            def job(fn):
                def step():
                    if mode == "fwd":
                        with torch.no_grad():
                            fn(ar, ai, xr, xi, tr)
                    else:
                        torch.autograd.grad(list(fn(ar, ai, xr, xi, tr)), leaves, up)
                return step
            jobs = dict(zip(("fused", "torch"), map(job, pairs[op])))
            times = {name: [] for name in jobs}
            for step in jobs.values():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            moved = plane * ({"fwd": 6, "fwd+bwd": 18} if op == "recurrence" else {"fwd": 4, "fwd+bwd": 8})[mode]
            rate = moved / (med["fused"] * 1e-3)
            lines.append(f"{op:10s} {str(list(shape)):16s}{' transposed' if tr else '':11s} {str(dtype)[6:]:9s} {p['path']:6s} "
                         f"segments={p['segments']:<4d} {mode:8s} " + "  ".join(f"{n} {ms:8.3f} ms" for n, ms in med.items()) +
                         f"   x{med['torch'] / med['fused']:6.2f}   fused {rate / 1e9:6.0f} GB/s ({100 * rate / PEAK:4.1f} % of peak), "
                         f"min..max {min(times['fused']):.3f}..{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
