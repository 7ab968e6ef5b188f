"""Times cplx.ssm_scan against ssm.composed (the same layer spelled with the package's other operations: torch products
on the [B, D, N, T] state, cplx.linear_recurrence, a sum over the states), forward and forward + backward, and writes
profiles/ssm_bench.txt.  Two shapes: Mamba-like (x and dt [B, D, T], b and c [B, 1, N, T] shared by the channels through
stride 0, poles a [D, N, 1]) and S4D-like, time-invariant (a, b, c [D, N, 1], no dt).  HIP events around `reps` calls,
the variants alternating in one process, every shape warmed up, the median of `rounds`.  The useful bytes of a pass are
computed from the shapes (forward: x and y, two planes each, and dt; the backward in x adds g, dx and dt again; b and c
once per batch entry) and shown over the CALL time (launch glue included) as a share of the 8 TB/s HBM peak.
`fwd+bwd x`: only x requires grad; `fwd+bwd all`: a, b, c, dt and x do (the fused route then recomputes the states)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx, ssm  # noqa: E402

PEAK = 8.0e12


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssm_bench.txt"))
    args = ap.parse_args()
    B, D, N = 4, 512, 16
    lines = [f"{torch.cuda.get_device_name(0)}; ms per CALL (HIP events around {args.reps} calls, launch glue included), median "
             f"of {args.rounds} rounds, variants alternating; B={B} D={D} N={N}, Cplx operands; GB/s = the useful bytes over the "
             f"fused call time; HBM peak {PEAK / 1e12:.0f} TB/s; `composed` = ssm.composed"]
    for kind, T, dtype in ((k, T, dt) for k, T in (("mamba", 2048), ("s4d", 4096)) for dt in (torch.float32, torch.bfloat16)):
        g = torch.Generator(device="cuda").manual_seed(0)
        n = lambda *s: torch.randn(2, *s, device="cuda", generator=g).to(dtype).requires_grad_()     # noqa: E731
        x = n(B, D, T)
        if kind == "mamba":
            a = torch.stack([-0.01 - torch.rand(D, N, 1, device="cuda", generator=g),
                             3.14 * (2 * torch.rand(D, N, 1, device="cuda", generator=g) - 1)]).to(dtype).requires_grad_()
            b, c = n(B, 1, N, T), n(B, 1, N, T)
            dt = (1e-3 + 0.1 * torch.rand(B, D, T, device="cuda", generator=g)).to(dtype).requires_grad_()
        else:
            r, th = 0.9 + 0.1 * torch.rand(D, N, 1, device="cuda", generator=g), 6.2831853 * torch.rand(D, N, 1, device="cuda", generator=g)
            a = torch.stack([r * th.cos(), r * th.sin()]).to(dtype).requires_grad_()
            b, c, dt = n(D, N, 1), n(D, N, 1), None
        up = torch.randn(2, B, D, T, device="cuda", generator=g).to(dtype)
        pair = lambda t, over=None: Cplx(*(t if over is None else t.expand(2, *over)))              # noqa: E731
        wide = (B, D, N, T) if kind == "mamba" else None
        p = ssm.plan(T, N, B * D, dtype, True, kind == "mamba")
        plane = B * D * T * x.element_size()
        for mode in ("fwd", "fwd+bwd x", "fwd+bwd all"):
            leaves = [] if mode == "fwd" else [x] if mode == "fwd+bwd x" else [t for t in (a, b, c, x, dt) if t is not None]

            def job(fn):
                def step():
                    with torch.set_grad_enabled(mode != "fwd"):
                        held = [t if any(t is v for v in leaves) else t.detach() for t in (a, b, c, x)]
                        y = fn(pair(held[0]), pair(held[1], wide), pair(held[2], wide), pair(held[3]),
                               dt=dt if dt is None or any(dt is v for v in leaves) else dt.detach())
                        if leaves:
                            torch.autograd.grad([y.real, y.imag], leaves, [up[0], up[1]])
                return step
            jobs = {"fused": job(cplx.ssm_scan), "composed": job(ssm.composed)}
            times = {name: [] for name in jobs}
            for step in jobs.values():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            moved = plane * ((5 if dt is not None else 4) * (1 if mode == "fwd" else 2))
            moved += 0 if kind == "s4d" else 4 * B * N * T * x.element_size() * (1 if mode == "fwd" else 2)
            rate = moved / (med["fused"] * 1e-3)
            lines.append(f"{kind:6s} T={T:<5d} {str(dtype)[6:]:9s} group={p['group']} grid={p['grid']:<5d} {mode:12s} " +
                         "  ".join(f"{n_} {ms:8.3f} ms" for n_, ms in med.items()) +
                         f"   x{med['composed'] / med['fused']:6.2f}   fused {rate / 1e9:6.0f} GB/s ({100 * rate / PEAK:4.1f} % of peak), "
                         f"min..max {min(times['fused']):.3f}..{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
