"""Times cplx.linear_attention against three spellings of the same layer -- linear_attention.composed (the quadratic
masked form in torch products; left out where its [T, T] matrices per batch entry do not fit), cplx.ssm_scan (N = E
states per value column: x = v^T, b = conj(k)^T and c = q^T shared by the columns through stride 0, a = exp(lambda);
the transposes are made outside the timed region) and, for context, causal cplx.scaled_dot_product_attention at the
same shape (another function: softmax, O(T^2)) -- forward and forward + backward (q, k, v and the decay require grad),
and writes profiles/linear_attention_bench.txt.  HIP events around `reps` calls, the variants alternating in one
process, every variant warmed up, the median of `rounds`.  TFLOP/s: the flops of the chunked form, 8 (C E + C Ev +
2 E Ev) per step and batch entry with C = plan["chunk"] (a complex multiply-add is 8), x 4 for forward + backward (three
more launches of the same kernel), over the CALL time (launch glue included)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx, linear_attention as la  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--composed-max", type=int, default=2048, help="the longest T at which `composed` is run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_attention_bench.txt"))
    args = ap.parse_args()
    BH, E, Ev = args.batch, 64, 64
    lines = [f"{torch.cuda.get_device_name(0)}; ms per CALL (HIP events around {args.reps} calls, launch glue included), median "
             f"of {args.rounds} rounds, variants alternating; B H={BH} E={E} Ev={Ev}, complex decay; TFLOP/s of the fused call"]
    for T, dtype in ((T, dt) for T in args.sizes for dt in (torch.float32, torch.bfloat16)):
        g = torch.Generator(device="cuda").manual_seed(0)
        n = lambda *s: torch.randn(2, *s, device="cuda", generator=g).to(dtype).requires_grad_()     # noqa: E731
        q, k, v = n(BH, T, E), n(BH, T, E), n(BH, T, Ev)
        lam = torch.stack([-0.001 - 0.1 * torch.rand(BH, T, device="cuda", generator=g),
                           3.14 * (2 * torch.rand(BH, T, device="cuda", generator=g) - 1)]).requires_grad_()
        up = torch.randn(2, BH, T, Ev, device="cuda", generator=g).to(dtype)
        # the ssm_scan spelling: time last; one row per value column, the E states shared by the columns
        with torch.no_grad():
            a = torch.stack([lam[0].exp() * lam[1].cos(), lam[0].exp() * lam[1].sin()]).to(dtype)[:, :, None, None, :]
            b = torch.stack([k[0], -k[1]]).transpose(-1, -2)[:, :, None].contiguous()
            c, x = q.detach().transpose(-1, -2)[:, :, None].contiguous(), v.detach().transpose(-1, -2).contiguous()
        sa, sb, sc, sx = (t.requires_grad_() for t in (a.expand(2, BH, 1, E, T).contiguous(), b, c, x))
        p = la.plan(T, E, Ev, BH, dtype)
        flops = 8 * (p["chunk"] * (E + Ev) + 2 * E * Ev) * T * BH
        for mode in ("fwd", "fwd+bwd"):
            def job(fn, leaves, upstream):
                def step():
                    with torch.set_grad_enabled(mode != "fwd"):
                        y = fn()
                        if mode != "fwd":
                            torch.autograd.grad([y.real, y.imag], leaves, list(upstream))
                return step
            main_leaves, wide = [q, k, v, lam], (2, BH, Ev, E, T)
            jobs = {"fused": job(lambda: cplx.linear_attention(Cplx(*q), Cplx(*k), Cplx(*v), Cplx(*lam)), main_leaves, up)}
            if T <= args.composed_max:
                jobs["composed"] = job(lambda: la.composed(Cplx(*q), Cplx(*k), Cplx(*v), Cplx(*lam)), main_leaves, up)
            jobs["ssm_scan"] = job(lambda: cplx.ssm_scan(Cplx(*sa.expand(wide)), Cplx(*sb.expand(wide)), Cplx(*sc.expand(wide)),
                                                         Cplx(*sx)), [sx], up.transpose(-1, -2))     # (dx only: its
            # parameter gradients are [B, Ev, E, T] float32 per operand)
            jobs["sdpa causal"] = job(lambda: cplx.scaled_dot_product_attention(Cplx(*q), Cplx(*k), Cplx(*v), is_causal=True),
                                      [q, k, v], up)
            times = {name: [] for name in jobs}
            for step in jobs.values():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            rate = flops * (1 if mode == "fwd" else 4) / (med["fused"] * 1e-3)
            lines.append(f"T={T:<6d} {str(dtype)[6:]:9s} grid={p['grid']:<5d} {mode:8s} " +
                         "  ".join(f"{n_} {ms:9.3f} ms" for n_, ms in med.items()) +
                         f"   fused {rate / 1e12:6.2f} TFLOP/s, min..max {min(times['fused']):.3f}..{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
