"""Times cplx.scaled_dot_product_attention against (a) the composition from cplx.einsum + torch softmax and (b) torch's
fused attention on cat-ed planes (copies included; score="real" only), forward and forward + backward, and writes
profiles/attention_bench.txt.  HIP events around `reps` calls, the variants alternating, the median of `rounds`."""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cplxmodule_amd import Cplx, cplx  # noqa: E402


def fused(q, k, v, causal):
    return cplx.scaled_dot_product_attention(q, k, v, is_causal=causal)


def composed(q, k, v, causal):
    s = cplx.einsum("bld,bsd->bls", q, k.conj).real / math.sqrt(q.real.shape[-1])
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool, device=s.device).triu(1), -math.inf)
    p = torch.softmax(s.float(), -1).to(s.dtype)
    return Cplx(p @ v.real, p @ v.imag)


def torch_cat(q, k, v, causal):
    cat = [torch.cat([t.real, t.imag], -1) for t in (q, k, v)]
    o = F.scaled_dot_product_attention(*cat, is_causal=causal, scale=1 / math.sqrt(q.real.shape[-1]))
    return Cplx(*o.chunk(2, -1))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.txt"))
    args = ap.parse_args()
    rows = [(64, 2048, 64, torch.bfloat16, False), (64, 2048, 64, torch.float32, False), (64, 2048, 64, torch.bfloat16, True),
            (64, 2048, 128, torch.bfloat16, False)]
    lines = [f"{torch.cuda.get_device_name(0)}; ms per call, median of {args.rounds} rounds of {args.reps} calls, variants "
             "alternating; TFLOP/s counts 4 L S (E + Ev) per batch entry forward (halved under the causal mask), 2.5 x that "
             "for the backward"]
    for BH, L, E, dtype, causal in rows:
        mk = lambda n: Cplx(torch.randn(BH, n, E, device="cuda").to(dtype).requires_grad_(True),  # noqa: E731
                            torch.randn(BH, n, E, device="cuda").to(dtype).requires_grad_(True))
        q, k, v = mk(L), mk(L), mk(L)
        leaves = [t for z in (q, k, v) for t in (z.real, z.imag)]
        flops = 4.0 * BH * L * L * 2 * E * (0.5 if causal else 1.0)
        for mode in ("fwd", "fwd+bwd"):
            def job(fn):
                def step():
                    if mode == "fwd":
                        with torch.no_grad():
                            fn(q, k, v, causal)
                    else:
                        o = fn(q, k, v, causal)
                        torch.autograd.grad([o.real, o.imag], leaves, [torch.ones_like(o.real)] * 2)
                return step
            jobs = {"fused": job(fused), "einsum+softmax": job(composed), "torch sdpa on cat": job(torch_cat)}
            times = {name: [] for name in jobs}
            for name, step in jobs.items():
                step()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, step in jobs.items():
                    times[name].append(timed(step, args.reps))
            med = {name: statistics.median(t) for name, t in times.items()}
            total = flops * (3.5 if mode == "fwd+bwd" else 1.0)
            lines.append(f"BH={BH} L=S={L} E=Ev={E} {str(dtype)[6:]:9s} causal={int(causal)} {mode:8s} " +
                         "  ".join(f"{name} {ms:8.3f} ms" for name, ms in med.items()) +
                         f"   fused {total / med['fused'] / 1e9:6.1f} TFLOP/s, min..max {min(times['fused']):.3f}..{max(times['fused']):.3f} ms")
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
