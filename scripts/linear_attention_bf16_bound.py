"""Measures the two bf16 bounds of tests/test_gpu_linear_attention.py: the norm-wise error (max |d - ref| / max |ref|)
against the float64 loop of `linear_attention.composed` -- the quadratic masked form, whose products torch's own bf16
arithmetic does -- on the same bf16 operands, over the test's parity cases and over its gradient cases; each bound is
twice the largest value.  Writes profiles/linear_attention_bf16_bound.txt.  Shapes, seeds, operands and the float64
reference are those of the test; the kernel under test is not run."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_linear_attention as t  # noqa: E402
from cplxmodule_amd import linear_attention as la  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_attention_bf16_bound.txt"))
args = ap.parse_args()
BF16 = torch.bfloat16


def worst(got, ref):
    """a plane, or a Cplx against a complex reference"""
    if not torch.is_tensor(got):
        return max(worst(got.real, ref.real), worst(got.imag, ref.imag))
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()


lines, fwd, grad = [], 0.0, 0.0
for T in t.SIZES:
    for E, Ev in t.HEADS:
        q, k, v, lam, state, _, _ = t.operands(T, E, Ev, BF16)
        for with_state, reverse in ((False, False), (True, False), (False, True), (True, True)):
            s = state if with_state else None
            ref = t.loop(t.wide(q), t.wide(k), t.wide(v), t.wide(lam), t.wide(s), E ** -0.5, reverse)
            got = la.composed(t.dev(q), t.dev(k), t.dev(v), t.dev(lam), None if s is None else t.dev(s), return_state=True,
                              reverse=reverse)
            err = max(worst(o, w) for o, w in zip(got, ref))
            fwd = max(fwd, err)
            lines.append(f"composed bf16 forward   T={T} E={E} Ev={Ev} state={int(with_state)} reverse={int(reverse)}  "
                         f"norm-wise error {err:.4e}")
for T in (t.C + 1, 2 * t.C + 1):
    for E, Ev in t.HEADS[1:3]:
        for reverse in (False, True):
            for decay in ("cplx", "real", "shared"):
                q, k, v, lam, state, go, gs = t.operands(T, E, Ev, BF16, decay=decay)
                leaves = [t.wide(p).requires_grad_() for p in (q, k, v, lam, state)]
                if decay == "real":
                    leaves[3] = lam[0].double().requires_grad_()
                o, f = t.loop(*leaves, E ** -0.5, reverse)
                ref = torch.autograd.grad((t.wide(go).conj() * o).real.sum() + (t.wide(gs).conj() * f).real.sum(), leaves)
                a = [t.dev(p, True) for p in (q, k, v, lam, state)]
                o, f = la.composed(*a, return_state=True, reverse=reverse)
                (gor, goi), (gsr, gsi) = ((x.to(t.DEV) for x in p) for p in (go, gs))
                ((o.real * gor).sum() + (o.imag * goi).sum() + (f.real * gsr).sum() + (f.imag * gsi).sum()).backward()
                for name, x, w in zip(("dq", "dk", "dv", "dlog_decay", "dstate"), a, ref):
                    err = worst(x.grad, w) if torch.is_tensor(x) else max(worst(x.real.grad, w.real), worst(x.imag.grad, w.imag))
                    grad = max(grad, err)
                    lines.append(f"composed bf16 backward  T={T} E={E} Ev={Ev} reverse={int(reverse)} decay={decay:6s} {name:10s} "
                                 f"norm-wise error {err:.4e}")
lines.append(f"largest forward  {fwd:.4e}  ->  BF16_FWD_TOL  = 2 x largest = {2 * fwd:.4e}")
lines.append(f"largest backward {grad:.4e}  ->  BF16_GRAD_TOL = 2 x largest = {2 * grad:.4e}")
print("\n".join(lines[-2:]))
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
