"""Measures the bound of the bf16 gradient test of cplx.scaled_dot_product_attention (tests/test_gpu_attention.py): the
norm-wise error against float64 of torch's own bf16 F.scaled_dot_product_attention backward on the concatenated planes
(score="real", scale = 1 / sqrt(E)) over the test's gradient cases; the bound is twice the largest value.  Appends to
profiles/attention_bf16_bound.txt.  Shapes, seeds and the float64 reference are those of the test."""
import math
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(33, 31, 8, 8), (64, 65, 40, 24), (129, 130, 64, 64)]


def reference(qr, qi, kr, ki, vr, vi, causal, scale):
    s = scale * (qr @ kr.mT + qi @ ki.mT)
    if causal:
        s = s + torch.full(s.shape[-2:], -math.inf, dtype=s.dtype).triu(1)
    p = torch.softmax(s, -1)
    return p @ vr, p @ vi


def planes(lead, L, S, E, Ev, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*lead, n, e, generator=g).to(dtype) for n, e in ((L, E), (L, E), (S, E), (S, E), (S, Ev), (S, Ev))]


worst, lines = 0.0, []
for L, S, E, Ev in SHAPES:
    for causal in (False, True):
        p = planes((2, 3), L, S, E, Ev, torch.bfloat16)
        g = torch.Generator().manual_seed(7)
        up = [torch.randn(2, 3, L, Ev, generator=g).bfloat16() for _ in range(2)]
        cat = [torch.cat(p[i:i + 2], -1).cuda().requires_grad_(True) for i in (0, 2, 4)]
        o = F.scaled_dot_product_attention(*cat, is_causal=causal, scale=1 / math.sqrt(E))
        got = torch.autograd.grad(o, cat, torch.cat(up, -1).cuda())
        r = [t.double().requires_grad_(True) for t in p]
        want = torch.autograd.grad(list(reference(*r, causal, 1 / math.sqrt(E))), r, [u.double() for u in up])
        for i, name in enumerate(("dq", "dk", "dv")):
            ref = torch.cat(want[2 * i:2 * i + 2], -1)
            err = ((got[i].double().cpu() - ref).abs().max() / ref.abs().max()).item()
            worst = max(worst, err)
            lines.append(f"torch bf16 sdpa backward  L={L} S={S} E={E} Ev={Ev} causal={int(causal)}  {name}  norm-wise error {err:.4e}")
lines.append(f"largest {worst:.4e}  ->  BF16_GRAD_TOL = 2 x largest = {2 * worst:.4e}")
print("\n".join(lines))
with open(os.path.join(ROOT, "profiles", "attention_bf16_bound.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
