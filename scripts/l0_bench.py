"""Train-step time of LinearL0 (each group) next to LinearMasked and LinearVD, and the L0 gate kernels alone.

    python scripts/l0_bench.py [--B 8192] [--I 4096] [--O 4096] [--steps 20]

bf16 activations, float32 parameters; a step is zero-grad, forward, y.backward(g) with a fixed g (no loss kernels), the
penalty sum's forward and backward for the relevance layers.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel
split.  The gate kernels' bytes are the algorithmic ones of csrc/l0.hip's header comment.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--I", type=int, default=4096)
    ap.add_argument("--O", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    from cplxmodule_amd import l0
    from cplxmodule_amd.nn import masked, relevance as rel
    dev = "cuda"
    B, I, O = args.B, args.I, args.O
    torch.manual_seed(0)
    x = torch.randn(B, I, device=dev).bfloat16().requires_grad_(True)
    gy = torch.randn(B, O, device=dev).bfloat16()
    res = {"shape": [B, I, O], "dtype": "bf16"}
    layers = {
        "LinearL0[None]": rel.LinearL0(I, O),
        "LinearL0[input]": rel.LinearL0(I, O, group="input"),
        "LinearL0[output]": rel.LinearL0(I, O, group="output"),
        "LinearMasked": masked.LinearMasked(I, O),
        "LinearVD": rel.LinearVD(I, O),
    }
    for name, layer in layers.items():
        layer = layer.to(dev).train()
        if isinstance(layer, masked.LinearMasked):
            layer.mask = torch.ones(O, I, device=dev)

        def step():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            layer(x).backward(gy)
            if isinstance(layer, rel.BaseARD):
                sum(rel.penalties(layer)).backward()
        res[name + " step ms"] = round(timed(step, args.steps), 4)
        del layer
    # the gate kernels alone (Philox mode)
    w = torch.randn(O, I, device=dev)
    la = torch.empty(O, I, device=dev).uniform_(-3, 3)
    D = torch.randn(O, I, device=dev)
    mode = l0.TRAIN
    t = timed(lambda: l0.gate_fwd(w, la, O, I, mode, seed=1, offset=2, out_dtype=torch.bfloat16), args.steps)
    res["gate fwd elementwise ms"] = round(t, 4)
    res["gate fwd elementwise GB/s"] = round(O * I * 10 / t / 1e6, 1)
    t = timed(lambda: l0.gate_bwd(D, w, la, O, I, mode, seed=1, offset=2), args.steps)
    res["gate bwd elementwise ms"] = round(t, 4)
    res["gate bwd elementwise GB/s"] = round(O * I * 20 / t / 1e6, 1)
    xb = x.detach()
    lac = torch.empty(I, device=dev).uniform_(-3, 3)
    t = timed(lambda: l0.gate_fwd(xb, lac, B, I, l0.COLS | mode, seed=1, offset=2), args.steps)
    res["gate fwd cols ms"] = round(t, 4)
    res["gate fwd cols GB/s"] = round(B * I * 4 / t / 1e6, 1)
    Dx = torch.randn(B, I, device=dev)
    t = timed(lambda: l0.gate_bwd(Dx, xb, lac, B, I, l0.COLS | mode, seed=1, offset=2, da_dtype=torch.bfloat16,
                                  az_dtype=torch.bfloat16),
              args.steps)
    res["gate bwd cols ms"] = round(t, 4)
    res["gate bwd cols GB/s"] = round(B * I * (4 + 2 + 2 + 2) / t / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
