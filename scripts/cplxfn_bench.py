"""The complex elementary functions (cplx.exp ... cplx.tanh, csrc/cplxfn.hip) at n = 2^26 complex elements, float32 and
bf16, next to the reference's formulas spelled with torch ops (cplxmodule/cplx.py:482-541, restated below) and a two-plane
copy_ as the bandwidth yardstick.

    python scripts/cplxfn_bench.py [--n 67108864] [--steps 20] [--dtypes float32,bfloat16] [--fns exp,log,...]

HIP events around `steps` launches after a warm-up.  Per function and dtype: the forward kernel, the backward kernel (the
library call alone, on preallocated planes), forward+backward through autograd for both spellings.  Bytes are the
algorithmic ones: float32 16 B per element forward (z in, y out), 24 B backward (z, g in, dz out), bf16 half; the copy
moves 16 B (bf16 8 B) per element.  "x copy" is the kernel's GB/s over the copy's.  Run under
`rocprofv3 --kernel-trace --stats` for per-kernel times.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")


# ---- the reference's spelling (cplxmodule/cplx.py:482-541, Cplx.__truediv__ :148-165, __abs__ :183-192) --------------
def _div(a, b):
    (ar, ai), (br, bi) = a, b
    den = br * br + bi * bi
    cr, ci = br / den, -bi / den
    return ar * cr - ai * ci, ai * cr + ar * ci


def _ref(fn, x, y):
    if fn == "exp":
        s = torch.exp(x)
        return s * torch.cos(y), s * torch.sin(y)
    if fn == "log":
        return torch.log(torch.norm(torch.stack([x, y], dim=0), p=2, dim=0)), torch.atan2(y, x)
    if fn == "sin":
        return torch.sin(x) * torch.cosh(y), torch.cos(x) * torch.sinh(y)
    if fn == "cos":
        return torch.cos(x) * torch.cosh(y), -torch.sin(x) * torch.sinh(y)
    if fn == "tan":
        return _div(_ref("sin", x, y), _ref("cos", x, y))
    if fn == "sinh":
        return torch.sinh(x) * torch.cos(y), torch.cosh(x) * torch.sin(y)
    if fn == "cosh":
        return torch.cosh(x) * torch.cos(y), torch.sinh(x) * torch.sin(y)
    return _div(_ref("sinh", x, y), _ref("cosh", x, y))


def timed(fn, steps, warmup=3):
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
    ap.add_argument("--n", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--fns", default=",".join(FUNCTIONS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cplxfn_bench.py measures on the GPU"
    from cplxmodule_amd import _lib, cplx
    from cplxmodule_amd._lib import call, dtype_code, ptr, stream_ptr
    n, steps = args.n, args.steps
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for dname in args.dtypes.split(","):
        dtype = getattr(torch, dname)
        esz = torch.finfo(dtype).bits // 8
        zr, zi, gr, gi = ((2 * torch.randn(n, generator=gen, device="cuda")).to(dtype) for _ in range(4))
        yr, yi = torch.empty_like(zr), torch.empty_like(zi)
        copy_ms = timed(lambda: (yr.copy_(zr), yi.copy_(zi)), steps)
        copy_gbs = 4 * esz * n / copy_ms / 1e6
        print(f"# {dname}: n = {n}, two-plane copy_ {copy_ms:.4f} ms, {copy_gbs:.0f} GB/s", flush=True)
        print(f"{'fn':<6}{'fwd ms':>9}{'GB/s':>7}{'x copy':>8}{'bwd ms':>9}{'GB/s':>7}{'x copy':>8}"
              f"{'f+b ms':>9}{'torch f+b':>11}{'speed-up':>10}{'torch fwd':>11}", flush=True)
        for fn in args.fns.split(","):
            code = _lib.CPLX_FN[fn]
            z = cplx.Cplx(zr, zi)
            with torch.no_grad():
                fwd_ms = timed(lambda: getattr(cplx, fn)(z), steps)
            bwd_ms = timed(lambda: call("cplxamd_cplx_fn_bwd", ptr(zr), ptr(zi), ptr(gr), ptr(gi), ptr(yr), ptr(yi), n, code,
                                        dtype_code(zr), stream_ptr()), steps)
            a, b = zr.detach().requires_grad_(True), zi.detach().requires_grad_(True)

            def ours():
                w = getattr(cplx, fn)(cplx.Cplx(a, b))
                return torch.autograd.grad((w.real, w.imag), (a, b), (gr, gi))

            def theirs():
                w = _ref(fn, a, b)
                return torch.autograd.grad(w, (a, b), (gr, gi))

            fb_ms = timed(ours, steps)
            with torch.no_grad():
                tf_ms = timed(lambda: _ref(fn, zr, zi), steps)
            tfb_ms = timed(theirs, steps)
            fgbs, bgbs = 4 * esz * n / fwd_ms / 1e6, 6 * esz * n / bwd_ms / 1e6
            row = dict(fn=fn, dtype=dname, n=n, fwd_ms=fwd_ms, fwd_gbs=fgbs, fwd_x_copy=fgbs / copy_gbs, bwd_ms=bwd_ms,
                       bwd_gbs=bgbs, bwd_x_copy=bgbs / copy_gbs, fwd_bwd_ms=fb_ms, torch_fwd_bwd_ms=tfb_ms,
                       torch_fwd_ms=tf_ms, copy_ms=copy_ms, copy_gbs=copy_gbs)
            rows.append(row)
            print(f"{fn:<6}{fwd_ms:>9.4f}{fgbs:>7.0f}{fgbs / copy_gbs:>8.2f}{bwd_ms:>9.4f}{bgbs:>7.0f}{bgbs / copy_gbs:>8.2f}"
                  f"{fb_ms:>9.4f}{tfb_ms:>11.4f}{tfb_ms / fb_ms:>10.2f}{tf_ms:>11.4f}", flush=True)
        del zr, zi, gr, gi, yr, yi
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
