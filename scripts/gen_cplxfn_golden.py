"""Record tests/golden/cplx_fn.npz from the reference package's complex elementary functions (cplxmodule/cplx.py:482-541)
on the CPU, in float64.

    python scripts/gen_cplxfn_golden.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

One input set of 1041 float32-representable points -- a Gaussian cloud (600 points, scale 1.5) and a 21 x 21 grid over
|x|, |y| <= 20 -- shared by the eight functions.  Per function: the reference's float64 output and the gradient of
sum(g_r * re f(z) + g_i * im f(z)) with respect to (re z, im z), for one fixed upstream gradient g.  Where the reference
overflows (tan / tanh far from the real / imaginary axis) the recorded values are not finite; the tests compare only
where they are.  TEST INFRASTRUCTURE only.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_l0_golden import import_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "cplx_fn.npz")
FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    from cplxmodule import cplx
    rs = np.random.RandomState(20261016)
    grid = np.linspace(-20.0, 20.0, 21)
    gx, gy = np.meshgrid(grid, grid)
    x = np.concatenate([1.5 * rs.randn(600), gx.ravel()]).astype(np.float32).astype(np.float64)
    y = np.concatenate([1.5 * rs.randn(600), gy.ravel()]).astype(np.float32).astype(np.float64)
    g_r, g_i = (rs.randn(len(x)).astype(np.float32).astype(np.float64) for _ in range(2))
    d = {"z_re": x, "z_im": y, "g_re": g_r, "g_im": g_i}
    for name in FUNCTIONS:
        zr = torch.tensor(x, requires_grad=True)
        zi = torch.tensor(y, requires_grad=True)
        out = getattr(cplx, name)(cplx.Cplx(zr, zi))
        loss = (out.real * torch.from_numpy(g_r)).sum() + (out.imag * torch.from_numpy(g_i)).sum()
        dr, di = torch.autograd.grad(loss, (zr, zi))
        d[f"{name}_re"], d[f"{name}_im"] = out.real.detach().numpy(), out.imag.detach().numpy()
        d[f"{name}_dre"], d[f"{name}_dim"] = dr.numpy(), di.numpy()
    total = sum(v.nbytes for v in d.values())
    assert total < 900 * 1024, total
    np.savez_compressed(OUT, **d)
    print(f"cplx_fn: {len(d)} arrays, {total / 1024:.1f} KiB uncompressed, {os.path.getsize(OUT) / 1024:.1f} KiB on disk")


if __name__ == "__main__":
    main()
