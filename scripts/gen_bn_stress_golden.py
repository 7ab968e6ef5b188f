"""Record tests/golden/bn_stress.npz: the reference package's complex batch norm (cplxmodule/nn/modules/batchnorm.py,
cplx_batch_norm + whiten2x2 under torch autograd) on the CPU, on every case of tests/bn_stress_cases.py.

    python scripts/gen_bn_stress_golden.py <reference checkout> [-v]    (the directory that holds cplxmodule/ and VERSION)

Each case runs in float64 and in float32, forward and backward, in training and in evaluation mode.  Recorded per case,
mode ("train" / "eval") and quantity (y, dx, dweight, dbias; running_mean, running_var in training mode):
  <case>/<mode>/e_ref/<quantity>   the reference's float32 error against its own float64 result, norm-wise per feature
                                   (||f32_f - f64_f|| / ||f64_f||), the maximum over the features.  The bf16 cases get the
                                   float32 run on the bf16-rounded values: recorded, not used as a margin.
  <case>/<mode>/f64/<quantity>     the float64 results, for the small cases only (Case.store64): what the numpy oracle
                                   has to reproduce (tests/test_bn_stress_host.py)
-v prints the error per feature with its condition (how the tiers of bn_stress_cases.py were chosen).  Numbers only: no
reference code goes into the file.  TEST INFRASTRUCTURE only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from gen_l0_golden import import_reference  # noqa: E402
import bn_stress_cases as sc  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "bn_stress.npz")


def reference_run(d, dtype, training):
    """-> dict over the quantities, as float64 numpy (y, dx: both planes stacked along axis 0)."""
    from cplxmodule.cplx import Cplx
    from cplxmodule.nn.modules.batchnorm import cplx_batch_norm
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    xr, xi = t(d["xr"]).requires_grad_(True), t(d["xi"]).requires_grad_(True)
    W, b = t(d["weight"]).requires_grad_(True), t(d["bias"]).requires_grad_(True)
    F = W.shape[-1]
    if training:
        rm = torch.zeros(2, F, dtype=dtype)
        rv = torch.eye(2, dtype=dtype).unsqueeze(-1).repeat(1, 1, F)
    else:
        rm, rv = t(d["running_mean"]), t(d["running_var"])
    y = cplx_batch_norm(Cplx(xr, xi), rm, rv, W, b, training, sc.MOMENTUM, sc.EPS)
    torch.autograd.backward((y.real, y.imag), (t(d["gr"]), t(d["gi"])))
    n = lambda v: v.detach().double().numpy()  # noqa: E731
    out = {"y": sc.stack_planes(n(y.real), n(y.imag)), "dx": sc.stack_planes(n(xr.grad), n(xi.grad)),
           "dweight": n(W.grad), "dbias": n(b.grad)}
    if training:
        out["running_mean"], out["running_var"] = n(rm), n(rv)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 1:
        sys.exit(__doc__)
    import_reference(os.path.abspath(args[0]))
    out = {}
    for case in sc.CASES:
        d = sc.build(case)
        floor = sc.floors(d)
        for mode, training in (("train", True), ("eval", False)):
            with np.errstate(all="ignore"):
                r64 = reference_run(d, torch.float64, training)
                r32 = reference_run(d, torch.float32, training)
            for q, v in r64.items():
                e = sc.rel_per_feature(sc.as_feature_rows(q, r32[q]), sc.as_feature_rows(q, v), floor.get(q))
                e = np.where(np.isfinite(e), e, np.inf)
                out[f"{case.name}/{mode}/e_ref/{q}"] = np.float64(e.max())
                if case.store64:
                    out[f"{case.name}/{mode}/f64/{q}"] = v
                if verbose and q in ("y", "dx", "running_var"):
                    worst = np.argsort(-e)[:4]
                    print(f"{case.name:16s} {mode:5s} {q:12s} max {e.max():.2e}  worst:",
                          ", ".join(f"{tuple(d['conds'][f])} {e[f]:.1e}" for f in worst))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 900 * 1024, size
    print(f"bn_stress: {len(out)} arrays, {size / 1024:.1f} KiB on disk")


if __name__ == "__main__":
    main()
