"""Record tests/golden/conv_transpose3d.npz from the reference package's cplx.conv_transpose3d and CplxConvTranspose3d
on the CPU.

    python scripts/gen_conv_transpose3d_golden.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

  * <case>_xr, _xi, _wr, _wi, (_br, _bi,) _gr, _gi: seeded float32 operands and the output gradient of a case of CASES;
    <case>_yr, _yi: what the reference's functional returns for them; <case>_dxr ... _dbi: its autograd gradients.
    The three cases pin the convention (no conjugation, weight [in, out / groups, kd, kh, kw], the order in which the
    circular padding wraps the dimensions).
  * layer_<tag>_keys / layer_<tag>_shape_<key>: state-dict keys and shapes of the reference's
    CplxConvTranspose3d(4, 6, 3, stride=2, padding=1) ('nobias': its default bias=None) and (..., bias=True) ('bias').
    The reference layer constructs on current torch but its forward does not run (torch's private _output_padding changed
    signature), so the layer is pinned by the functional.
TEST INFRASTRUCTURE only; the arrays are data.
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "conv_transpose3d.npz")

# name -> (input shape, weight shape, bias?, keyword arguments of cplx.conv_transpose3d)
CASES = {
    "aniso": ((2, 4, 3, 4, 5), (4, 3, 2, 3, 4), True,
              dict(stride=(1, 2, 3), padding=(0, 1, 2), output_padding=(0, 1, 2), dilation=(2, 1, 1), groups=2)),
    "circular": ((2, 4, 3, 4, 5), (4, 3, 2, 3, 4), True, dict(padding=(1, 2, 3), groups=2, padding_mode="circular")),
    "k4s2p1": ((1, 3, 2, 3, 4), (3, 5, 4, 4, 4), False, dict(stride=2, padding=1, groups=1)),
}
EXPECTED_SHAPES = {"circular": (2, 6, 7, 8, 9)}


def import_reference(ref):
    sys.path.insert(0, ref)
    m = types.ModuleType("cplxmodule.__version__")           # (a setup.py-generated module in the reference)
    m.__version__ = open(os.path.join(ref, "VERSION")).read().strip()
    sys.modules["cplxmodule.__version__"] = m
    import cplxmodule  # noqa: F401


def npy(t):
    return t.detach().numpy().copy()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    from cplxmodule import cplx
    from cplxmodule.nn import CplxConvTranspose3d
    torch.set_num_threads(1)
    d = {"cases": np.array(list(CASES))}
    for n, (name, (xs, ws, has_bias, kw)) in enumerate(CASES.items()):
        torch.manual_seed(3100 + n)
        t = {"xr": torch.randn(xs), "xi": torch.randn(xs), "wr": 0.3 * torch.randn(ws), "wi": 0.3 * torch.randn(ws)}
        if has_bias:
            nb = ws[1] * kw["groups"]
            t["br"], t["bi"] = torch.randn(nb), torch.randn(nb)
        for v in t.values():
            v.requires_grad_(True)
        bias = cplx.Cplx(t["br"], t["bi"]) if has_bias else None
        y = cplx.conv_transpose3d(cplx.Cplx(t["xr"], t["xi"]), cplx.Cplx(t["wr"], t["wi"]), bias, **kw)
        if name in EXPECTED_SHAPES:
            assert tuple(y.shape) == EXPECTED_SHAPES[name], y.shape
        gr, gi = torch.randn(y.shape), torch.randn(y.shape)
        torch.autograd.backward((y.real, y.imag), (gr, gi))
        for k, v in t.items():
            d[f"{name}_{k}"] = npy(v)
            d[f"{name}_d{k}"] = npy(v.grad)
        d[f"{name}_yr"], d[f"{name}_yi"], d[f"{name}_gr"], d[f"{name}_gi"] = npy(y.real), npy(y.imag), npy(gr), npy(gi)
    for tag, kw in (("nobias", {}), ("bias", {"bias": True})):
        sd = CplxConvTranspose3d(4, 6, 3, stride=2, padding=1, **kw).state_dict()
        d[f"layer_{tag}_keys"] = np.array(list(sd))
        for k, v in sd.items():
            d[f"layer_{tag}_shape_{k}"] = np.array(v.shape, dtype=np.int64)
    np.savez_compressed(OUT, **d)
    print(f"wrote {os.path.normpath(OUT)}: {os.path.getsize(OUT)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
