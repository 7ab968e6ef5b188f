"""Record tests/golden/init.npz from the reference package's initialisers (cplxmodule/nn/init.py) on the CPU.

    python scripts/gen_init_golden.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

  * thin_<name>_<shape>_<dtype>_re / _im: the planes cplx_kaiming_normal_, cplx_xavier_normal_ and cplx_xavier_uniform_
    leave under torch.manual_seed(thin_seed), shapes (6, 10) and (4, 3, 2, 2), float32 and float64 (they draw from torch's
    generator, so this package must reproduce them bit for bit);
  * fans_<shape>: the reference's get_fans; scale_<shape>_<kind>: the scale both Trabelsi initialisers derive from it
    (nn/init.py:72-76, 111-115); std_<shape>_<kind>: numpy's M.std() of the weight a reference run of
    cplx_trabelsi_independent_ leaves (float64) -- the same number read back from the reference's own output.
Shapes: the reference's tests/test_init.py cases and the small ones of the GPU tier.  TEST INFRASTRUCTURE only.
"""
import math
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "init.npz")

THIN_SEED = 20181
THIN = ("cplx_kaiming_normal_", "cplx_xavier_normal_", "cplx_xavier_uniform_")
THIN_SHAPES = ((6, 10), (4, 3, 2, 2))
TRABELSI_SHAPES = ((500, 1250), (1250, 500), (32, 64, 3, 3), (3, 7, 5, 5), (48, 80), (80, 48), (8, 6, 3, 3))
KINDS = ("glorot", "xavier", "kaiming", "he")


def import_reference(ref):
    sys.path.insert(0, ref)
    m = types.ModuleType("cplxmodule.__version__")           # (a setup.py-generated module in the reference)
    m.__version__ = open(os.path.join(ref, "VERSION")).read().strip()
    sys.modules["cplxmodule.__version__"] = m
    import cplxmodule  # noqa: F401


def tag(shape):
    return "x".join(map(str, shape))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    from cplxmodule import Cplx
    from cplxmodule.nn import init
    torch.set_num_threads(1)
    d = {"thin_seed": np.array(THIN_SEED), "thin_names": np.array(THIN), "kinds": np.array(KINDS),
         "thin_shapes": np.array([tag(s) for s in THIN_SHAPES]), "trabelsi_shapes": np.array([tag(s) for s in TRABELSI_SHAPES])}
    for name in THIN:
        for shape in THIN_SHAPES:
            for dt, dn in ((torch.float32, "f32"), (torch.float64, "f64")):
                w = Cplx.empty(*shape, dtype=dt)
                torch.manual_seed(THIN_SEED)
                getattr(init, name)(w)
                d[f"thin_{name}_{tag(shape)}_{dn}_re"] = w.real.numpy().copy()
                d[f"thin_{name}_{tag(shape)}_{dn}_im"] = w.imag.numpy().copy()
    np.random.seed(5)
    for shape in TRABELSI_SHAPES:
        fan_in, fan_out = init.get_fans(Cplx.empty(*shape))
        d[f"fans_{tag(shape)}"] = np.array([int(fan_in), int(fan_out)], dtype=np.int64)
        for kind in KINDS:
            d[f"scale_{tag(shape)}_{kind}"] = np.array(
                1 / math.sqrt(fan_in + fan_out) if kind in ("glorot", "xavier") else 1 / math.sqrt(fan_in))
            w = init.cplx_trabelsi_independent_(Cplx.empty(*shape, dtype=torch.float64), kind=kind)
            d[f"std_{tag(shape)}_{kind}"] = np.array((w.real.numpy() + 1j * w.imag.numpy()).std())
    total = sum(np.asarray(v).nbytes for v in d.values())
    assert total < (1 << 20)
    np.savez_compressed(OUT, **d)
    print(f"init: {len(d)} arrays, {total / 1024:.1f} KiB uncompressed, {os.path.getsize(OUT) / 1024:.1f} KiB on disk")


if __name__ == "__main__":
    main()
