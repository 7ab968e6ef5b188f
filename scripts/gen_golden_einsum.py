"""Record tests/golden/einsum*.npz from the reference package's `cplx.einsum` (cplxmodule/cplx.py:1032-1059) on the CPU.

    python scripts/gen_golden_einsum.py <reference checkout>     (the directory that holds cplxmodule/ and VERSION)

Per two-operand case (`cases` holds the tags, `<tag>_eq` the equation): float32-representable operands `<tag>_ar/_ai/_br/
_bi` ~ N(0, 1/2) per plane and an upstream gradient `<tag>_gr/_gi`, then for P in (f32, f64) the reference's output
`<tag>_P_re/_im` and its autograd gradients `<tag>_P_dar/_dai/_dbr/_dbi` of the loss sum(re * gr + im * gi), computed by
the reference in that precision from the same values.  One-operand cases (`cases1`): `<tag>_zr/_zi` and the float64
output.  Before anything is written every output is checked against numpy.einsum on complex128 (float64 halves at
1e-12, float32 halves at 1e-5 of the largest entry).  The arrays are spread over einsum.part<k>.npz files of at most
900 KiB raw each (tests/conftest.py load_golden reads the union).  TEST INFRASTRUCTURE only.
"""
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_l0_golden import import_reference  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REF_SHAPES = ((6, 16, 24), (6, 24, 16))
CASES = [(f"ref_{i}", eq) + REF_SHAPES for i, eq in enumerate(
    ["ijk, ikj", "ijk, ikj -> ij", "ijk, ikj -> k", "ijk, lkj", "ijk, lkj -> li", "ijk, lkj -> lji", "ijk, lkp"])] + [
    ("bmm", "bmk,bkn->bmn", (7, 33, 65), (7, 65, 17)),
    ("bmm_out_perm", "bmk,bkn->nbm", (7, 33, 65), (7, 65, 17)),
    ("linear", "bsi,oi->bso", (5, 6, 70), (48, 70)),
    ("heads", "bhqd,bhkd->bhqk", (3, 4, 19, 16), (3, 4, 23, 16)),
    ("two_k_modes", "abcd,cdef->abef", (5, 6, 7, 9), (7, 9, 4, 11)),
    ("k_split_order", "acbd,dfce->abef", (5, 7, 6, 9), (9, 11, 7, 4)),
    ("ellipsis", "...ik,...kj->...ij", (2, 3, 9, 31), (2, 3, 31, 5)),
    ("ellipsis_bcast", "...ik,...kj->...ij", (2, 1, 9, 31), (3, 31, 5)),
    ("sum_only", "ijk,jl->il", (6, 8, 5), (8, 9)),
    ("diag_operand", "iij,jk->ik", (8, 8, 12), (12, 5)),
    ("dot", "i,i->", (1000,), (1000,)),
    ("outer", "i,j->ij", (37,), (41,)),
    ("hadamard", "ij,ij->ij", (13, 29), (13, 29)),
    ("k1", "ik,kj->ij", (20, 1), (1, 30)),
]
CASES1 = [("one_ijk", "ijk", (10, 10, 10)), ("one_iij", "iij", (10, 10, 10)), ("one_iji", "iji", (10, 10, 10)),
          ("one_jii", "jii", (10, 10, 10)), ("one_iii", "iii", (10, 10, 10)), ("one_t", "ij->ji", (10, 10)),
          ("one_sum", "ij->", (10, 10)), ("one_trace", "ii", (10, 10))]


def close(got, want, tol, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= tol, (what, err)
    return err


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import_reference(os.path.abspath(sys.argv[1]))
    from cplxmodule import cplx
    rs = np.random.RandomState(20261016)
    draw = lambda shape: np.asarray(rs.randn(*shape) * np.sqrt(0.5), dtype=np.float32).reshape(shape)  # noqa: E731
    records, worst = [], 0.0
    for tag, eq, sa, sb in CASES:
        d = {f"{tag}_eq": np.array(eq)}
        ar, ai, br, bi = draw(sa), draw(sa), draw(sb), draw(sb)
        want = np.einsum(eq.replace(" ", ""), ar.astype(np.float64) + 1j * ai, br.astype(np.float64) + 1j * bi)
        gr, gi = draw(want.shape), draw(want.shape)
        d.update({f"{tag}_ar": ar, f"{tag}_ai": ai, f"{tag}_br": br, f"{tag}_bi": bi, f"{tag}_gr": gr, f"{tag}_gi": gi})
        for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
            ts = [torch.from_numpy(v).to(dt).requires_grad_(True) for v in (ar, ai, br, bi)]
            out = cplx.einsum(eq, cplx.Cplx(ts[0], ts[1]), cplx.Cplx(ts[2], ts[3]))
            loss = (out.real * torch.from_numpy(gr).to(dt)).sum() + (out.imag * torch.from_numpy(gi).to(dt)).sum()
            grads = torch.autograd.grad(loss, ts)
            re, im = out.real.detach().numpy(), out.imag.detach().numpy()
            tol = 1e-5 if prec == "f32" else 1e-12
            e = max(close(re, want.real, tol, (tag, prec, "re")), close(im, want.imag, tol, (tag, prec, "im")))
            if prec == "f32":
                worst = max(worst, e)
            d[f"{tag}_{prec}_re"], d[f"{tag}_{prec}_im"] = re, im
            for name, g in zip(("dar", "dai", "dbr", "dbi"), grads):
                d[f"{tag}_{prec}_{name}"] = g.numpy()
        records.append(d)
    for tag, eq, shape in CASES1:
        zr, zi = draw(shape), draw(shape)
        out = cplx.einsum(eq, cplx.Cplx(torch.from_numpy(zr).double(), torch.from_numpy(zi).double()))
        want = np.einsum(eq, zr.astype(np.float64) + 1j * zi)
        close(out.real.numpy(), want.real, 1e-12, (tag, "re"))
        close(out.imag.numpy(), want.imag, 1e-12, (tag, "im"))
        records.append({f"{tag}_eq": np.array(eq), f"{tag}_zr": zr, f"{tag}_zi": zi, f"{tag}_re": out.real.numpy(),
                        f"{tag}_im": out.imag.numpy()})
    records[0]["cases"] = np.array([c[0] for c in CASES])
    records[0]["cases1"] = np.array([c[0] for c in CASES1])
    parts, size = [{}], 0
    for d in records:
        n = sum(v.nbytes for v in d.values())
        if size + n > 900 * 1024:
            parts.append({})
            size = 0
        parts[-1].update(d)
        size += n
    for old in glob.glob(os.path.join(GOLDEN, "einsum*.npz")):
        os.remove(old)
    for k, d in enumerate(parts):
        path = os.path.join(GOLDEN, "einsum.npz" if len(parts) == 1 else f"einsum.part{k}.npz")
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < 1024 * 1024, path
        print(f"{os.path.basename(path)}: {len(d)} arrays, {os.path.getsize(path) / 1024:.1f} KiB on disk")
    print(f"worst float32 deviation of the reference from numpy.einsum: {worst:.2e} of the largest entry")


if __name__ == "__main__":
    main()
