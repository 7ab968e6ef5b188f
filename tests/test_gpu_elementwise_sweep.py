"""The elementwise layer (csrc/cplxfn.hip, csrc/layout.hip, the elementwise half of csrc/util.hip, csrc/pool.hip) on the GPU
against tests/elementwise_cases.py:
  A. value seams of the eight cplx.* functions (both branches of chsh at 88, the tanh saturation at 11, parts that are
     representable where e^|s| is not, tiny and huge arguments, multiples of pi / 2) against torch complex128 on the CPU,
     modulus-wise (16 u |f| forward, 32 u |f'| |g| backward; bf16 2^-8, 2^-7), per part for the product forms (16 u |part|),
     and a table of signed zeros and infinities;
  B. every streaming kernel over sizes around the vector body, its tail and the second grid-stride trip: the truth (a float64
     formula at the existing test's bound, or the documented float32 chain bit for bit), position independence under
     roll, edge values;  the large sizes repeat a 1027-element pattern and must reproduce the 1027-element result (which
     is compared with the CPU) bit for bit;
  C. no kernel of the util.hip / layout.hip / cplxfn.hip families sees a pointer that is not 16-byte aligned;
  D. abs-max pooling on Gaussian integers (exact ties) over the configuration product, exactly.
Each test prints `SWEEP ...` lines (pytest -s); profiles/elementwise_sweep.txt is a copy of them.

Measured on an MI355X, float32, worst over all functions and families: 4.6 u modulus-wise (tan / tanh), 4.1 u per part
(part_overflow), 10.1 u backward (tan / tanh); bf16 at most 0.996 of its bounds.  What the sweep found, and the library now
handles: parts of exp / sin / cos / sinh / cosh that overflowed where the part is representable; a last-bit difference
between vector body and tail in every float32 backward of cplxfn.hip (fused multiply-adds chosen differently: the file is
now compiled with contraction off); modReLU dropping the NaN of one part (fmaxf); misaligned views reaching 16-byte loads
in the util.hip group; modReLU with a full-shape threshold on an empty input."""
import ctypes

import numpy as np
import pytest
import torch

import elementwise_cases as ec
from gpu_util import DEV
from oracle import cplx_oracle as orc

pytestmark = pytest.mark.gpu

F32T, BF = torch.float32, torch.bfloat16
DTYPES = (F32T, BF)
IDS = ("f32", "bf16")
P = ec.PERIOD


def _cplx():
    from cplxmodule_amd import cplx
    return cplx


def _ops():
    from cplxmodule_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same(a, b):
    """bit-identical, NaNs comparing equal"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return bool(((_bits(a) == _bits(b)) | (a.isnan() & b.isnan())).all())


def _np(t):
    return t.detach().float().cpu().numpy()


def _say(line):
    print("SWEEP " + line)


# ---- A. value seams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fn", ec.FUNCTIONS)
def test_value_seams_against_complex128(fn, dtype):
    cplx, bad = _cplx(), []
    unit = "u" if dtype == F32T else "bound"
    k = (16.0, 32.0) if dtype == F32T else (1.0, 1.0)           # float32 ratios are printed in units of u
    for name in ec.families(fn):
        zr, zi, gr, gi = (t.to(DEV) for t in ec.points(fn, name, dtype))
        zr.requires_grad_(True)
        zi.requires_grad_(True)
        y = getattr(cplx, fn)(cplx.Cplx(zr, zi))
        assert y.real.dtype == dtype
        r = ec.reference(fn, name, dtype)
        worst, part, keep, _ = ec.forward_ratios(fn, dtype, _np(y.real), _np(y.imag), r["f"])
        line = f"A {fn:5s} {IDS[DTYPES.index(dtype)]:4s} {name:14s} modulus {worst * k[0]:7.3f} {unit}  kept {keep:.3f}"
        if part is not None:
            line += f"  part {part * k[0]:7.3f} {unit}  points with a part {ec.has_part(r['f']):.3f}"
        if not (worst <= 1 and keep >= ec.keep_min(fn, name)) or (part is not None and not part <= 1):
            bad.append(line)
        if name == "part_overflow":
            if fn in ec.PRODUCT_FORM and ec.has_part(r["f"]) < ec.part_keep_min(dtype):
                bad.append(line)
        else:                                                   # (there |f'| overflows: the mask would drop the points)
            dr, di = torch.autograd.grad((y.real, y.imag), (zr, zi), (gr, gi))
            assert dr.dtype == dtype
            bw, bk, small = ec.backward_ratios(dtype, _np(dr), _np(di), r)
            line += f"  backward {bw * k[1]:7.3f} {unit}  kept {bk:.3f}"
            if not (bw <= 1 and small and bk >= ec.keep_min(fn, name, backward=True)):
                bad.append(line)
        _say(line)
    assert not bad, "\n".join(bad)


def test_signed_zeros_and_infinities():
    cplx = _cplx()
    table = ec.special_table()
    ref = ec.special_reference(table)
    bad = []
    for fn in ec.FUNCTIONS:
        rows = [i for i, t in enumerate(table) if t[0] == fn]
        if not rows:
            continue
        zr = torch.tensor([table[i][1] for i in rows], dtype=F32T, device=DEV)
        zi = torch.tensor([table[i][2] for i in rows], dtype=F32T, device=DEV)
        zr, zi = torch.cat([zr, zr[:3]]), torch.cat([zi, zi[:3]])          # (some in a vector body, some in the tail)
        y = getattr(cplx, fn)(cplx.Cplx(zr, zi))
        yr, yi = _np(y.real), _np(y.imag)
        for j, i in enumerate(rows):
            if not (ec.same_special(float(yr[j]), ref[i][0]) and ec.same_special(float(yi[j]), ref[i][1])):
                bad.append((table[i], (float(yr[j]), float(yi[j])), ref[i]))
    _say(f"A special values: {len(table)} entries, {len(bad)} differ from torch complex128")
    assert not bad, bad


# ---- B. index space -----------------------------------------------------------------------------------------------------
def _t(a, dtype):
    """numpy float32 pattern -> CPU tensor of dtype"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


def _leaf(x):
    return x.detach().requires_grad_(True)


def _roll(xs, r, n):
    return [torch.roll(x, r * (x.numel() // n)) if isinstance(x, torch.Tensor) and n and x.numel() >= n and x.numel() % n == 0
            else x for x in xs]


def _drive(group, dtype, pats, run, truth, tag):
    """pats: CPU tensors of P (or a multiple of P) elements; run(list of device tensors) -> tuple of elementwise outputs;
    truth(n, outputs) compares a run on the first n elements with the CPU.  Every size of the group."""
    per = None
    for n in ec.sizes(group, dtype):
        xs = [ec.tile_to(p, n * (p.numel() // P)).to(DEV) for p in pats]
        ys = run(xs)
        if n <= P:
            truth(n, ys)
        else:
            if per is None:
                per = run([p.to(DEV) for p in pats])            # the n = P run, just compared with the CPU
            for j, (y, q) in enumerate(zip(ys, per)):
                assert same(y, ec.tile_to(q, y.numel())), (tag, n, "output", j, "differs from the periodic small run")
        if n < 2:
            continue
        for r in ec.ROLLS:
            yr = run(_roll(xs, r, n))
            for j, (a, b) in enumerate(zip(yr, _roll(list(ys), r, n))):
                assert same(a, b), (tag, n, "roll", r, "output", j)
    _say(f"B {tag}: sizes {ec.sizes(group, dtype)[-2:]} and {len(ec.SMALL_SIZES)} small ones, rolls {ec.ROLLS}: ok")


def _exact(got, want32, dtype, what):
    """a device result against a float32 numpy chain rounded once to dtype: bit for bit, NaNs equal"""
    want = _t(want32, dtype).to(DEV)
    assert same(got.reshape(-1), want.reshape(-1)), what


def _f32(x):
    return x.float().numpy() if isinstance(x, torch.Tensor) else x


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fn", ec.FUNCTIONS)
def test_index_space_cplx_fn(fn, dtype):
    cplx = _cplx()
    pats = [_t(ec.pattern(s, scale=sc), dtype) for s, sc in ((1, 2.0), (2, 2.0), (3, 1.0), (4, 1.0))]
    z = torch.complex(pats[0].double(), pats[1].double())
    g = torch.complex(pats[2].double(), pats[3].double())
    d = ec.deriv(fn, z)
    ref = dict(f=getattr(torch, fn)(z).numpy(), d=(d.conj() * g).numpy(), scale=(d.abs() * g.abs()).numpy())

    def run(xs):
        zr, zi = _leaf(xs[0]), _leaf(xs[1])
        y = getattr(cplx, fn)(cplx.Cplx(zr, zi))
        dr, di = torch.autograd.grad((y.real, y.imag), (zr, zi), (xs[2], xs[3]))
        return y.real.detach(), y.imag.detach(), dr, di

    def truth(n, ys):
        yr, yi, dr, di = (_np(t) for t in ys)
        w, part, _, _ = ec.forward_ratios(fn, dtype, yr, yi, ref["f"][:n])
        bw, _, small = ec.backward_ratios(dtype, dr, di, {k: v[:n] for k, v in ref.items()})
        assert w <= 1 and (part is None or part <= 1) and bw <= 1 and small, (fn, n, w, part, bw)

    _drive("cplxfn", dtype, pats, run, truth, f"cplx.{fn} {IDS[DTYPES.index(dtype)]}")


@pytest.mark.parametrize("kind", ["gauss", "edge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["scalar", "one", "full", "scalar_negative"])
def test_index_space_modrelu(variant, dtype, kind):
    """forward: oracle.cplx_oracle.modrelu's float32 chain bit for bit (bf16: the chain on the bf16 values, rounded once);
    backward on the Gaussian inputs: oracle.modrelu_bwd in float64 at tests/test_gpu_extras.py's bounds (2e-5; threshold
    1e-4; bf16 2e-2, its bound for bf16 planes); on the edge values: position independence"""
    cplx = _cplx()
    if kind == "edge":
        zr, zi, tau, _, _, _ = ec.edge_planes(P)
    else:
        zr, zi, tau = ec.pattern(5), ec.pattern(6), ec.pattern(7, scale=0.5)
    pats = [_t(zr, dtype), _t(zi, dtype), _t(ec.pattern(8, scale=1.0), dtype), _t(ec.pattern(9, scale=1.0), dtype), _t(tau, F32T)]
    tau0 = -0.5 if variant == "scalar_negative" else 0.5
    sums = []

    def run(xs):
        a, b = _leaf(xs[0]), _leaf(xs[1])
        if variant.startswith("scalar"):
            t = tau0
        elif variant == "one":
            t = torch.tensor([tau0], device=DEV, requires_grad=True)
        else:
            t = _leaf(xs[4])
        y = cplx.modrelu(cplx.Cplx(a, b), t)
        wrt = (a, b) + ((t,) if isinstance(t, torch.Tensor) else ())
        gs = torch.autograd.grad((y.real, y.imag), wrt, (xs[2], xs[3]))
        if variant == "one":
            sums.append(gs[2])
        return (y.real.detach(), y.imag.detach(), gs[0], gs[1]) + ((gs[2],) if variant == "full" else ())

    def truth(n, ys):
        a, b, gr, gi = (_f32(p)[:n] for p in pats[:4])
        t = pats[4].numpy()[:n] if variant == "full" else np.float32(tau0)
        with np.errstate(all="ignore"):
            yr, yi = orc.modrelu(a, b, t)
        _exact(ys[0], yr, dtype, (variant, kind, n, "re"))
        _exact(ys[1], yi, dtype, (variant, kind, n, "im"))
        if kind == "edge":
            return
        f = np.float64
        ref = orc.modrelu_bwd(gr.astype(f), gi.astype(f), a.astype(f), b.astype(f), np.asarray(t, f))
        tol = 2e-5 if dtype == F32T else 2e-2
        np.testing.assert_allclose(_np(ys[2]), ref["dzr"], rtol=tol, atol=tol)
        np.testing.assert_allclose(_np(ys[3]), ref["dzi"], rtol=tol, atol=tol)
        ttol = 1e-4 if dtype == F32T else 2e-2
        if variant == "full":
            np.testing.assert_allclose(_np(ys[4]), ref["dtau"], rtol=ttol, atol=ttol)
        if variant == "one":
            np.testing.assert_allclose(float(sums[-1]), ref["dtau"].sum(), rtol=ttol, atol=ttol * max(1.0, np.abs(ref["dtau"]).sum()))

    _drive("layout", dtype, pats, run, truth, f"cplx.modrelu {variant} {IDS[DTYPES.index(dtype)]} {kind}")


@pytest.mark.parametrize("kind", ["gauss", "edge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_space_abs(dtype, kind):
    """abs(Cplx): oracle.cplx_oracle.cplx_abs's float32 chain bit for bit; backward against g z / |z| in float64 at
    tests/test_gpu_r02.py's bound (1e-6, 1e-7; bf16: the one rounding of a float32 result, 2^-8), 0 at z = 0"""
    cplx = _cplx()
    zr, zi = ec.edge_planes(P)[:2] if kind == "edge" else (ec.pattern(11), ec.pattern(12))
    pats = [_t(zr, dtype), _t(zi, dtype), _t(ec.pattern(13, scale=1.0), dtype)]

    def run(xs):
        a, b = _leaf(xs[0]), _leaf(xs[1])
        m = abs(cplx.Cplx(a, b))
        da, db = torch.autograd.grad(m, (a, b), xs[2])
        return m.detach(), da, db

    def truth(n, ys):
        a, b, g = (_f32(p)[:n] for p in pats)
        with np.errstate(all="ignore"):
            _exact(ys[0], orc.cplx_abs(a, b), dtype, (kind, n))
        zero = (a == 0) & (b == 0)
        assert (_np(ys[1])[zero] == 0).all() and (_np(ys[2])[zero] == 0).all()
        if kind == "edge":
            return
        f = np.float64
        ra, rb = orc.cplx_abs_bwd(g.astype(f), a.astype(f), b.astype(f))
        rtol, atol = (1e-6, 1e-7) if dtype == F32T else (2.0 ** -8, 1e-30)
        np.testing.assert_allclose(_np(ys[1]), ra, rtol=rtol, atol=atol)
        np.testing.assert_allclose(_np(ys[2]), rb, rtol=rtol, atol=atol)

    _drive("util", dtype, pats, run, truth, f"abs(Cplx) {IDS[DTYPES.index(dtype)]} {kind}")


@pytest.mark.parametrize("kind", ["gauss", "edge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("div", [False, True], ids=["mul", "div"])
def test_index_space_mul_div(div, dtype, kind):
    """Cplx * Cplx and Cplx / Cplx: the float32 chain of csrc/layout.hip (ec.mul_chain) bit for bit, forward and -- float32
    -- both gradients (the same kernel on g, conj(b) and the saved quotient); bf16 gradients, whose intermediate is rounded
    between two launches, within 2^-6 of the complex128 gradient on the Gaussian inputs.  The edge table locks in the
    quotient that becomes 0 or NaN when c^2 + d^2 overflows or underflows."""
    cplx = _cplx()
    if kind == "edge":
        zr, zi, _, wr, wi, _ = ec.edge_planes(P)
    else:
        zr, zi, wr, wi = (ec.pattern(s) for s in (21, 22, 23, 24))
    pats = [_t(a, dtype) for a in (zr, zi, wr, wi, ec.pattern(25, scale=1.0), ec.pattern(26, scale=1.0))]

    def run(xs):
        a, b, c, d = (_leaf(x) for x in xs[:4])
        y = cplx.Cplx(a, b) / cplx.Cplx(c, d) if div else cplx.Cplx(a, b) * cplx.Cplx(c, d)
        gs = torch.autograd.grad((y.real, y.imag), (a, b, c, d), (xs[4], xs[5]))
        return (y.real.detach(), y.imag.detach()) + tuple(gs)

    def truth(n, ys):
        if n == 0:
            return                                  # (an empty product keeps torch's elementwise kernels: cplx_mul_ok)
        a, b, c, d, gr, gi = (_f32(p)[:n] for p in pats)
        yr, yi = ec.mul_chain(a, b, c, d, div)
        _exact(ys[0], yr, dtype, (div, kind, n, "re"))
        _exact(ys[1], yi, dtype, (div, kind, n, "im"))
        if dtype == F32T:
            if div:                                 # da = g / conj(b);  db = -(g conj(y)) / conj(b)
                da = ec.mul_chain(gr, gi, c, -d, True)
                t = ec.mul_chain(gr, gi, yr, -yi, False)
                db = ec.mul_chain(t[0], t[1], c, -d, True)
                db = (-db[0], -db[1])
            else:                                   # da = g conj(b);  db = g conj(a)
                da, db = ec.mul_chain(gr, gi, c, -d), ec.mul_chain(gr, gi, a, -b)
            for got, want, what in zip(ys[2:], da + db, ("da re", "da im", "db re", "db im")):
                _exact(got, want, dtype, (div, kind, n, what))
        elif kind == "gauss":
            f = np.float64
            z, w, g = a.astype(f) + 1j * b, c.astype(f) + 1j * d, gr.astype(f) + 1j * gi
            da, db = (g / w.conj(), -(g * (z / w).conj()) / w.conj()) if div else (g * w.conj(), g * z.conj())
            for (gre, gim), want in ((ys[2:4], da), (ys[4:6], db)):
                err = np.abs((_np(gre) + 1j * _np(gim)) - want)
                assert (err <= 2.0 ** -6 * np.abs(want)).all(), (div, n, float((err / np.abs(want)).max()))

    _drive("layout", dtype, pats, run, truth, f"Cplx {'/' if div else '*'} Cplx {IDS[DTYPES.index(dtype)]} {kind}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_space_split_relu(dtype):
    """torch's ReLU on both planes and its backward on the saved output, exactly, on the edge values (NaN passes)"""
    ops = _ops()
    zr, zi = ec.edge_planes(P)[:2]
    zr = np.where(np.arange(P) % 3 == 0, -zr, zr)            # (negative values of every kind as well)
    pats = [_t(a, dtype) for a in (zr, zi, ec.pattern(31, scale=1.0), ec.pattern(32, scale=1.0))]

    def run(xs):
        a, b = _leaf(xs[0]), _leaf(xs[1])
        yr, yi = ops.split_relu(a, b)
        da, db = torch.autograd.grad((yr, yi), (a, b), (xs[2], xs[3]))
        return yr.detach(), yi.detach(), da, db

    def truth(n, ys):
        a, b, gr, gi = (_f32(p)[:n] for p in pats)
        ya, yb = ec.split_relu_chain(a), ec.split_relu_chain(b)
        _exact(ys[0], ya, dtype, (n, "re"))
        _exact(ys[1], yb, dtype, (n, "im"))
        with np.errstate(invalid="ignore"):
            _exact(ys[2], np.where(ya <= 0, np.float32(0), gr), dtype, (n, "d re"))
            _exact(ys[3], np.where(yb <= 0, np.float32(0), gi), dtype, (n, "d im"))

    _drive("layout", dtype, pats, run, truth, f"ops.split_relu {IDS[DTYPES.index(dtype)]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_space_interleave(dtype):
    """cplx.from_interleaved_real / to_interleaved_real: permutations, exactly (values and gradients)"""
    cplx = _cplx()
    x = np.stack([ec.edge_planes(P)[0], ec.pattern(41)], axis=-1).reshape(-1)         # 2 P reals
    pats = [_t(x, dtype), _t(ec.pattern(42), dtype), _t(ec.pattern(43), dtype)]

    def run(xs):
        v = _leaf(xs[0])
        z = cplx.from_interleaved_real(v, True, -1)
        back = cplx.to_interleaved_real(z, True, -1)
        (dv,) = torch.autograd.grad((z.real, z.imag), v, (xs[1], xs[2]), retain_graph=True)
        return z.real.detach(), z.imag.detach(), back.detach(), dv

    def truth(n, ys):
        v, gr, gi = (_f32(p) for p in pats)
        re, im = orc.from_interleaved_real(v[:2 * n])
        _exact(ys[0], re, dtype, (n, "re"))
        _exact(ys[1], im, dtype, (n, "im"))
        _exact(ys[2], v[:2 * n], dtype, (n, "back"))
        _exact(ys[3], orc.to_interleaved_real(gr[:n], gi[:n]), dtype, (n, "grad"))

    _drive("layout", dtype, pats, run, truth, f"interleaved converters {IDS[DTYPES.index(dtype)]}")


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_space_abs2_cast_mask_mul(dtype, out_dtype):
    """ops.abs2 (one and two planes), ops.cast and ops.mask_mul (one and two planes) for one in / out dtype pair: the float32
    operation(s), one rounding each (x x + y y: three), rounded once more to the output dtype, bit for bit"""
    ops = _ops()
    zr, zi, _, _, _, mask = ec.edge_planes(P)
    pats = [_t(zr, dtype), _t(zi, dtype), _t(mask, F32T)]

    def run(xs):
        a, b, m = xs
        out = (ops.abs2(a, b, out_dtype=out_dtype), ops.abs2(a, None, out_dtype=out_dtype), ops.cast(a, out_dtype))
        return out + ops.mask_mul(a, b, m, out_dtype=out_dtype) + ops.mask_mul(b, None, m, out_dtype=out_dtype)[:1]

    def truth(n, ys):
        a, b, m = (_f32(p)[:n] for p in pats)
        with np.errstate(all="ignore"):
            want = (ec.abs2_chain(a, b), ec.abs2_chain(a), a, a * m, b * m, b * m)
        for j, (got, w) in enumerate(zip(ys, want)):
            assert got.dtype == out_dtype
            _exact(got, w, out_dtype, (n, j))

    _drive("util", dtype, pats, run, truth, f"ops.abs2 / cast / mask_mul {IDS[DTYPES.index(dtype)]} -> {IDS[DTYPES.index(out_dtype)]}")


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
def test_index_space_exp(out_dtype):
    """ops.exp (float32 in): the device expf is within 1 ulp, so 2 u of the float64 value (bf16 out: one more rounding, 2^-8),
    over the whole range where the result is a normal number, +-inf and NaN included"""
    ops = _ops()
    x = ec.pattern(51, scale=30.0)
    x[:8] = [0.0, -0.0, 88.7, -87.0, np.inf, -np.inf, np.nan, 1e-40]
    pats = [_t(x, F32T)]

    def truth(n, ys):
        v = pats[0].numpy()[:n].astype(np.float64)
        with np.errstate(all="ignore"):
            ref = np.exp(v)
        got = _np(ys[0]).astype(np.float64)
        fin = np.isfinite(ref) & (ref > 1.2e-38) & (ref < 3.3e38)
        rel = 2 * ec.U if out_dtype == F32T else 2.0 ** -8
        assert (np.abs(got[fin] - ref[fin]) <= rel * ref[fin]).all()
        assert np.array_equal(np.isnan(got), np.isnan(v)) and (got[v == np.inf] == np.inf).all() and (got[v == -np.inf] == 0).all()

    _drive("util", F32T, pats, lambda xs: (ops.exp(xs[0], out_dtype=out_dtype),), truth, f"ops.exp -> {IDS[DTYPES.index(out_dtype)]}")


@pytest.mark.parametrize("ga_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_index_space_lrt_dx_accum(dtype, ga_dtype):
    """dx += 2 x ga, one fused multiply-add per element: within half an ulp of the float64 value, 2^-24 |ref|; bf16 planes round
    that once more, by less than 2^-8 / (1 + 2^-8) of it: 2^-8 |ref| in all"""
    ops = _ops()
    pats = [_t(ec.pattern(s), dtype) for s in (61, 62, 63, 64)] + [_t(ec.pattern(65), ga_dtype)]

    def run(xs):
        dr, di = xs[0].clone(), xs[1].clone()
        ops.lrt_dx_accum(dr, di, xs[2], xs[3], xs[4])
        d1 = xs[0].clone()
        ops.lrt_dx_accum(d1, None, xs[2], None, xs[4])           # the real layers' form
        return dr, di, d1

    def truth(n, ys):
        d0, d1, xr, xi, ga = (_f32(p)[:n].astype(np.float64) for p in pats)
        rel = 2.0 ** -24 if dtype == F32T else 2.0 ** -8
        for got, ref in zip(ys, (d0 + 2 * xr * ga, d1 + 2 * xi * ga, d0 + 2 * xr * ga)):
            assert (np.abs(_np(got) - ref) <= rel * np.abs(ref) * (1 + 1e-9) + 1e-45).all(), n

    _drive("util", dtype, pats, run, truth, f"ops.lrt_dx_accum {IDS[DTYPES.index(dtype)]}, ga {IDS[DTYPES.index(ga_dtype)]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_mask_matches_the_oracle_at_every_size(dtype):
    """position-dependent by design: the keep mask is oracle.cplx_oracle.cplx_dropout_mask at every size, the last, partly
    filled Philox group included; kept values are x / (1 - p), exactly for p = 0.5"""
    from cplxmodule_amd.nn.relevance import noise
    cplx = _cplx()
    for n in ec.sizes("layout", dtype):
        noise.manual_seed(77)
        zr = (torch.rand(n, device=DEV) + 0.5).to(dtype)
        zi = (torch.rand(n, device=DEV) + 0.5).to(dtype)
        y = cplx.dropout(cplx.Cplx(zr, zi), 0.5)
        keep = torch.from_numpy(orc.cplx_dropout_mask(n, 0.5, seed=77, offset=noise.counter)).to(DEV)
        assert y.real.shape == (n,)
        assert torch.equal(y.real != 0, keep) and torch.equal(y.imag != 0, keep), n
        assert torch.equal(y.real[keep], 2 * zr[keep]) and torch.equal(y.imag[keep], 2 * zi[keep]), n
    _say(f"B cplx.dropout {IDS[DTYPES.index(dtype)]}: mask = oracle at sizes {ec.sizes('layout', dtype)}")


# ---- C. alignment -------------------------------------------------------------------------------------------------------
def _misaligned(x):
    """a contiguous view that starts one element into an aligned buffer"""
    return torch.cat([x.new_zeros(1), x.reshape(-1)])[1:]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_misaligned_views_never_reach_a_kernel(dtype, monkeypatch):
    """every wrapper of B on contiguous buf[1:] views: each plane pointer that reaches the library is 16-byte aligned (the
    wrappers re-home the view), the values equal those of the aligned copy bit for bit, gradients flow back to the view"""
    cplx, ops = _cplx(), _ops()
    from cplxmodule_amd.nn.relevance import noise
    n = 37
    seen, real_call = [], ops.call

    def spy(name, *args):
        for j, a in enumerate(args[:-1]):                       # (the last argument is the stream)
            if isinstance(a, ctypes.c_void_p) and a.value and a.value % 16:
                seen.append((name, j, "misaligned"))
        seen.append((name, -1, "call"))
        return real_call(name, *args)

    monkeypatch.setattr(ops, "call", spy)
    x = [_t(ec.pattern(70 + j), dtype).to(DEV)[:n] for j in range(6)]
    x2 = _t(ec.pattern(80, n=2 * P), dtype).to(DEV)[:2 * n]
    tau = torch.rand(n, device=DEV)
    mask = (torch.rand(n, device=DEV) < 0.5).float()
    x32 = x[0].float()

    def fn_of(name):
        def run(a, b, gr, gi):
            a, b = _leaf(a), _leaf(b)
            y = getattr(cplx, name)(cplx.Cplx(a, b))
            return (y.real.detach(), y.imag.detach()) + torch.autograd.grad((y.real, y.imag), (a, b), (gr, gi))
        return run

    def modrelu(a, b, gr, gi, t):
        a, b, t = _leaf(a), _leaf(b), _leaf(t)
        y = cplx.modrelu(cplx.Cplx(a, b), t)
        return (y.real.detach(), y.imag.detach()) + torch.autograd.grad((y.real, y.imag), (a, b, t), (gr, gi))

    def absz(a, b, g):
        a, b = _leaf(a), _leaf(b)
        m = abs(cplx.Cplx(a, b))
        return (m.detach(),) + torch.autograd.grad(m, (a, b), g)

    def abs2fn(a, b, g):
        a, b = _leaf(a), _leaf(b)
        m = ops.Abs2Fn.apply(a, b)
        return (m.detach(),) + torch.autograd.grad(m, (a, b), g)

    def muldiv(div):
        def run(a, b, c, d, gr, gi):
            a, b, c, d = (_leaf(t) for t in (a, b, c, d))
            y = cplx.Cplx(a, b) / cplx.Cplx(c, d) if div else cplx.Cplx(a, b) * cplx.Cplx(c, d)
            return (y.real.detach(), y.imag.detach()) + torch.autograd.grad((y.real, y.imag), (a, b, c, d), (gr, gi))
        return run

    def relu(a, b, gr, gi):
        a, b = _leaf(a), _leaf(b)
        y = ops.split_relu(a, b)
        return (y[0].detach(), y[1].detach()) + torch.autograd.grad(y, (a, b), (gr, gi))

    def deint(v, gr, gi):
        v = _leaf(v)
        z = cplx.from_interleaved_real(v, True, -1)
        return (z.real.detach(), z.imag.detach()) + torch.autograd.grad((z.real, z.imag), v, (gr, gi))

    def inter(a, b, g):
        a, b = _leaf(a), _leaf(b)
        out = cplx.to_interleaved_real(cplx.Cplx(a, b), True, -1)
        return (out.detach(),) + torch.autograd.grad(out, (a, b), g)

    def dropout(a, b, gr, gi):
        noise.manual_seed(5)
        a, b = _leaf(a), _leaf(b)
        y = cplx.dropout(cplx.Cplx(a, b), 0.5)
        return (y.real.detach(), y.imag.detach()) + torch.autograd.grad((y.real, y.imag), (a, b), (gr, gi))

    def accum(d0, d1, a, b, g):
        d0, d1 = _misaligned(d0) if d0.data_ptr() % 16 else d0.clone(), _misaligned(d1) if d1.data_ptr() % 16 else d1.clone()
        ops.lrt_dx_accum(d0, d1, a, b, g)                       # in place, also on a misaligned accumulator
        return d0, d1

    other = BF if dtype == F32T else F32T
    cases = [(f"cplx.{f}", fn_of(f), x[:4]) for f in ec.FUNCTIONS] + [
        ("modrelu", modrelu, x[:4] + [tau]), ("abs", absz, x[:3]), ("Abs2Fn", abs2fn, x[:3]),
        ("mul", muldiv(False), x[:6]), ("div", muldiv(True), x[:6]), ("split_relu", relu, x[:4]),
        ("deinterleave", deint, [x2, x[0], x[1]]), ("interleave", inter, [x[0], x[1], x2]), ("dropout", dropout, x[:4]),
        ("abs2", lambda a, b: (ops.abs2(a, b), ops.abs2(a, None, out_dtype=other)), x[:2]),
        ("modulus", lambda a, b: (ops.modulus(a, b),), x[:2]),
        ("cast", lambda a: (ops.cast(a, other),), x[:1]),
        ("mask_mul", lambda a, b, m: ops.mask_mul(a, b, m) + ops.mask_mul(a, None, m, out_dtype=other)[:1], x[:2] + [mask]),
        ("exp", lambda a: (ops.exp(a), ops.exp(a, out_dtype=BF)), [x32]),
        ("lrt_dx_accum", accum, x[:5]),
    ]
    for name, run, args in cases:
        want = run(*args)
        del seen[:]
        views = [_misaligned(a) for a in args]
        assert all(v.data_ptr() % 16 and v.is_contiguous() for v in views)
        got = run(*views)
        assert [s for s in seen if s[2] == "call"], name                    # the library was called
        assert not [s for s in seen if s[2] == "misaligned"], (name, seen)
        assert len(got) == len(want)
        for j, (a, b) in enumerate(zip(got, want)):
            assert b is not None and same(a, b), (name, j)
    _say(f"C {len(cases)} wrappers on misaligned {IDS[DTYPES.index(dtype)]} views: aligned pointers only, same bits, gradients flow")


# ---- D. abs-max pooling -------------------------------------------------------------------------------------------------
def test_max_pool2d_on_gaussian_integers_is_exact():
    """values, selected positions (the index plane saved for the backward) and both gradients against F.max_pool2d(|z|, return_indices=True) on the CPU plus two gathers -- |z| in float32 in the form
    oracle.cplx_oracle.cplx_abs states; for bf16 planes the modulus is taken in float32 of the bf16 values, as the kernel
    does (Gaussian integers up to 5 are bf16 numbers, so the reference is the same).  Planar and channels-last, float32 and
    bf16, with and without NaNs, every configuration torch accepts."""
    cplx = _cplx()
    cfgs = ec.pool_configs()
    runs = 0
    for nan in (False, True):
        zr, zi = ec.pool_planes(nan)
        for cfg in cfgs:
            yr, yi, idx, gr, gi, dzr, dzi = ec.pool_reference(zr, zi, cfg)
            k, s, p, d, ceil = cfg
            for dtype in DTYPES:
                for fmt in (torch.contiguous_format, torch.channels_last):
                    dev = lambda t: t.to(DEV).to(dtype).contiguous(memory_format=fmt)  # noqa: E731
                    a, b = _leaf(dev(torch.from_numpy(zr))), _leaf(dev(torch.from_numpy(zi)))
                    y = cplx.max_pool2d(cplx.Cplx(a, b), k, s, p, d, ceil)
                    what = (cfg, dtype, fmt, nan)
                    assert same(y.real.detach().contiguous(), yr.to(dtype).to(DEV)), what
                    assert same(y.imag.detach().contiguous(), yi.to(dtype).to(DEV)), what
                    (sel,) = y.real.grad_fn.saved_tensors       # the index plane the backward gathers by
                    assert torch.equal(sel.long().contiguous().cpu(), idx), what
                    da, db = torch.autograd.grad((y.real, y.imag), (a, b), (dev(gr), dev(gi)))
                    assert same(da.contiguous(), dzr.to(dtype).to(DEV)) and same(db.contiguous(), dzi.to(dtype).to(DEV)), what
                    runs += 1
    assert runs == 2 * len(cfgs) * 4
    _say(f"D max_pool2d: {len(cfgs)} configurations x planar / channels-last x float32 / bf16 x with / without NaN: exact")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_max_pool1d_and_3d_see_ties(dtype):
    """the composition layers on Gaussian integers: max_pool1d against F.max_pool1d(|z|) + gathers, max_pool3d against
    oracle.cplx_oracle.cplx_max_pool3d (first maximum in (d, h, w) order), two configurations each, exactly"""
    cplx = _cplx()
    rs = np.random.RandomState(23)
    zr, zi = rs.randint(-5, 6, (2, 3, 19)).astype(np.float32), rs.randint(-5, 6, (2, 3, 19)).astype(np.float32)
    mod = torch.from_numpy(orc.cplx_abs(zr, zi))
    for k, s, p, d, ceil in ((3, 2, 1, 1, False), (2, 1, 0, 2, True)):
        _, idx = torch.nn.functional.max_pool1d(mod, k, s, p, d, ceil, return_indices=True)
        y = cplx.max_pool1d(cplx.Cplx(torch.from_numpy(zr).to(DEV).to(dtype), torch.from_numpy(zi).to(DEV).to(dtype)), k, s, p, d, ceil)
        assert same(y.real, torch.from_numpy(zr).gather(2, idx).to(dtype).to(DEV)), (k, s, p, d, ceil)
        assert same(y.imag, torch.from_numpy(zi).gather(2, idx).to(dtype).to(DEV)), (k, s, p, d, ceil)
    zr, zi = rs.randint(-5, 6, (2, 2, 5, 6, 7)).astype(np.float32), rs.randint(-5, 6, (2, 2, 5, 6, 7)).astype(np.float32)
    for k, s, p, d, ceil in ((2, 2, 0, 1, False), ((3, 2, 3), (1, 2, 2), (1, 1, 1), 1, True)):
        want = orc.cplx_max_pool3d(zr, zi, k, s, p, d, ceil)
        y = cplx.max_pool3d(cplx.Cplx(torch.from_numpy(zr).to(DEV).to(dtype), torch.from_numpy(zi).to(DEV).to(dtype)), k, s, p, d, ceil)
        assert same(y.real, torch.from_numpy(want[0]).to(dtype).to(DEV)) and same(y.imag, torch.from_numpy(want[1]).to(dtype).to(DEV)), (k, s)
    _say(f"D max_pool1d / max_pool3d {IDS[DTYPES.index(dtype)]}: exact on Gaussian integers")
