"""The FFT engine (csrc/fft_engine.h through fft.hip and rfft.hip) swept on the GPU: 1. every transform length the engine
is compiled for, direct, four-step and Bluestein, complex and real, each vector against complex128; 2. every route that is
not the packed workgroup -- one vector per workgroup, the fused Bluestein pair at 4096 and 8192 points, four-step and
Bluestein through the workspace -- under every layout, padding, scale and dtype pair, BIT FOR BIT against its own dense
run ("the arithmetic of a vector does not depend on where it lies"), and across the batch seam of the workspace loop and
the 65536th workgroup.  Cases and helpers: fft_sweep_cases.py; reference (torch.fft in complex128 on the CPU) and bounds
(float32 1e-5, float64 1e-11, here per vector; bf16 2^-8 |ref| + 1e-5 max|ref| per entry): fft_cases.py."""
import functools

import pytest
import torch

import fft_cases as fc
import fft_sweep_cases as sc
import rfft_cases as rc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd import rfft as hostrfft

pytestmark = pytest.mark.gpu

WIDE_IDS = [sc.IDS[d] for d in sc.WIDE]
F32_ROUTES = [c for c in sc.ROUTES if c[3] == sc.F32]


def dev(xs):
    return tuple(x.to(DEV) for x in xs)


def same_bits(got, want):
    assert len(got) == len(want)
    return all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


# ---- 1. every compiled size, each vector against complex128 ----------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", sc.FFT_LENGTHS)
def test_fft_at_every_compiled_size(n, dtype):
    v = sc.vectors(n)
    path, vpw = hostfft.plan(n, v, dtype)[:2]
    assert (path, vpw) == sc.expected_fft_plan(n, dtype)
    re, im = fc.gaussian((v, n), dtype, seed=n)
    z = Cplx(re.to(DEV), im.to(DEV))
    ref = fc.c128(re, im)
    e_f = sc.per_vector(cplx.fft(z), torch.fft.fft(ref))
    e_i = sc.per_vector(cplx.ifft(z, norm="forward"), torch.fft.ifft(ref, norm="forward"))
    print(f"fft_sweep c2c n={n} M={fc.transform_size(n)} {sc.IDS[dtype]} {path}: forward {e_f:.3g} inverse {e_i:.3g}")
    assert e_f <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_f, e_i)


@pytest.mark.parametrize("dtype", sc.WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", sc.RFFT_LENGTHS)
def test_rfft_and_irfft_at_every_compiled_size(n, dtype):
    v = sc.vectors(n)
    for c2r in (False, True):
        assert hostrfft.plan(n, v, dtype, c2r)[:4] == sc.expected_rfft_plan(n, dtype)
    path, cn, points, _ = sc.expected_rfft_plan(n, dtype)
    x = rc.real_gaussian((v, n), dtype, seed=n)
    xr, xi = rc.half_spectrum((v, n // 2 + 1), dtype, seed=n + 1)
    assert bool((xi[:, 0] != 0).all()) and bool((xi[:, -1] != 0).all())
    e_f = sc.per_vector(cplx.rfft(x.to(DEV)), torch.fft.rfft(x.double()))
    e_i = sc.per_vector(cplx.irfft(Cplx(xr.to(DEV), xi.to(DEV)), n=n, norm="forward"),
                        torch.fft.irfft(fc.c128(xr, xi), n=n, norm="forward"))
    print(f"fft_sweep real n={n} L={cn} M={points} {sc.IDS[dtype]} {path}: rfft {e_f:.3g} irfft {e_i:.3g}")
    assert e_f <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_f, e_i)


# ---- 2. every route that is not the packed workgroup -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def baseline(kind, n, dtype):
    """(input planes on the device, D): D is the dense, contiguous, last-dim, full-length, scale-1 run of the route's B
    vectors -- computed once, shared and left unchanged"""
    xs = dev(sc.baseline_input(kind, n, dtype))
    return xs, sc.run(kind, xs, n)


def assert_route(case):
    kind, route, n, dtype = case
    path = (hostfft.plan(n, sc.B, dtype) if kind == "c2c" else hostrfft.plan(n, sc.B, dtype, kind == "c2r"))[0]
    vpw = hostfft.plan(n, sc.B, dtype)[1] if kind == "c2c" else hostrfft.plan(n, sc.B, dtype, kind == "c2r")[3]
    assert (path, vpw) == (sc.ROUTE_PLAN[route][0], 1)


@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_dense_run_against_complex128(case):
    kind, _, n, dtype = case
    assert_route(case)
    xs, D = baseline(kind, n, dtype)
    cpu = sc.baseline_input(kind, n, dtype)
    e = sc.per_vector(D, sc.reference(kind, cpu, n))
    other = not sc.default_sign(kind)
    e_o = sc.per_vector(sc.run(kind, xs, n, positive=other), sc.reference(kind, cpu, n, positive=other))
    print(f"fft_sweep dense {sc.route_id(case)}: {e:.3g} other sign {e_o:.3g}")
    assert e <= fc.tol(dtype) and e_o <= fc.tol(dtype), (e, e_o)


@pytest.mark.parametrize("name", sc.LAYOUTS)
@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_layouts_give_the_dense_runs_bits(case, name):
    """element strides (along dim 0, a middle dim, every second element, channels-last, transposed), 1, 2 and 3 batch
    runs and an `expand`ed batch dim: transformed where they lie, and equal to D bit for bit"""
    kind, _, n, dtype = case
    xs, D = baseline(kind, n, dtype)
    runs, copies = sc.LAYOUTS[name]
    views = []
    for x in xs:
        v, dim, unbatch = sc.layout(name, x)
        views.append(v)
    assert sc.takes_no_copy(kind, views, n, dim) and len(sc.runs_of(kind, views[0], n, dim)) == runs
    got = tuple(unbatch(y) for y in sc.run(kind, tuple(views), n, dim=dim))
    assert got[0].shape == (copies, sc.B, sc.out_len(kind, n))
    assert same_bits(got, tuple(d.unsqueeze(0).expand(copies, -1, -1) for d in D))


@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_padding_and_truncation_give_the_dense_runs_bits(case):
    """fewer entries than the transform reads are zeros the loader never loads: the same bits as explicit zeros; more
    entries are never read: the same bits as the narrowed copy (D)"""
    kind, _, n, dtype = case
    xs, D = baseline(kind, n, dtype)
    full = sc.in_len(kind, n)

    def first(x, n_in):
        # dense [B, n_in], the first B rows of a buffer one row longer: a loader that reads an element too many reads a
        # one, not whatever follows the allocation
        buf = torch.ones(sc.B + 1, n_in, dtype=dtype, device=DEV)
        buf[:sc.B] = x[:, :n_in]
        return buf[:sc.B]

    for n_in in (1, full // 2, full - 1):
        short = tuple(first(x, n_in) for x in xs)
        assert short[0].is_contiguous()
        padded = tuple(torch.cat([s, torch.zeros(sc.B, full - n_in, dtype=dtype, device=DEV)], dim=1) for s in short)
        assert same_bits(sc.run(kind, short, n), sc.run(kind, padded, n)), n_in
    longer = tuple(torch.cat([x, torch.ones(sc.B, 5, dtype=dtype, device=DEV)], dim=1) for x in xs)
    assert same_bits(sc.run(kind, longer, n), D)
    # a view of the longer buffer that is already narrow: the vectors lie full + 5 apart
    half = full // 2
    assert same_bits(sc.run(kind, tuple(t[:, :half] for t in longer), n), sc.run(kind, tuple(first(x, half) for x in xs), n))


@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_norms_both_ways_against_complex128(case):
    """norm = "ortho" and "forward": the scale multiplies inside the store (out / fft_scatter and their rfft twins), which
    changes the rounding, so each vector is compared with complex128"""
    kind, _, n, dtype = case
    xs, _ = baseline(kind, n, dtype)
    cpu = sc.baseline_input(kind, n, dtype)
    if kind == "c2c":
        z, ref = Cplx(*xs), fc.c128(*cpu)
        pairs = [(cplx.fft, torch.fft.fft, {}), (cplx.ifft, torch.fft.ifft, {})]
    elif kind == "r2c":
        z, ref = xs[0], cpu[0].double()
        pairs = [(cplx.rfft, torch.fft.rfft, {}), (cplx.ihfft, torch.fft.ihfft, {})]
    else:
        z, ref = Cplx(*xs), fc.c128(*cpu)
        pairs = [(cplx.irfft, torch.fft.irfft, dict(n=n)), (cplx.hfft, torch.fft.hfft, dict(n=n))]
    for ours, theirs, kw in pairs:
        for norm in ("ortho", "forward"):
            e = sc.per_vector(ours(z, norm=norm, **kw), theirs(ref, norm=norm, **kw))
            print(f"fft_sweep norm {sc.route_id(case)} {theirs.__name__} {norm}: {e:.3g}")
            assert e <= fc.tol(dtype), (theirs.__name__, norm, e)


def bf16_check(kind, got, ref):
    if kind == "c2r":
        return rc.bf16_real_violations(got[0], ref)
    return fc.bf16_violations(Cplx(*got), ref)


@pytest.mark.parametrize("case", F32_ROUTES, ids=sc.route_id)
def test_dtype_pairs_round_once(case):
    """bf16 -> float32 (what fft2 and every backward run) equals the float32 transform of the widened values bit for
    bit; bf16 -> bf16 and float32 -> bf16 equal that result rounded once"""
    kind, _, n, _ = case
    narrow = dev(sc.planes(kind, (sc.B, sc.in_len(kind, n)), sc.BF16, seed=3 * n + 1))
    wide = tuple(x.float() for x in narrow)
    F = sc.run(kind, wide, n)
    assert F[0].dtype == sc.F32
    assert same_bits(sc.run(kind, narrow, n, out_dtype=sc.F32), F), "bf16 -> float32"
    once = tuple(f.to(sc.BF16) for f in F)
    ref = sc.reference(kind, wide, n)
    for name, xs in (("bf16 -> bf16", narrow), ("float32 -> bf16", wide)):
        got = sc.run(kind, xs, n, out_dtype=sc.BF16)
        assert same_bits(got, once), name
        bad, worst = bf16_check(kind, got, ref)
        print(f"fft_sweep bf16 {sc.route_id(case)} {name}: worst entry at {worst:.3f} of the bound")
        assert bad == 0, (name, bad, worst)
    # along a strided dim as well: the loaders and stores of every dtype pair take the element stride
    strided = tuple(sc.layout("dim0", x)[0] for x in narrow)
    got = sc.run(kind, strided, n, dim=0, out_dtype=sc.BF16)
    assert same_bits(tuple(y.t() for y in got), once), "bf16 -> bf16 along dim 0"


# ---- the batch seam of the workspace loop ----------------------------------------------------------------------------
def cycled(xs, batch, d):
    """`batch` vectors: the first d of xs, expanded over a leading dim"""
    assert batch % d == 0
    return tuple(x[:d].unsqueeze(0).expand(batch // d, d, x.shape[1]) for x in xs)


@pytest.mark.parametrize("which", [0, 1], ids=["GL+1", "2GL+3"])
@pytest.mark.parametrize("case", sc.SEAMS, ids=sc.seam_id)
def test_workspace_batches_beyond_the_batch_limit(case, which):
    """GL + 1 and 2 GL + 3 vectors: the loop of fft_ws / rfft_run runs a second and a third time with v0 = GL, 2 GL.
    The batch is d distinct vectors expanded, d not a divisor of GL: vector v must have the bits of vector v % d of the
    dense run of those d"""
    kind, n, dtype, GL = case
    batch = sc.seam_batches(GL)[which]
    d = sc.CYCLE[batch]
    assert sc.workspace_bytes(kind, n, GL, dtype) == sc.workspace_bytes(kind, n, batch, dtype)
    xs = dev(sc.planes(kind, (d, sc.in_len(kind, n)), dtype, seed=n + d))
    D = sc.run(kind, xs, n)
    assert sc.per_vector(D, sc.reference(kind, xs, n)) <= fc.tol(dtype)
    views = cycled(xs, batch, d)
    assert sc.takes_no_copy(kind, views, n, 2) and views[0].stride(0) == 0
    got = sc.run(kind, views, n, dim=2)
    assert got[0].shape == (batch // d, d, sc.out_len(kind, n))
    for y, want in zip(got, D):
        assert torch.equal(y, want.unsqueeze(0).expand_as(y))


DISTINCT = [c for c in sc.SEAMS if c[2] == sc.F32 and (c[1] != 4097 or c[0] == "c2c")]


@pytest.mark.parametrize("case", DISTINCT, ids=sc.seam_id)
def test_distinct_vectors_beyond_the_batch_limit_against_complex128(case):
    """once per workspace route (four-step, Bluestein) and primitive: GL + 1 different vectors, each against complex128"""
    kind, n, dtype, GL = case
    cpu = sc.planes(kind, (GL + 1, sc.in_len(kind, n)), dtype, seed=n + 2)
    e = sc.per_vector(sc.run(kind, dev(cpu), n), sc.reference(kind, cpu, n))
    print(f"fft_sweep seam {sc.seam_id(case)} {GL + 1} distinct vectors: {e:.3g}")
    assert e <= fc.tol(dtype), e


# ---- the workgroup count of the one-vector-per-workgroup kernel ------------------------------------------------------
@pytest.mark.parametrize("batch, d", sc.GRID_BATCHES)
@pytest.mark.parametrize("case", sc.GRID_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_one_vector_per_workgroup_grids(case, batch, d):
    kind, n, dtype = case
    xs, D = baseline(kind, n, dtype)
    if batch <= sc.B:
        assert same_bits(sc.run(kind, tuple(x[:batch] for x in xs), n), tuple(y[:batch] for y in D))
        return
    xs7 = dev(sc.planes(kind, (7, sc.in_len(kind, n)), dtype, seed=n + 7))
    D7 = sc.run(kind, xs7, n)
    got = sc.run(kind, cycled(xs7, batch, d), n, dim=2)
    assert got[0].shape == (batch // d, d, sc.out_len(kind, n))
    for y, want in zip(got, D7):
        assert torch.equal(y, want[:d].unsqueeze(0).expand_as(y))
