"""The Welch kernels (csrc/spectrum.hip) swept on the GPU over the indexing their other tests never reach: 2. integer planes
through one-, two- and four-point transforms, bit for bit, forward and gradient, over every seam of the segment chunks (G >
1, a part chunk, fewer chunks than planned, one chunk) and of the gather (step 1, n - 1, n, n + 3; samples under 1 .. n
segments and under none), in float32, bf16 and float64 planes, and every layout against the contiguous call's bits; 3. the
real transforms, each ROW against complex128, on the fused routes with a part chunk and on the workspace route with several
batches and a batch that ends inside a row, forward and gradient with a different g per row; 4. the linear power of channels
40, 60 and 80 dB below the main one through bandwidth_power and acpr_calc.  Cases, reference (the reference's formula in
complex128 on the CPU, autograd through it) and bounds: welch_sweep_cases.py; test_welch_sweep_host.py shows that every
case crosses its seam and that complex64 on the CPU keeps a quarter of each float32 bound."""
import pytest
import torch

import welch_sweep_cases as wc
from gpu_util import DEV

from cplxmodule_amd import spectrum as hs

pytestmark = pytest.mark.gpu

EXACT = wc.exact_cases()


def compute(dtype):
    return wc.F64 if dtype == wc.F64 else wc.F32


def planes(x, dtype):
    """the planes of a complex128 CPU tensor on the device in `dtype`; the values must survive the rounding"""
    pr, pi = x.real.to(dtype).to(DEV), x.imag.to(dtype).to(DEV)
    assert torch.equal(pr.double().cpu(), x.real) and torch.equal(pi.double().cpu(), x.imag)
    return pr, pi


def welch(pr, pi, w, step, fs, scaling, g=None):
    """-> (Pxx, gradient as complex128 on the CPU or None) of planes [rows, T]"""
    if g is None:
        return hs.welch(pr, pi, 1, w, fs, scaling, step), None
    pr, pi = pr.detach().requires_grad_(True), pi.detach().requires_grad_(True)
    p = hs.welch(pr, pi, 1, w, fs, scaling, step)
    gr, gi = torch.autograd.grad(p, (pr, pi), grad_outputs=g)
    assert gr.dtype == pr.dtype and gi.dtype == pr.dtype
    return p.detach(), torch.complex(gr.double().cpu(), gi.double().cpu())


# ---- 2. integer planes: bit-exact forward and gradient ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", wc.EXACT_DTYPES, ids=[wc.IDS[d] for d in wc.EXACT_DTYPES])
@pytest.mark.parametrize("case", EXACT, ids=wc.exact_id)
def test_integer_planes_are_exact(case, dtype):
    rows, S, n, step = case
    x, g, w, pxx_acc, grad_acc, k = wc.exact_reference(case)
    scaling, fs = wc.exact_scaling(case)
    cdt = compute(dtype)
    assert hs.plan(n, rows, S, dtype) == wc.expected_plan(n, rows, S, dtype)
    pr, pi = planes(x, dtype)
    p, grad = welch(pr, pi, w.to(cdt).to(DEV), step, fs, scaling, g.to(cdt).to(DEV))
    assert p.dtype == cdt and p.shape == (rows, n) and grad.shape == x.shape
    p, grad = p.cpu(), torch.view_as_real(grad)
    acc, gacc = pxx_acc.round(), torch.view_as_real(grad_acc).round()
    if wc.is_strict(case):
        # 1 / (S scale) is a power of two: the reference, rounded once, is the only right answer
        assert torch.equal(p, (acc / k).to(cdt))
        assert torch.equal(grad, (gacc * (2 / k)).to(dtype).double())
    else:
        # the factor is rounded: the integer accumulator must come back
        assert torch.equal((p.double() * k).round(), acc)
        if dtype != wc.BF16:
            assert torch.equal((grad * (k / 2)).round(), gacc)
        else:
            # the gradient is stored as bf16: the rounding of the float32 value, which lies within three float32
            # roundings of the reference -- the reference rounded once, unless it lies that close to a bf16 tie
            ref = gacc * (2 / k)
            lo, hi = (ref * (1 - 2.0 ** -22)).to(wc.BF16).double(), (ref * (1 + 2.0 ** -22)).to(wc.BF16).double()
            assert bool(((grad == lo) | (grad == hi)).all())
    cov = wc.coverage(wc.exact_length(case), n, step)
    assert bool((grad[:, cov == 0] == 0).all())           # samples that no segment covers: exactly 0


@pytest.mark.parametrize("n", [128, 100], ids=["direct-128", "bluestein-100"])
def test_layouts_give_the_contiguous_calls_bits(n, monkeypatch):
    """each layout is one cplxamd_welch_fwd (and one _bwd) that reads the caller's own planes, except where the dims other
    than time do not collapse into one row stride (copied first); the bits are the contiguous call's either way"""
    R, T, step = wc.LAYOUT_ROWS, wc.LAYOUT_T, 37
    x = torch.complex(wc.gaussian((R, T), n).float(), wc.gaussian((R, T), n + 1).float()).to(DEV).requires_grad_(True)
    w = torch.hamming_window(n, periodic=False, device=DEV)
    g = wc.gaussian((R, n), n + 2).float().to(DEV)
    calls = []

    def recording(name, *args):
        calls.append((name,) + tuple(v.value for v in args[:2]))
        return orig(name, *args)

    orig = hs.call
    monkeypatch.setattr(hs, "call", recording)
    base = hs.welch(x.real.contiguous(), x.imag.contiguous(), 1, w, 2.0, "density", step)
    (base_grad,) = torch.autograd.grad(base, x, grad_outputs=g)
    assert [c[0] for c in calls] == ["cplxamd_welch_fwd", "cplxamd_welch_bwd"]
    for name, copies in wc.LAYOUTS.items():
        pr, pi, dim, unbatch = wc.layout(name, x)
        del calls[:]
        p = unbatch(hs.welch(pr, pi, dim, w, 2.0, "density", step))
        (grad,) = torch.autograd.grad(p, x, grad_outputs=g)
        assert [c[0] for c in calls] == ["cplxamd_welch_fwd", "cplxamd_welch_bwd"], name
        for c in calls:
            assert (c[1:] != (pr.data_ptr(), pi.data_ptr())) == copies, name
        assert torch.equal(p, base), name
        assert torch.equal(torch.view_as_real(grad), torch.view_as_real(base_grad)), name


# ---- 3. the real transforms, per row ---------------------------------------------------------------------------------
FWD_RUNS, BWD_RUNS = wc.tol_runs(4), wc.tol_runs(5)


@pytest.mark.parametrize("run", FWD_RUNS, ids=wc.tol_id)
def test_pxx_per_row_across_chunks_and_batches(run):
    (name, n, rows, S, _, _), dtype = run
    narrow = dtype == wc.BF16
    x, w, _ = wc.tol_input(name, narrow)
    assert hs.plan(n, rows, S, dtype) == wc.expected_plan(n, rows, S, dtype)
    pr, pi = planes(x, dtype)
    p, _ = welch(pr, pi, w.to(compute(dtype)).to(DEV), 1, wc.TOL_FS, wc.TOL_SCALING)
    assert p.shape == (rows, n) and p.dtype == compute(dtype)
    e = wc.per_row(p, wc.tol_pxx(name, narrow))
    print(f"welch_sweep pxx {wc.tol_id(run)} {hs.plan(n, rows, S, dtype)[0]}: {e:.3g} of {wc.PXX_TOL[dtype]:.0e}")
    assert e <= wc.PXX_TOL[dtype]


@pytest.mark.parametrize("run", BWD_RUNS, ids=wc.tol_id)
def test_gradient_per_row_across_chunks_and_batches(run):
    (name, n, rows, S, _, _), dtype = run
    narrow = dtype == wc.BF16
    x, w, g = wc.tol_input(name, narrow)
    assert hs.plan(n, rows, S, dtype) == wc.expected_plan(n, rows, S, dtype)
    assert not bool((g[0] == g[1]).any())                 # a different g per row: a wrong row index changes the result
    pr, pi = planes(x, dtype)
    cdt = compute(dtype)
    _, grad = welch(pr, pi, w.to(cdt).to(DEV), 1, wc.TOL_FS, wc.TOL_SCALING, g.to(cdt).to(DEV))
    ref = wc.tol_grad(name, narrow)
    e = wc.per_row(grad, ref)
    if narrow:
        ratio = wc.bf16_grad_ratio(grad, ref)
        print(f"welch_sweep grad {wc.tol_id(run)}: worst entry at {ratio:.3f} of the bf16 bound (norm-wise {e:.3g})")
        assert ratio <= 1.0
    else:
        print(f"welch_sweep grad {wc.tol_id(run)}: {e:.3g} of {wc.GRAD_TOL[dtype]:.0e}")
        assert e <= wc.GRAD_TOL[dtype]


# ---- 4. weak bands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", wc.BAND_DTYPES, ids=[wc.IDS[d] for d in wc.BAND_DTYPES])
@pytest.mark.parametrize("fn, nperseg", wc.BAND_RUNS)
def test_weak_bands_keep_their_own_power(fn, nperseg, dtype):
    from cplxmodule_amd.utils import spectrum as sp
    x = wc.band_signal()
    sig = torch.stack(planes(x, dtype), dim=-1)           # [2, T, 2]
    ov, scaling = wc.band_run_params(fn, nperseg)
    ref = wc.band_ref_pxx(x, nperseg, ov, scaling)
    pb, ptot = wc.band_powers(ref, nperseg), ref.sum(-1, keepdim=True)
    bound = wc.band_bound(pb, ptot, wc.BAND_EPS[dtype])
    got = {}
    if fn == "bandwidth_power":
        _, px, db = sp.bandwidth_power(sig, wc.BAND_FS, wc.band_edges(0) + wc.band_edges(1), nperseg=nperseg)
        assert px.dtype == dtype and db.shape == (2, 8)
        got["spectrum"] = wc.band_powers(px, nperseg)
        got["decibels"] = torch.stack([10 ** (db[r, 4 * r:4 * r + 4].double().cpu() / 10) for r in range(2)])
    else:
        rows = []
        for r, (mcf, acf) in enumerate(wc.BAND_ROWS):
            m, a = sp.acpr_calc(sig, wc.BAND_FS, mcf + wc.BAND_OFFSET, wc.BAND_MCB, acf=[f + wc.BAND_OFFSET for f in acf],
                                acb=wc.BAND_ACB, nperseg=nperseg)
            assert m.shape == (2, 1) and a.shape == (2, 3) and m.dtype == dtype
            rows.append(10 ** (torch.cat([m[r], a[r]]).double().cpu() / 10))
        got["decibels"] = torch.stack(rows)
    for what, p in got.items():
        ratio = (p - pb).abs() / bound
        print(f"welch_sweep bands {fn} n={nperseg} {wc.IDS[dtype]} {what}: error / bound per band (main, -40, -60, -80 dB) "
              f"{[f'{v:.3g}' for v in ratio.flatten().tolist()]}")
        assert float(ratio.max()) <= 1.0, what
