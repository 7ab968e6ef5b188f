"""The Welch sweep without a GPU: the library's plan is pinned to the rule welch_sweep_cases.py restates (path and both
workspace sizes, for every case), every case crosses the seam it claims, the integer cases are integers below 2^20, and the
complex64 CPU formula stays within a quarter of every float32 bound the GPU test asserts (the reference-only headroom)."""
import pytest
import torch

import welch_sweep_cases as wc
from cplxmodule_amd import spectrum as hs

EXACT = wc.exact_cases()


def all_plan_cases():
    """(n, rows, S, dtype) of every GPU run of the sweep"""
    out = [(n, rows, S, d) for rows, S, n, _ in EXACT for d in wc.EXACT_DTYPES]
    out += [(c[1], c[2], c[3], d) for c in wc.TOL_CASES for d in set(c[4]) | set(c[5])]
    for fn, n in wc.BAND_RUNS:
        ov, _ = wc.band_run_params(fn, n)
        out += [(n, 2, (wc.BAND_T - n) // (n - ov) + 1, d) for d in wc.BAND_DTYPES]
    return sorted(set(out), key=lambda c: (c[0], c[1], c[2], wc.IDS[c[3]]))


# ---- the plan --------------------------------------------------------------------------------------------------------
def test_the_library_plans_what_the_restated_rule_implies():
    cases = all_plan_cases()
    assert len(cases) > 100
    for n, rows, S, dtype in cases:
        assert hs.plan(n, rows, S, dtype) == wc.expected_plan(n, rows, S, dtype), (n, rows, S, dtype)


@pytest.mark.parametrize("n", [1, 2, 3, 500, 4095, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 1 << 20])
def test_the_restated_rule_over_a_grid_of_shapes(n):
    """beyond the cases: the rule at the ends of every size class, at row counts round 2048 and at vector counts round GL"""
    for dtype in (wc.F32, wc.F64, wc.BF16):
        GL = wc.batch_limit(n, dtype)
        for rows in (1, 2, 3, 700, 2047, 2048, 2049):
            for S in (1, 2, 5, 683, 2049, GL - 1, GL, GL + 1):
                if S >= 1 and rows * S * n <= 1 << 40:
                    assert hs.plan(n, rows, S, dtype) == wc.expected_plan(n, rows, S, dtype), (n, rows, S, dtype)


def test_a_changed_rule_is_noticed(monkeypatch):
    """the pin has teeth: another workgroup target or batch size moves the expected workspace of cases of the sweep"""
    lib = {c: hs.plan(*c) for c in all_plan_cases()}
    monkeypatch.setattr(wc, "TARGET_WGS", 1024)
    assert any(wc.expected_plan(*c) != p for c, p in lib.items())
    monkeypatch.undo()
    monkeypatch.setattr(wc, "LARGE_WS", 128 << 20)
    assert any(wc.expected_plan(*c) != p for c, p in lib.items())


# ---- what each case hits ---------------------------------------------------------------------------------------------
def test_exact_shapes_cross_the_chunk_seams_they_claim():
    for (rows, S), claim in wc.EXACT_SHAPES.items():
        assert wc.chunk_seams(rows, S) == claim, (rows, S, wc.chunking(rows, S))
    union = set().union(*wc.EXACT_SHAPES.values())
    assert union == {"G>1", "part-chunk", "chunks>1", "fewer-chunks"}
    # the chunk layouts the list is meant to hold
    assert wc.chunking(1024, 5)[1:] == (3, 2) and wc.chunking(512, 10)[1:] == (3, 4) and 10 - 3 * 3 == 1
    assert wc.chunking(512, 9) == (4, 3, 3) and wc.chunking(3, 1001) == (683, 2, 501)
    assert wc.chunking(2048, 6)[2] == 1 and wc.chunking(2049, 6)[2] == 1 and wc.chunking(1, 2049)[1:] == (2, 1025)
    # every exact case is fused both ways in every dtype: the chunk rule is what it runs
    for rows, S, n, step in EXACT:
        for d in wc.EXACT_DTYPES:
            assert wc.fused(n, d) == (True, True)


def test_exact_cases_cover_every_step_seam_and_every_coverage_count():
    seen = {n: set() for n in wc.EXACT_N}
    for case in EXACT:
        rows, S, n, step = case
        seam = wc.step_seam(n, step)
        assert seam, case
        seen[n] |= seam
        T = wc.exact_length(case)
        assert (T - n) // step + 1 == S
        cov = wc.coverage(T, n, step)
        if step == 1:
            assert set(cov.tolist()) == set(range(1, min(n, S) + 1)), case      # samples under 1, 2, ..., n segments
        if step > n:
            assert int((cov == 0).sum()) == (S - 1) * (step - n) + step - 1, case   # gaps between segments, and the tail
        if step > 1:
            assert bool((cov[-(step - 1):] == 0).all()), case                     # a tail that no segment covers
    assert seen[1] == {"step=1", "step=n", "step=n+3"}                             # n = 1: step n - 1 would be 0
    assert seen[2] == seen[4] == {"step=1", "step=n-1", "step=n", "step=n+3"}
    assert any(wc.is_strict(c) for c in EXACT) and not all(wc.is_strict(c) for c in EXACT)
    assert {wc.exact_scaling(c)[0] for c in EXACT if wc.is_strict(c)} == {"density", "spectrum"}


def test_toleranced_cases_cross_the_seams_they_claim():
    for name, n, rows, S, fwd, bwd in wc.FUSED_CASES:
        for d in fwd:
            assert wc.fused(n, d)[0], (name, d)
        for d in bwd:
            assert wc.fused(n, d)[1], (name, d)
        assert wc.chunk_seams(rows, S) == {"G>1", "part-chunk", "chunks>1"}
    assert not wc.fused(16384, wc.F64)[0] and not wc.fused(16384, wc.F32)[1]      # why direct-16384 is float32 forward
    limits = {"four-step-32768": 512, "four-step-16384-S600": 1024, "four-step-16384-S300": 512,
              "bluestein-four-step-8193": 512}
    for name, n, rows, S, fwd, bwd in wc.WORKSPACE_CASES:
        for d in fwd:
            assert not wc.fused(n, d)[0], (name, d)
        for d in bwd:
            assert not wc.fused(n, d)[1], (name, d)
        for d in set(fwd) | set(bwd):
            assert wc.batch_limit(n, d) == limits[name]
            assert wc.batch_seams(n, rows, S, d) == {"batches>1", "batch-ends-inside-a-row"}, (name, d)
            assert rows > 1 and S > 1                       # row and segment indices beyond 0 in vec_scale and seg_store
    paths = {hs.plan(c[1], c[2], c[3], d)[0] for c in wc.WORKSPACE_CASES for d in c[4]}
    assert paths == {"four-step", "bluestein+four-step"}
    assert {hs.plan(c[1], c[2], c[3], d)[0] for c in wc.FUSED_CASES for d in c[4]} == {"direct", "bluestein"}
    for c in wc.WORKSPACE_CASES:                            # the unfolded complex128 block of a case stays small
        assert c[2] * c[3] * c[1] * 16 <= 350e6


# ---- the integer cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=wc.exact_id)
def test_exact_references_are_integers_below_2_20(case):
    rows, S, n, step = case
    x, g, w, pxx, grad, k = wc.exact_reference(case)
    assert float(x.real.abs().max()) <= 4 and float(x.imag.abs().max()) <= 4 and float(g.abs().max()) <= 4
    assert bool((w == 1).all()) and k == S * (n * n if wc.exact_scaling(case)[0] == "spectrum" else 2.0 * n)
    # the float64 formula lands on the integers an int64 DFT gives
    acc = wc.integer_dft_accumulator(x, n, step)
    assert float((pxx - acc).abs().max()) < 1e-6 and torch.equal(pxx.round().long(), acc)
    gi = torch.view_as_real(grad)
    assert float((gi - gi.round()).abs().max()) < 1e-6
    # three roundings of at most 2^-24 each cannot move an accumulator below 2^20 by 0.5
    assert int(acc.max()) < 1 << 20 and float(gi.abs().max()) < 1 << 20
    cov = wc.coverage(wc.exact_length(case), n, step)
    assert bool((gi[:, cov == 0] == 0).all())


def test_blocked_references_equal_the_formula():
    x = torch.complex(wc.gaussian((5, 300), 1), wc.gaussian((5, 300), 2))
    w = torch.hamming_window(32, periodic=False, dtype=wc.F64)
    g = wc.gaussian((5, 32), 3)
    for step in (1, 7, 32, 40):
        a, b = wc.ref_pxx(x, w, step, 2.0, "density"), wc.ref_pxx_blocked(x, w, step, 2.0, "density", rows_block=2)
        assert torch.equal(a, b)
        ga = wc.ref_grad(x, w, g, step, 2.0, "density")
        gb = wc.ref_grad_blocked(x, w, g, step, 2.0, "density", rows_block=2, seg_block=3)
        assert wc.per_row(gb, ga) < 1e-14


# ---- the layouts -----------------------------------------------------------------------------------------------------
def test_layouts_hold_the_same_rows_and_copy_only_where_documented():
    x = torch.complex(wc.gaussian((wc.LAYOUT_ROWS, wc.LAYOUT_T), 4), wc.gaussian((wc.LAYOUT_ROWS, wc.LAYOUT_T), 5))
    strides = set()
    for name, copies in wc.LAYOUTS.items():
        pr, pi, dim, unbatch = wc.layout(name, x)
        assert pr.shape == pi.shape and pr.shape[dim] == wc.LAYOUT_T
        back = torch.complex(pr, pi).movedim(dim, -1).reshape(wc.LAYOUT_ROWS, wc.LAYOUT_T)
        assert torch.equal(back, x), name
        qr, qi, _, rs, es = hs._layout(pr, pi, dim)
        assert (qr.data_ptr() != pr.data_ptr()) == copies, name
        strides.add((rs, es))
    T = wc.LAYOUT_T                                         # (row stride, element stride): four no-copy layouts differ
    assert {(2 * T, 2), (T, 1), (3 * T, 3), (2, 12)} <= strides, strides


# ---- the headroom of the bounds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [r for r in wc.tol_runs(4) if r[1] == wc.F32], ids=wc.tol_id)
def test_complex64_formula_stays_within_a_quarter_of_the_pxx_bound(run):
    (name, n, rows, S, _, _), dtype = run
    x, w, _ = wc.tol_input(name, False)
    got = wc.ref_pxx_blocked(x.to(torch.complex64), w.float(), 1, wc.TOL_FS, wc.TOL_SCALING)
    assert got.dtype == wc.F32 and got.shape == (rows, n)
    e = wc.per_row(got, wc.tol_pxx(name, False))
    print(f"welch_headroom pxx {name}: {e:.3g} of {wc.PXX_TOL[dtype]:.0e}")
    assert e <= wc.HEADROOM * wc.PXX_TOL[dtype]


@pytest.mark.parametrize("run", [r for r in wc.tol_runs(5) if r[1] == wc.F32], ids=wc.tol_id)
def test_complex64_formula_stays_within_a_quarter_of_the_gradient_bound(run):
    (name, n, rows, S, _, _), dtype = run
    x, w, g = wc.tol_input(name, False)
    got = wc.ref_grad_blocked(x.to(torch.complex64), w.float(), g.float(), 1, wc.TOL_FS, wc.TOL_SCALING)
    assert got.dtype == torch.complex64 and got.shape == x.shape
    e = wc.per_row(got, wc.tol_grad(name, False))
    print(f"welch_headroom grad {name}: {e:.3g} of {wc.GRAD_TOL[dtype]:.0e}")
    assert e <= wc.HEADROOM * wc.GRAD_TOL[dtype]


# ---- weak bands ------------------------------------------------------------------------------------------------------
def test_band_edges_select_the_same_bins_in_both_precisions():
    from cplxmodule_amd.utils import spectrum as sp
    for n in wc.BAND_NPERSEG:
        spacing = wc.BAND_FS / n
        for r in range(2):
            bands = wc.band_edges(r)
            a, b = wc.band_select(n, bands, wc.F32), wc.band_select(n, bands, wc.F64)
            for (lo, hi), ia, ib in zip(bands, a, b):
                assert torch.equal(ia, ib) and len(ia) >= 19
                for edge in (lo, hi):                       # no edge within a hundredth of a bin of a frequency
                    assert abs(edge / spacing - round(edge / spacing)) > 0.01
            for dtype in wc.BAND_DTYPES:                    # and the library's host bins are the same ranges
                assert [list(range(p, q)) for p, q in sp._band_bins(n, wc.BAND_FS, bands, dtype)] == [i.tolist() for i in a]
        assert (wc.BAND_ROWS[0][0] / spacing).is_integer()  # the tone is on a bin


@pytest.mark.parametrize("fn, nperseg", wc.BAND_RUNS)
def test_band_levels_and_complex64_headroom(fn, nperseg):
    x = wc.band_signal()
    assert torch.equal(x.real, x.real.float().double())
    ov, scaling = wc.band_run_params(fn, nperseg)
    ref = wc.band_ref_pxx(x, nperseg, ov, scaling)
    pb, ptot = wc.band_powers(ref, nperseg), ref.sum(-1, keepdim=True)
    db = 10 * torch.log10(pb[:, 1:] / pb[:, :1])
    print(f"welch_bands {fn} n={nperseg}: levels {[round(v, 2) for v in db.flatten().tolist()]} dB")
    assert float((db - torch.tensor(wc.BAND_LEVELS_DB, dtype=wc.F64)).abs().max()) <= wc.BAND_LEVEL_SLACK_DB
    assert float((pb[:, :1] / ptot).min()) > 0.98            # the main channel holds the tone
    got = wc.band_powers(wc.band_ref_pxx(x, nperseg, ov, scaling, torch.complex64), nperseg)
    ratio = (got - pb).abs() / wc.band_bound(pb, ptot, wc.BAND_EPS[wc.F32])
    print(f"welch_bands {fn} n={nperseg} complex64: error / bound per band {[f'{v:.3g}' for v in ratio.flatten().tolist()]}")
    assert float(ratio.max()) <= wc.HEADROOM
