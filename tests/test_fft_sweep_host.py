"""The FFT engine sweep without a GPU: the case lists of fft_sweep_cases.py reach every transform length the engine is
compiled for (computed from the library's plan over the lists, so a length dropped from a list fails here), every strided
view of the sweep takes the no-copy branch with the number of batch runs it is meant to have, and the batch limit of the
workspace loop that the GPU test straddles is the library's."""
import pytest
import torch

import fft_cases as fc
import fft_sweep_cases as sc
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd import rfft as hostrfft

FOUR_STEP_HALVES = {(8, 7), (8, 8), (9, 8), (9, 9), (10, 9), (10, 10), (11, 10), (11, 11)}


def coverage(plans):
    """plans: (path, points run, dtype, complex length) of every case of a list -> the sets of compiled sizes they reach;
    a Bluestein size counts only when BOTH ends of the range of lengths that selects it are in the list"""
    direct, fused, workspace, halves = {sc.F32: set(), sc.F64: set()}, set(), set(), set()
    lengths = {}
    for path, points, dtype, cn in plans:
        if path.startswith("bluestein"):
            lengths.setdefault((path, points), set()).add(cn)
    for path, points, dtype, cn in plans:
        lg = sc.log2(points)
        if path.startswith("bluestein"):
            lo, hi = min(lengths[path, points]), max(lengths[path, points])
            if fc.transform_size(lo - 2) == points or fc.transform_size(hi + 2) == points:      # (the lengths are odd)
                continue
        if path == "direct":
            direct[dtype].add(lg)
        elif path == "bluestein":
            fused.add(lg)
        elif path == "bluestein+four-step":
            workspace.add(lg)
        else:
            assert path == "four-step", path
            halves.add(sc.halves(points, dtype))
    return direct, fused, workspace, halves


def assert_complete(direct, fused, workspace, halves):
    assert direct[sc.F32] == set(range(0, 15)), sorted(set(range(0, 15)) - direct[sc.F32])
    assert direct[sc.F64] == set(range(0, 14)), sorted(set(range(0, 14)) - direct[sc.F64])
    assert fused == set(range(3, 14)), sorted(set(range(3, 14)) - fused)
    assert len(workspace) >= 2, workspace
    assert FOUR_STEP_HALVES <= halves, sorted(FOUR_STEP_HALVES - halves)


def fft_plans(lengths):
    return [(hostfft.plan(n, sc.vectors(n), dtype)[0], fc.transform_size(n), dtype, n) for n in lengths for dtype in sc.WIDE]


def rfft_plans(lengths):
    out = []
    for n in lengths:
        for dtype in sc.WIDE:
            path, cn, points = hostrfft.plan(n, sc.vectors(n), dtype)[:3]
            out.append((path, points, dtype, cn))
    return out


def test_the_fft_list_reaches_every_compiled_size():
    assert_complete(*coverage(fft_plans(sc.FFT_LENGTHS)))


def test_the_rfft_list_reaches_every_compiled_size_on_both_routes():
    """the half-length route alone (even n) reaches every size but the four-step halves (11, 11) -- n = 2^23 is beyond
    the longest transform --; the odd lengths reach every Bluestein size again on the full-length route"""
    even = [n for n in sc.RFFT_LENGTHS if n % 2 == 0]
    odd = [n for n in sc.RFFT_LENGTHS if n % 2 == 1]
    direct, fused, workspace, halves = coverage(rfft_plans(even))
    assert_complete(direct, fused, workspace, halves | {(11, 11)})
    assert (11, 11) not in halves
    _, fused, workspace, _ = coverage(rfft_plans(odd))
    assert fused == set(range(3, 14)) and len(workspace) >= 2


@pytest.mark.parametrize("drop", [16, 4096, 1 << 17, 1 << 22, 3, 17, 31, 2049, 4095])
def test_a_dropped_length_is_noticed(drop):
    assert drop in sc.FFT_LENGTHS
    with pytest.raises(AssertionError):
        assert_complete(*coverage(fft_plans([n for n in sc.FFT_LENGTHS if n != drop])))


def test_both_ends_of_every_bluestein_range_select_its_size():
    for m in range(3, 16):
        ends = sc.bluestein_ends(m)
        assert len(ends) == (1 if m == 3 else 2)
        for n in ends:
            assert fc.transform_size(n) == 1 << m
        assert fc.transform_size(ends[0] - 1) < 1 << m and fc.transform_size(ends[-1] + 2) > 1 << m   # (n odd: n + 1 is 2^k)


def test_the_library_plans_what_the_lists_expect():
    for n in sc.FFT_LENGTHS:
        for dtype in sc.WIDE:
            assert hostfft.plan(n, sc.vectors(n), dtype)[:2] == sc.expected_fft_plan(n, dtype), (n, dtype)
    for n in sc.RFFT_LENGTHS:
        for dtype in sc.WIDE:
            for c2r in (False, True):
                assert hostrfft.plan(n, sc.vectors(n), dtype, c2r)[:4] == sc.expected_rfft_plan(n, dtype), (n, dtype)


@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_routes_are_the_smallest_lengths_off_the_packed_kernel(case):
    kind, route, n, dtype = case
    path, points = sc.ROUTE_PLAN[route]
    if kind == "c2c":
        got_path, vpw = hostfft.plan(n, sc.B, dtype)[:2]
        got_points = fc.transform_size(n)
    else:
        got_path, cn, got_points, vpw = hostrfft.plan(n, sc.B, dtype, kind == "c2r")[:4]
        assert cn == (n if route.endswith("odd") else n // 2)
    assert (got_path, vpw) == (path, 1)
    assert points in (None, got_points)
    if path == "four-step":
        assert sc.halves(got_points, dtype) is not None
        smaller = hostfft.plan(n // 2, sc.B, dtype)[0] if kind == "c2c" else hostrfft.plan(n // 2, sc.B, dtype)[0]
        assert smaller == "direct"


# ---- the views of the layout sweep take the no-copy branch -------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ROUTES, ids=sc.route_id)
def test_every_view_is_transformed_where_it_lies(case):
    kind, _, n, dtype = case
    xs = sc.baseline_input(kind, n, dtype)
    assert len(sc.runs_of(kind, xs[0], n, -1)) == 1                      # the baseline: one run
    for name, (runs, copies) in sc.LAYOUTS.items():
        views, dim = [], None
        for x in xs:
            v, dim, unbatch = sc.layout(name, x)
            views.append(v)
        assert sc.takes_no_copy(kind, views, n, dim), name
        assert len(sc.runs_of(kind, views[0], n, dim)) == runs, (name, sc.runs_of(kind, views[0], n, dim))
        # the view holds the baseline's vectors, `copies` times over
        back = unbatch(views[0])
        assert back.shape == (copies, sc.B, sc.in_len(kind, n)) and torch.equal(back, xs[0].expand_as(back)), name
    assert any(views[0].stride(d) == 0 for d in range(views[0].dim()))   # the last one is the expanded batch


# ---- the batch limit of the workspace loop -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.SEAMS, ids=sc.seam_id)
def test_the_seam_batches_straddle_the_librarys_batch_limit(case):
    kind, n, dtype, GL = case
    ws = lambda batch: sc.workspace_bytes(kind, n, batch, dtype)  # noqa: E731
    assert ws(GL) == ws(GL + 1) == ws(2 * GL + 3)         # the buffers stop growing at GL vectors
    assert ws(GL - 1) < ws(GL)
    for batch in sc.seam_batches(GL):
        d = sc.CYCLE[batch]
        assert batch % d == 0 and GL % d != 0 and d >= 5
    path = (hostfft.plan(n, GL, dtype) if kind == "c2c" else hostrfft.plan(n, GL, dtype))[0]
    assert path in ("four-step", "bluestein+four-step")


def test_the_grid_batches_cross_65536_workgroups():
    for kind, n, dtype in sc.GRID_CASES:
        if kind == "c2c":
            path, vpw = hostfft.plan(n, 65537, dtype)[:2]
        else:
            path, _, _, vpw = hostrfft.plan(n, 65537, dtype, kind == "c2r")[:4]
        assert (path, vpw) == ("direct", 1)
    assert [b for b, _ in sc.GRID_BATCHES] == [1, 2, 65537, 65541]
    assert all(b % d == 0 for b, d in sc.GRID_BATCHES)
