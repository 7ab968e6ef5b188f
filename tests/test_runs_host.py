"""The batch-run layer of the signal features (cplxmodule_amd/_runs.py) on the CPU: no library, no GPU.

The run lists of RUNS are literals recorded from the two functions this module replaced (`fft._runs` for one skipped dim and
two tensors, `fftconv._runs` for the last dim and any number of tensors) at the commit before it; where both applied
they agreed.
"""
import pytest
import torch

from cplxmodule_amd import _lib, _runs
from cplxmodule_amd._lib import CplxAmdError

# (name, shape, strides per tensor (the result's last), skipped dim, runs [size, stride per tensor ...] outermost first)
RUNS = [
    ("contiguous", (4, 5, 6, 8), ((240, 48, 8, 1), (240, 48, 8, 1)), -1,
     [[120, 8, 8]]),
    ("channels_last_to_itself", (4, 5, 6, 8), ((240, 1, 40, 5), (240, 1, 40, 5)), -1,
     [[24, 40, 40], [5, 1, 1]]),
    ("channels_last_to_dense", (4, 5, 6, 8), ((240, 1, 40, 5), (240, 48, 8, 1)), -1,
     [[4, 240, 240], [5, 1, 48], [6, 40, 8]]),
    ("transposed_pair", (4, 5, 6, 8), ((48, 192, 8, 1), (240, 48, 8, 1)), -1,
     [[4, 48, 240], [5, 192, 48], [6, 8, 8]]),
    ("step_slice", (4, 5, 6, 8), ((960, 96, 16, 1), (240, 48, 8, 1)), -1,
     [[4, 960, 240], [30, 16, 8]]),
    ("expanded_filter", (4, 5, 6, 8), ((240, 48, 8, 1), (0, 3, 0, 1), (240, 48, 8, 1)), -1,
     [[4, 240, 0, 240], [5, 48, 3, 48], [6, 8, 0, 8]]),
    ("size_1_between_fusable", (4, 1, 6, 8), ((48, 48, 8, 1), (48, 48, 8, 1)), -1,
     [[24, 8, 8]]),
    ("size_1_with_a_stray_stride", (4, 1, 6, 8), ((48, 7, 8, 1), (48, 48, 8, 1)), -1,
     [[24, 8, 8]]),
    ("two_tensors", (4, 5, 6, 8), ((48, 192, 8, 1), (48, 192, 8, 1)), -1,
     [[120, 8, 8]]),
    ("three_tensors", (4, 5, 6, 8), ((960, 96, 16, 1), (18, 0, 3, 1), (240, 48, 8, 1)), -1,
     [[4, 960, 18, 240], [5, 96, 0, 48], [6, 16, 3, 8]]),
    ("four_tensors", (4, 5, 6, 8), ((240, 48, 8, 1), (0, 12, 0, 1), (0, 4, 0, 1), (660, 132, 22, 1)), -1,      # filtfilt's x, c, u, y
     [[4, 240, 0, 0, 660], [5, 48, 12, 4, 132], [6, 8, 0, 0, 22]]),
    ("four_tensors_strided_x", (4, 5, 6, 8), ((960, 96, 16, 1), (0, 12, 0, 1), (0, 4, 0, 1), (660, 132, 22, 1)), -1,
     [[4, 960, 0, 0, 660], [5, 96, 12, 4, 132], [6, 16, 0, 0, 22]]),
    ("exactly_3_runs", (4, 5, 6, 8), ((240, 48, 8, 1), (18, 0, 3, 1), (240, 48, 8, 1)), -1,
     [[4, 240, 18, 240], [5, 48, 0, 48], [6, 8, 3, 8]]),
    ("4_runs", (2, 3, 4, 5, 8), ((480, 160, 40, 8, 1), (12, 0, 3, 0, 1), (480, 160, 40, 8, 1)), -1,
     [[2, 480, 12, 480], [3, 160, 0, 160], [4, 40, 3, 40], [5, 8, 0, 8]]),
    ("skip_last", (4, 5, 6, 8), ((240, 1, 40, 5), (240, 1, 40, 5)), 3,
     [[24, 40, 40], [5, 1, 1]]),
    ("skip_middle", (4, 5, 6, 8), ((240, 1, 40, 5), (240, 1, 40, 5)), 1,
     [[192, 5, 5]]),
    ("skip_middle_transposed", (4, 5, 6, 8), ((48, 192, 8, 1), (240, 48, 8, 1)), 2,
     [[4, 48, 240], [5, 192, 48], [8, 1, 1]]),
    ("skip_first", (4, 5, 6, 8), ((960, 96, 16, 1), (240, 48, 8, 1)), 0,
     [[30, 16, 8], [8, 1, 1]]),
]


@pytest.mark.parametrize("name, shape, strides, skip, want", RUNS, ids=[c[0] for c in RUNS])
def test_run_lists_are_the_recorded_ones(name, shape, strides, skip, want):
    assert _runs.runs(shape, strides, skip) == want


def test_the_strides_of_the_table_are_the_layouts_they_name():
    """the literal strides above are what torch gives these views (a few of them, so that the table means what it says)"""
    by_name = {c[0]: c for c in RUNS}
    cl = torch.empty(4, 6, 8, 5).permute(0, 3, 1, 2)
    assert by_name["channels_last_to_dense"][2] == (cl.stride(), tuple(_runs.dense(cl.shape)))
    s = torch.empty(8, 5, 12, 8)[::2, :, ::2]
    assert by_name["step_slice"][2][0] == s.stride()
    h = torch.empty(1, 5, 1, 3)
    assert by_name["expanded_filter"][2][1] == h.expand(4, 5, 6, 3).stride()
    assert by_name["four_tensors"][2][3] == tuple(_runs.dense((4, 5, 6, 22)))


def test_dense_and_dense_like():
    assert _runs.dense((4, 5, 6)) == [30, 6, 1]
    assert _runs.dense((4, 0, 6)) == [6, 6, 1]
    cl = torch.empty(4, 6, 8, 5).permute(0, 3, 1, 2)
    shape, strides = _runs.dense_like(cl, 3, 16)
    assert (shape, strides) == ([4, 5, 6, 16], list(torch.empty(4, 6, 16, 5).permute(0, 3, 1, 2).stride()))


def test_share_copies_only_planes_without_a_common_layout():
    a, b = torch.randn(4, 6), torch.randn(6, 4).t()
    assert _runs.share(a, None) == (a, None)
    pr, pi = _runs.share(a, a[:])
    assert pr is a
    pr, pi = _runs.share(a, b)
    assert pr.stride() == pi.stride() == (6, 1) and torch.equal(pi, b)


# ---- fit -------------------------------------------------------------------------------------------------------------------
def _conv_fit(x, h, length=11):
    shape = tuple(x[0].shape[:-1]) + (length,)
    return _runs.fit(shape, [x, h], _runs.dense(shape), [(0,), (1,)])


def test_fit_returns_the_same_tensors_when_three_runs_do():
    xr, xi = torch.randn(4, 5, 6, 8), torch.randn(4, 5, 6, 8)
    hr = torch.randn(4, 1, 6, 3)
    ((ar, ai), (br, bi)), runs = _conv_fit((xr, xi), (hr, None))
    assert ar is xr and ai is xi and br is hr and bi is None
    assert runs == [[4, 240, 18, 330], [5, 48, 0, 66], [6, 8, 3, 11]]


def test_fit_copies_the_signal_only_when_that_is_enough():
    base = torch.randn(4, 6, 8, 10, 8, requires_grad=True)
    xr = base[::2, ::2, ::2, ::2]                         # [2, 3, 4, 5, 8]: no two dims fuse
    hr = torch.randn(1, 1, 1, 1, 3)
    assert len(_runs.runs((2, 3, 4, 5, 11), (xr.stride(), hr.expand(2, 3, 4, 5, 3).stride(), _runs.dense((2, 3, 4, 5, 11))))) == 4
    ((ar, ai), (br, bi)), runs = _conv_fit((xr, None), (hr, None))
    assert ar is not xr and ar.is_contiguous() and torch.equal(ar, xr) and ai is None
    assert br is hr
    assert runs == [[120, 8, 0, 11]]
    # the copy is differentiable: the gradient reaches the leaf, at the entries the view reads
    w = torch.randn_like(ar)
    (ar * w).sum().backward()
    want = torch.zeros_like(base)
    want[::2, ::2, ::2, ::2] = w
    assert torch.equal(base.grad, want)


def test_fit_expands_a_filter_whose_broadcast_pattern_alone_is_too_much():
    xr, xi = torch.randn(2, 3, 4, 5, 8), torch.randn(2, 3, 4, 5, 8)
    hr = torch.randn(2, 1, 4, 1, 3, requires_grad=True)
    ((ar, ai), (br, bi)), runs = _conv_fit((xr, xi), (hr, None))
    assert ar is xr and ai is xi                          # a dense signal: `contiguous` gives it back
    assert tuple(br.shape) == (2, 3, 4, 5, 3) and br.is_contiguous() and torch.equal(br, hr.expand(2, 3, 4, 5, 3))
    assert runs == [[120, 8, 3, 11]]
    br.sum().backward()
    assert torch.equal(hr.grad, torch.full_like(hr, 15.0))


def test_fit_like_follows_the_operands_memory_order_and_copies_once():
    pr, pi = torch.randn(4, 16, 6), torch.randn(6, 16, 4).permute(2, 1, 0)
    qr, qi, runs, ys = _runs.fit_like(pr, pi, 1, 9)       # planes without a common layout: both dense
    assert qr is pr and qi.stride() == pr.stride() and torch.equal(qi, pi)
    assert runs == [[4, 96, 54], [6, 1, 1]] and ys == [54, 6, 1]
    qr, qi, runs, ys = _runs.fit_like(pi, pi, 1, 16)      # transposed planes are read where they lie, the result alike
    assert qr is pi and qi is pi and ys == [1, 4, 64]
    assert runs == [[6, 64, 64], [4, 1, 1]]               # (the 16 transformed entries lie between: the two do not fuse)
    qr, qi, runs, ys = _runs.fit_like(pr, None, 1, 16)    # a real operand
    assert qr is pr and qi is None and runs == [[4, 96, 96], [6, 1, 1]]
    base = torch.randn(4, 6, 8, 10, 8, requires_grad=True)
    x = base[::2, ::2, ::2, ::2]                          # no two dims fuse: four runs, one differentiable copy
    assert len(_runs.runs(x.shape, (x.stride(), _runs.dense_like(x, 4, 8)[1]), 4)) == 4
    qr, qi, runs, ys = _runs.fit_like(x, x, 4, 8)
    assert qr.is_contiguous() and qi.is_contiguous() and torch.equal(qr, x) and runs == [[120, 8, 8]] and ys == [480, 160, 40, 8, 1]
    (qr + 2 * qi).sum().backward()
    want = torch.zeros_like(base)
    want[::2, ::2, ::2, ::2] = 3
    assert torch.equal(base.grad, want)


def test_fit_keeps_a_trailing_dim_behind_the_skipped_one():
    """iir's coefficients [*Bc, S, W] ride along with x [*B, N]: their batch strides count, their copy is [*B, S, W]"""
    xr = torch.randn(2, 3, 4, 5, 9)
    cr = torch.randn(2, 1, 4, 1, 2, 6)
    ((ar, _), (br, _)), runs = _runs.fit(xr.shape, [(xr, None), (cr, None)], _runs.dense(xr.shape), [(0,), (1,)])
    assert ar is xr and tuple(br.shape) == (2, 3, 4, 5, 2, 6) and br.is_contiguous()
    assert runs == [[120, 9, 12, 9]]


def test_fit_wgrad_copies_both_operands_then_falls_back_to_per_row_results():
    ar, cr = torch.randn(2, 3, 4, 5, 8), torch.randn(2, 3, 4, 5, 11)
    a, c, runs, f = _runs.fit_wgrad((ar, None), (cr, None), 3, (2, 3, 1, 1))
    assert a[0] is ar and c[0] is cr and f == (2, 3, 1, 1)
    assert runs == [[6, 160, 220, 3], [20, 8, 11, 0]]
    base = torch.randn(4, 6, 8, 10, 8)
    a, c, runs, f = _runs.fit_wgrad((base[::2, ::2, ::2, ::2], None), (cr, None), 3, (1, 1, 1, 1))
    assert a[0].is_contiguous() and c[0] is cr and f == (1, 1, 1, 1) and runs == [[120, 8, 11, 0]]
    a, c, runs, f = _runs.fit_wgrad((ar, None), (cr, None), 3, (2, 1, 4, 1))   # the pattern itself needs four runs
    assert a[0] is ar and c[0] is cr and f == (2, 3, 4, 5) and runs == [[120, 8, 11, 3]]


# ---- fill ------------------------------------------------------------------------------------------------------------------
DESCS = [
    (_lib.FftDesc, ("x_stride", "y_stride")),
    (_lib.FftConvDesc, ("a_stride", "b_stride", "y_stride")),
    (_lib.UpfirdnDesc, ("a_stride", "b_stride", "y_stride")),
    (_lib.IirDesc, ("x_stride", "c_stride", "y_stride")),
    (_lib.FiltFiltDesc, ("x_stride", "c_stride", "z_stride", "y_stride")),
]


@pytest.mark.parametrize("cls, fields", DESCS, ids=[d[0].__name__ for d in DESCS])
def test_fill_writes_sizes_strides_and_the_run_count(cls, fields):
    runs = [[4] + [100 * (i + 1) for i in range(len(fields))], [6] + [10 * (i + 1) for i in range(len(fields))]]
    d = cls()
    assert _runs.fill(d, runs, fields) == (24, 1)
    assert d.runs == 2 and list(d.size) == [4, 6, 0]
    for i, f in enumerate(fields):
        assert list(getattr(d, f)) == [100 * (i + 1), 10 * (i + 1), 0]
    d = cls()
    assert _runs.fill(d, [], fields) == (1, 1)
    assert d.runs == 0 and list(d.size) == [0, 0, 0] and all(list(getattr(d, f)) == [0, 0, 0] for f in fields)
    d = cls()
    assert _runs.fill(d, [[5, 7], [3]], fields) == (15, 1)      # what a run leaves out stays zero (the split path's transition)
    assert list(d.size) == [5, 3, 0] and list(getattr(d, fields[0])) == [7, 0, 0] and list(getattr(d, fields[1])) == [0, 0, 0]


@pytest.mark.parametrize("cls, fields", DESCS[1:], ids=[d[0].__name__ for d in DESCS[1:]])
def test_fill_counts_rows_and_distinct_filters_by_the_key_column(cls, fields):
    n = len(fields)
    shared = [[4] + [240] * n, [5] + [48] * n, [6] + [8] * n]                # run 1's filter stride is zero below
    shared[0][2], shared[2][2] = 0, 0
    assert _runs.fill(cls(), shared, fields, fields[1]) == (120, 5)
    assert _runs.fill(cls(), shared, fields, fields[0]) == (120, 120)
    wgrad = [[6] + [160] * n, [20] + [8] * n]                                 # the result is shared by the inner run
    wgrad[1][n] = 0
    assert _runs.fill(cls(), wgrad, fields, "y_stride") == (120, 6)


# ---- code, planes ----------------------------------------------------------------------------------------------------------
def test_code_and_planes_keep_their_messages():
    from cplxmodule_amd.cplx import Cplx
    assert (_runs.code(torch.float32), _runs.code(torch.bfloat16), _runs.code(torch.float64)) == (_lib.F32, _lib.BF16, _lib.F64)
    with pytest.raises(CplxAmdError, match=r"^fft: planes must be float32, bfloat16 or float64, got torch.float16$"):
        _runs.code(torch.float16)
    x = torch.randn(3)
    assert _runs.planes(x, "x", "upfirdn") == (x, None)
    z = Cplx(x, x + 1)
    assert _runs.planes(z, "x", "upfirdn") == (z.real, z.imag)
    with pytest.raises(CplxAmdError, match="^lfilter: the planes of `b` have different dtypes: torch.float32 and torch.float64$"):
        _runs.planes(Cplx(x, x.double()), "b", "lfilter")
    with pytest.raises(CplxAmdError, match="^fftconvolve: `other` is a Tensor of complex dtype, not a Cplx or a real"):
        _runs.planes(torch.zeros(3, dtype=torch.complex64), "other", "fftconvolve")
    with pytest.raises(CplxAmdError, match="^sosfilt: `sos` is a list, not a Cplx or a real torch.Tensor"):
        _runs.planes([1.0], "sos", "sosfilt")
