"""CPU tests of x2_range_cases.py: the numpy emulation of csrc/split.hip against what the design documents, the error model
against the emulated split products on every case the GPU tests run (sections D and E), the cases' own preconditions, and a
demonstration on the CPU of why the LRT layers' variance products cannot run on one scale per tensor (section F's recipe)."""
import numpy as np
import pytest

import conv_exact_cases as CE
import x2_range_cases as X
from oracle import cplx_oracle as orc

KINDS = ("x2", "x3")


# ---- the emulation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", X.C_SHAPES)
def test_scale_seams_emulated(rows, cols):
    for name, (a, b, op) in X.scale_seam_inputs(rows, cols).items():
        s, inv = X.emulate_absmax_scale(a, b, op)
        assert s == np.float32(2.0 ** X.SCALE_EXPECT[name]) and s * inv == 1.0, (name, s, inv)
    for n in X.PARTIAL_COUNTS:
        p, m = X.partial_inputs(n)
        assert (p[:n].max() if n else 0.0) == m and (n == 2048 or not p[n:].max() <= m)
    assert X.scale_from_max(9.5)[0] == 2.0 ** 11 and X.scale_from_max(0.0)[0] == 1.0


def test_emulation_agrees_with_the_convolution_tests_emulation():
    a = (np.random.RandomState(0).randn(40, 64) * 3.0).astype(np.float32)
    s, p0, p1 = CE.emulate_x2_split(a)
    sc = X.emulate_absmax_scale(a)
    h0, h1 = X.emulate_split2h(a, sc[0])
    assert s == float(sc[0]) and np.array_equal(p0, h0.astype(np.float64)) and np.array_equal(p1, h1.astype(np.float64))


@pytest.mark.parametrize("rows,cols", X.C_SHAPES)
def test_split2h_emulated_on_the_seam_input(rows, cols):
    """The documented piece errors hold on the emulation, element by element: |x s - h0 - h1| <= max(2^-22 |x s|, 2^-25);
    ties go to even; a stale scale 16 times too large makes the first piece inf and the second 0."""
    x = X.split_seam_input(rows, cols)
    s, _ = X.emulate_absmax_scale(x)
    assert s == 2.0 ** X.SPLIT_S
    h0, h1 = X.emulate_split2h(x, s)
    v = x.astype(np.float64) * float(s)
    rem = np.abs(v - h0.astype(np.float64) - h1.astype(np.float64))
    assert (rem <= np.maximum(np.abs(v) * 2.0 ** -22, 2.0 ** -25)).all()
    assert np.array_equal(rem / float(s) <= X.piece_error("x2", x, s), np.ones_like(rem, dtype=bool))
    if x.size >= 16:
        f0 = h0.reshape(-1).astype(np.float64)
        # 2^10 (1 + (2 j + 1) 2^-11) lies halfway between two halves: to the even one
        assert list(f0[1:4]) == [1024.0, 1026.0, 1026.0] and f0[4] == -(2.0 ** 14) * (1 + 4 * 2.0 ** -11)
        assert f0[5] == 0.0 and f0[6] == -(2.0 ** -23) and f0[7] == 0.0 and np.signbit(h0.reshape(-1)[8])
        assert (h0 == 0).sum() > 2 and ((np.abs(f0) < 2.0 ** -14) & (f0 != 0)).any()      # flushes and subnormals occur
    g0, g1 = X.emulate_split2h(x, s * np.float32(16.0))
    big = np.abs(v) * 16.0 > 65504.0
    assert big.any() and np.isinf(g0[big].astype(np.float64)).all() == bool((np.abs(v[big]) * 16 >= 65520).all())
    assert (g1[big] == 0).all()


def test_split3_emulated_is_exact():
    rs = np.random.RandomState(1)
    x = (rs.randn(64, 40) * np.exp(rs.uniform(-30, 30, (64, 40)))).astype(np.float32)
    x0, x1, x2 = X.emulate_split3(x)
    assert np.array_equal((x2 + x1) + x0, x)
    for p in (x0, x1, x2):
        assert not (p.view(np.uint32) & 0xffff).any()
    t = np.array([np.inf, -np.inf, np.nan, 3.4e38], dtype=np.float32)
    y0, y1, y2 = X.emulate_split3(t)
    assert np.isinf(y0[:2]).all() and np.isnan(y0[2]) and np.isinf(y0[3]) and not y1.any() and not y2.any()
    a = X.op_value(X.OP_ABS2, np.float32([3.0, 1e-30]), np.float32([4.0, 1e-30]))
    assert a[0] == 25.0 and a[1] == 0.0


# ---- the error model on the cases of sections D and E ------------------------------------------------------------------------
def _emulated(kind, pa, pb, conj_b=False):
    """The emulated product per plane, and the planes' scales (one per operand)."""
    sa = sb = None
    if kind == "x2":
        sa = X.emulate_absmax_scale(*pa, op=X.OP_MAX2) if len(pa) == 2 else X.emulate_absmax_scale(pa[0])
        sb = X.emulate_absmax_scale(*pb, op=X.OP_MAX2) if len(pb) == 2 else X.emulate_absmax_scale(pb[0])
    if len(pa) == 1:
        return (X.emulated_product(kind, pa[0], pb[0], sa, sb),), sa, sb
    pairs = X.cplx_as_real(pa[0], pa[1], pb[0], pb[1], conj_b)
    return tuple(X.emulated_product(kind, a.astype(np.float32), b.astype(np.float32), sa, sb) for a, b in pairs), sa, sb


def _bounds(kind, pa, pb, **kw):
    if len(pa) == 1:
        return (X.bound(kind, pa[0], pb[0], **kw),)
    return X.cplx_bound(kind, pa[0], pa[1], pb[0], pb[1], **kw)


@pytest.mark.parametrize("cplx", (False, True))
@pytest.mark.parametrize("M,N,K", X.SHAPES)
def test_invariance_cases_and_their_bound(M, N, K, cplx):
    """Section D on the CPU: the shifts are exact, both scale exponents stay inside the clip and move with the shift (the
    pieces are the same bits), every result a GPU test compares stays a normal float32, and the emulated products lie inside
    the bound -- including the pair beyond the clip."""
    d = X.invariance_operands(M, N, K, cplx)
    base = {k: _emulated(k, d["a"], d["b"]) for k in KINDS}
    ref0 = X.reference(d["a"], d["b"])
    for p, q in X.PAIRS + (X.BEYOND_CLIP,):
        a, b = X.shifted(d["a"], p), X.shifted(d["b"], q)
        clipped = (p, q) == X.BEYOND_CLIP
        if not clipped:
            for u, v, e in zip(d["a"] + d["b"], a + b, (p,) * len(a) + (q,) * len(b)):
                assert np.array_equal(v.astype(np.float64), u.astype(np.float64) * 2.0 ** e)
            # what the three drivers return: the raw product, + bias, + beta * C_old -- all normal after the shift
            outs = [v for r, bi, c0 in zip(ref0, d["bias"], d["c0"]) for v in (r, r + bi, r + X.BETA * c0.astype(np.float64))]
            assert 2.0 ** -125 < min(float(np.abs(v).min()) for v in outs) * 2.0 ** (p + q)
            assert max(float(np.abs(v).max()) for v in outs) * 2.0 ** (p + q) < 2.0 ** 126
        ref = X.reference(a, b)
        for kind in KINDS:
            if clipped and kind == "x3":
                continue                                   # (no scale, nothing to clip; float32 subnormal operands)
            got, sa, sb = _emulated(kind, a, b)
            if kind == "x2":
                ka, kb = int(np.log2(float(sa[0]))), int(np.log2(float(sb[0])))
                assert (ka == X.CLIP) == clipped and abs(kb) < X.CLIP
                if not clipped:
                    assert float(sa[0]) == float(base[kind][1][0]) * 2.0 ** -p and float(sb[0]) == float(base[kind][2][0]) * 2.0 ** -q
                    if (p, q) in ((-52, -52), (-60, -45)):
                        assert ka + kb >= 128                # sa sb is inf in float32: what the scale undo must survive
            if not clipped:                                  # the emulation itself is invariant, bit for bit
                for g, g0 in zip(got, base[kind][0]):
                    assert np.array_equal(g, np.ldexp(g0, p + q))
            for g, r, bd in zip(got, ref, _bounds(kind, a, b)):
                assert np.isfinite(g).all() and (np.abs(g.astype(np.float64) - r) <= bd).all(), (kind, p, q)


@pytest.mark.parametrize("cplx", (False, True))
@pytest.mark.parametrize("side", ("a", "b"))
def test_row_range_cases_and_their_bound(cplx, side):
    """Section E on the CPU: inside the bound for both arithmetics; 'x2' returns exact zeros from 2^-41 on and 'x3' is
    invariant under the row scaling, bit for bit."""
    a0, b0, r = X.row_range_operands(cplx, side)
    a, b = (X.scale_rows(a0, r), b0) if side == "a" else (a0, X.scale_rows(b0, r))
    ref = X.reference(a, b)
    for kind in KINDS:
        got, _, _ = _emulated(kind, a, b)
        base, _, _ = _emulated(kind, a0, b0)
        for g, g0, rf, bd in zip(got, base, ref, _bounds(kind, a, b)):
            assert (np.abs(g.astype(np.float64) - rf) <= bd).all(), kind
            rows = g if side == "a" else g.T
            if kind == "x2":
                assert not rows[r >= X.ZERO_FROM].any() and rows[r < X.ZERO_FROM].all()
            else:
                assert np.array_equal(rows, np.ldexp(g0 if side == "a" else g0.T, -r[:, None]))


# ---- why 'auto' runs the variance products on bf16 pieces ---------------------------------------------------------------------
@pytest.mark.parametrize("cplx", (True, False))
def test_one_scale_per_tensor_breaks_small_samples_variance(cplx):
    """Section F's recipe (sample blocks scaled by 2^(8 - 2 j), j = 0 .. 7: |x|^2 spans 2^28 -- the span the issue states, not
    narrowed) on the emulation.  The 'x2' variance product s2 = |x|^2 exp(log_sigma2)^T misses the per-row 1e-5 check on
    the small samples' rows; the 'x3' variance product together with the 'x2' mean product passes it on every row of s2
    and of y with a factor 2 to spare."""
    d = X.layer_inputs(cplx)
    f = lambda t: t.astype(np.float64)  # noqa: E731
    a32 = X.op_value(X.OP_ABS2, d["x"][0], d["x"][1] if cplx else None)
    S32 = X.op_value(X.OP_EXP, d["ls2"])
    if cplx:
        yr, yi, aux = orc.lrt_cplx_linear(f(d["x"][0]), f(d["x"][1]), f(d["w"][0]), f(d["w"][1]), f(d["b"][0]), f(d["b"][1]),
                                          f(d["ls2"]), f(d["eps"][0]), f(d["eps"][1]))
        y_ref = (yr, yi)
    else:
        y, aux = orc.lrt_real_linear(f(d["x"][0]), f(d["w"][0]), f(d["b"][0]), f(d["ls2"]), f(d["eps"][0]))
        y_ref = (y,)
    assert aux["s2"].min() > 50 * X.CLAMP                # every s2 far above the clamp of reparam.hip
    s2 = {k: X.emulated_product(k, a32, S32).astype(np.float64) for k in KINDS}
    worst2, bad = X.row_check(s2["x2"], aux["s2"])
    assert len(bad) >= 16 and bad.min() >= 5 * 16 and worst2 > 10.0, (worst2, bad)     # samples 2^-20 and more below the largest
    worst3, bad3 = X.row_check(s2["x3"], aux["s2"])
    assert worst3 <= 0.5 and not len(bad3), worst3
    mu, _, _ = _emulated("x2", d["x"], d["w"])
    for p, (m, yref) in enumerate(zip(mu, y_ref)):
        y = (m.astype(np.float64) + f(d["b"][p])) + f(d["eps"][p]) * np.sqrt(np.maximum(s2["x3"], X.CLAMP))
        worst, _ = X.row_check(y, yref)
        assert worst <= 0.5, (p, worst)
        y2 = (m.astype(np.float64) + f(d["b"][p])) + f(d["eps"][p]) * np.sqrt(np.maximum(s2["x2"], X.CLAMP))
        assert X.row_check(y2, yref)[0] > 1.0            # ... and with the 'x2' variance the layer's output misses it too
