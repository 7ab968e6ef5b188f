"""The float32 split products over operand range (cplxmodule_amd/x3.py, csrc/split.hip; cases, emulation and error model:
x2_range_cases.py).

    C  the scale and the half split at their seams, bit for bit against the numpy emulation;
    D  power-of-two invariance of the three launch sequences and of the 'x2' convolution: operands times 2^p, 2^q must give
       the same bits times 2^(p + q) -- no reference needed -- down to operands whose scales' product leaves float32;
    E  rows of one operand scaled block by block: element-wise inside the derived bound, and what each arithmetic
       promises row by row;
    F  the LRT layers sample by sample and output unit by output unit against the float64 oracle at the 1e-5 parity bar.
"""
import numpy as np
import pytest
import torch

import gemm_exact_cases as G
import x2_range_cases as X
from gpu_util import N, T
from oracle import cplx_oracle as orc

pytestmark = pytest.mark.gpu

FLAGS = {"eight-wave": G.K1, "one-wave-per-SIMD": G.K3}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_halves(got, want_np):
    """fp16 tensor == numpy float16 array, bit for bit (so that -0 and the NaN pattern count)."""
    return torch.equal(_bits(got), _bits(T(want_np)))


# ---- C: the scale -------------------------------------------------------------------------------------------------------
def _strided(a, pad):
    """`a` as a column block of a wider matrix whose other columns hold `pad` values: they must never be read."""
    rows, cols = a.shape
    wide = np.empty((rows, cols + 16), dtype=np.float32)
    wide[:] = pad
    wide[1::2, :8] = np.nan
    wide[:, 8:8 + cols] = a
    w = T(wide)
    v = w[:, 8:8 + cols]
    assert v.data_ptr() % 16 == 0 and (rows == 1 or v.stride(0) == cols + 16)
    return v


@pytest.mark.parametrize("rows,cols", X.C_SHAPES)
def test_scale_at_its_seams(rows, cols):
    from cplxmodule_amd import x3
    for name, (a, b, op) in X.scale_seam_inputs(rows, cols).items():
        want = np.array(X.emulate_absmax_scale(a, b, op), dtype=np.float32)
        assert want[0] == np.float32(2.0 ** X.SCALE_EXPECT[name])
        got = N(x3.scale_of(T(a), None if b is None else T(b), op))
        assert np.array_equal(got, want), (name, got, want)
        if rows > 1:                                         # a strided source: the padding holds larger values and NaN
            got = N(x3.scale_of(_strided(a, 3.0e38), None if b is None else _strided(b, 3.0e38), op))
            assert np.array_equal(got, want), (name, "strided", got, want)


@pytest.mark.parametrize("n", X.PARTIAL_COUNTS)
def test_scale_from_partials(n):
    from cplxmodule_amd._lib import call, ptr, stream_ptr
    p, m = X.partial_inputs(n)
    part, out = T(p), torch.full((2,), float("nan"), device="cuda")
    call("cplxamd_absmax_scale_partials", ptr(part), n, ptr(out), stream_ptr())
    assert np.array_equal(N(out), np.array(X.scale_from_max(m), dtype=np.float32)), (n, N(out))


# ---- C: the half split ----------------------------------------------------------------------------------------------------
def _pieces_of(p, pattern, stacked, cols):
    """The piece planes of a Pieces tensor in storage order."""
    n = 2 if pattern == 0 else 3
    return [p.t[j] for j in range(n)] if stacked else [p.t[:, j * cols:(j + 1) * cols] for j in range(n)]


@pytest.mark.parametrize("stacked", (False, True))
@pytest.mark.parametrize("pattern", (0, 1))
@pytest.mark.parametrize("rows,cols", X.C_SHAPES)
def test_split2h_at_its_seams(rows, cols, pattern, stacked):
    """Normal halves, subnormal halves, flush to zero, exact ties, -0: every piece equals the emulation bit for bit, in both
    patterns (A: h1 h0, B: w1 w0 w0) and both layouts; so do a strided source, the |x|^2 and exp operands, and a stale scale."""
    from cplxmodule_amd import ops, x3
    x = X.split_seam_input(rows, cols)
    sc = x3.scale_of(T(x))
    s = X.emulate_absmax_scale(x)
    assert np.array_equal(N(sc), np.array(s, dtype=np.float32)) and s[0] == 2.0 ** X.SPLIT_S
    order = (1, 0) if pattern == 0 else (1, 0, 0)             # which emulated piece each stored plane holds

    def check(p, want, what):
        assert p.t.dtype == torch.float16
        for j, (got, k) in enumerate(zip(_pieces_of(p, pattern, stacked, cols), order)):
            assert _same_halves(got, want[k]), (what, "stored plane", j)

    want = X.emulate_split2h(x, s[0])
    check(x3.split(T(x), pattern, kind="x2", stacked=stacked, scale=sc), want, "dense")
    if rows > 1:
        check(x3.split(_strided(x, 3.0e38), pattern, kind="x2", stacked=stacked, scale=sc), want, "strided")
    # a stale scale, 16 times too large: the first piece overflows to inf, the second is 0 -- what a wrong scale hint would do
    stale = T(np.array([s[0] * 16, s[1] / 16], dtype=np.float32))
    wst = X.emulate_split2h(x, s[0] * np.float32(16))
    assert np.isinf(wst[0].astype(np.float64)).any() and not wst[1][np.isinf(wst[0].astype(np.float64))].any()
    check(x3.split(T(x), pattern, kind="x2", stacked=stacked, scale=stale), wst, "stale scale")
    if pattern == 0 and not stacked:
        y = X.split_seam_input(cols, rows).T.copy()           # a second plane
        sa = X.emulate_absmax_scale(x, y, X.OP_ABS2)
        p = x3.split(T(x), op=x3.OP_ABS2, t2=T(y), kind="x2")
        assert np.array_equal(N(p.scale), np.array(sa, dtype=np.float32))
        check(p, X.emulate_split2h(x, sa[0], y, X.OP_ABS2), "|x|^2")
        z = (np.log(np.abs(x) + 1e-30)).astype(np.float32)    # exp(z) spans the same range; the device's expf decides the bits
        ez = N(ops.exp(T(z)))
        se = X.emulate_absmax_scale(None, op=X.OP_EXP, value=ez)
        p = x3.split(T(z), op=x3.OP_EXP, kind="x2")
        assert np.array_equal(N(p.scale), np.array(se, dtype=np.float32))
        check(p, X.emulate_split2h(None, se[0], op=X.OP_EXP, value=ez), "exp")


@pytest.mark.parametrize("rows,cols", X.C_SHAPES)
def test_split3_matches_the_emulation(rows, cols):
    from cplxmodule_amd import x3
    x = X.split_seam_input(rows, cols)
    want = X.emulate_split3(x)
    a = x3.split(T(x)).t                                    # [x2 | x1 | x0]
    for j, k in enumerate((2, 1, 0)):
        assert torch.equal(a[:, j * cols:(j + 1) * cols].float(), T(want[k])), j


# ---- D: power-of-two invariance of the launch sequences -------------------------------------------------------------------
def _drive(lay, kind, M, N_, K, a, b, bias=None, c0=None):
    """One launch sequence of x3.py on float32 operand planes (numpy; 1 plane: real, 2: complex) -> tuple of result planes.
    NN: A B^T + bias.  NT: A conj(Bk) with Bk = B^T stored [K, N].  TT: Ak^T conj(Bk) + BETA * c0, both K-major."""
    from cplxmodule_amd import x3
    cplx = len(a) == 2
    At, Bt = [T(v) for v in a], [T(v) for v in b]
    sp = lambda ts, *args, **k: x3.split_planes(tuple(ts), *args, kind=kind, **k)  # noqa: E731
    if lay == "NN":
        bt = None if bias is None else tuple(T(v) for v in bias)
        got = x3.gemm_nn(sp(At), sp(Bt, x3.SPLIT_B), M, N_, K, bias=bt if cplx or bt is None else bt[0])
    elif lay == "NT":
        got = x3.gemm_nt(sp(At), sp([v.t().contiguous() for v in Bt], x3.SPLIT_B, stacked=True), M, N_, K, conj_b=cplx)
    else:
        Ak, Bk = [v.t().contiguous() for v in At], [v.t().contiguous() for v in Bt]
        if c0 is None:
            got = x3.gemm_tt(sp(Ak), sp(Bk), M, N_, K, conj_b=cplx)
        else:
            out = tuple(T(v) for v in c0)
            got = x3.gemm_tt(sp(Ak), sp(Bk), M, N_, K, conj_b=cplx, out=out if cplx else out[0], accumulate=True,
                             beta=torch.tensor(X.BETA, device="cuda"))
    return got if isinstance(got, tuple) else (got,)


def _launches(lay, kind, K):
    """(K of the launch, plan epilogue code) per launch of a sequence: K-concatenated pieces for NN / NT (x3.py _SEQ), one
    launch per piece pair for TT; every launch but the first of NN / NT accumulates."""
    if lay == "TT":
        return [(K, 2)]
    return [(n * K, 0 if i == 0 else 2) for i, n in enumerate((1, 2) if kind == "x2" else (1, 2, 3))]


def _first_bad(got, want):
    bad = ~(got == want)
    n = int(bad.sum())
    if not n:
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{n} of {bad.numel()} differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}"


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("M,N_,K", X.SHAPES)
@pytest.mark.parametrize("kind", ("x2", "x3"))
@pytest.mark.parametrize("cplx", (False, True))
@pytest.mark.parametrize("lay", X.LAYOUTS)
def test_power_of_two_invariance(lay, cplx, kind, M, N_, K, family):
    """gemm(A 2^p, B 2^q, bias 2^(p+q)) == gemm(A, B, bias) 2^(p+q) bit for bit: the scales adapt, the pieces are the same
    bits, the undo and the bias must not care where the exponents sit.  'x3' has no scales: the control -- bit-exact while
    its unscaled partial sums stay normal (p + q >= -65), within the flushes of subnormal partial sums below (measured on
    the MI355X: one element of 65536 of one case, complex TT 256 x 256 x 128 at (-60, -45), differs, by 2^-132 on a result of
    2^-110 that is the remainder of a cancellation; every other 'x3' case is bit-exact on every pair).  Then the base case
    against float64 inside the derived bound, tiny operands against an unscaled bias, and one pair beyond the clip."""
    from cplxmodule_amd import _lib
    flags = FLAGS[family]
    ta, tb = lay == "TT", lay != "NN"
    for Kl, epi in _launches(lay, kind, K):                  # the family that runs, by the dispatcher's dry run
        on_device = _lib.load().cplxamd_gemm_plan(int(cplx), M, N_, Kl, int(ta), int(tb), G.DTYPE_CODE["f32"], epi, flags, 0)
        assert on_device == X.expected_kind(family, M, N_, Kl, cplx), (Kl, G.KIND_NAME.get(on_device))
    d = X.invariance_operands(M, N_, K, cplx)
    problems = []
    with _lib.launch_policy(flags):
        run = lambda a, b, bias, c0: _drive(lay, kind, M, N_, K, a, b, bias if lay == "NN" else None,  # noqa: E731
                                            c0 if lay == "TT" else None)
        base = run(d["a"], d["b"], d["bias"], d["c0"])
        for p, q in X.PAIRS[1:]:
            got = run(X.shifted(d["a"], p), X.shifted(d["b"], q), X.shifted(d["bias"], p + q), X.shifted(d["c0"], p + q))
            for pl, (g, g0) in enumerate(zip(got, base)):
                want = g0 * 2.0 ** (p + q)
                msg = _first_bad(g, want)
                if msg and kind == "x3" and p + q < X.X3_EXACT_FROM:
                    # subnormal partial sums in unscaled accumulators (x2_range_cases.X3_EXACT_FROM): flushes + one rounding
                    print(f"x3 ({p}, {q}) plane {pl}: {msg}")
                    tol = X.x3_flush_allowance(K, cplx) + want.abs().double() * 2.0 ** -23
                    msg = "" if bool(((g.double() - want.double()).abs() <= tol).all()) else msg + " (beyond the flush allowance)"
                if msg:
                    problems.append(f"(p, q) = ({p}, {q}), plane {pl}: {msg}")
        # the base case against float64
        ref = X.reference(d["a"], d["b"], conj_b=cplx and lay != "NN")
        head, extra = (None, 0) if lay == "NT" else ((d["bias"], 1) if lay == "NN" else (tuple(X.BETA * v for v in d["c0"]), 2))
        if head is not None:
            ref = tuple(r + h.astype(np.float64) for r, h in zip(ref, head))
        bd = (X.cplx_bound(kind, *d["a"], *d["b"], head=head, extra=extra) if cplx
              else (X.bound(kind, d["a"][0], d["b"][0], head=head[0] if head else None, extra=extra),))
        for pl, (g, r, b_) in enumerate(zip(base, ref, bd)):
            err = np.abs(N(g).astype(np.float64) - r)
            if not (err <= b_).all():
                problems.append(f"base case, plane {pl}: error {err.max():.3e} at {np.unravel_index((err / b_).argmax(), err.shape)}"
                                f" exceeds the bound by a factor {(err / b_).max():.2f}")
        if lay == "NN":
            # tiny operands, a bias of order 1 -- and none of 0: fl32(bias + product) is the bias (the products are 2^-96
            # and smaller); a zero bias changes nothing about the product, which float32 holds as a normal number
            p, q = X.TINY
            a, b = X.shifted(d["a"], p), X.shifted(d["b"], q)
            zero = tuple(np.zeros_like(v) for v in d["bias"])
            for pl, (g, z, g0, bi) in enumerate(zip(run(a, b, d["bias"], None), run(a, b, zero, None),
                                                    _drive(lay, kind, M, N_, K, a, b), d["bias"])):
                msg = _first_bad(g, T(bi).expand_as(g))
                if msg:
                    problems.append(f"tiny operands + bias of order 1, plane {pl}: {msg}")
                msg = _first_bad(z, g0)
                if msg or not bool((g0 != 0).all()):
                    problems.append(f"tiny operands + zero bias vs no bias, plane {pl}: {msg}; zeros: {int((g0 == 0).sum())}")
        if kind == "x2":
            # beyond the clip (k = 137 -> 120): no invariance; finite and inside the bound with the clipped scale
            p, q = X.BEYOND_CLIP
            a, b = X.shifted(d["a"], p), X.shifted(d["b"], q)
            ref = X.reference(a, b, conj_b=cplx and lay != "NN")
            bd = X.cplx_bound(kind, *a, *b) if cplx else (X.bound(kind, a[0], b[0]),)
            for pl, (g, r, b_) in enumerate(zip(_drive(lay, kind, M, N_, K, a, b), ref, bd)):
                err = np.abs(N(g).astype(np.float64) - r)
                if not (np.isfinite(N(g)).all() and (err <= b_).all()):
                    problems.append(f"beyond the clip, plane {pl}: error / bound up to {(err / b_).max():.2f}")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("p,q", ((-52, -52), (58, 58)))
def test_x2_convolution_power_of_two_invariance(p, q):
    """CplxConv2d(64, 64, 3, padding=1) float32 on half pieces, batch 1, 16 x 32, channels-last: the forward with a bias
    (x 2^p, w 2^q, bias 2^(p+q)), the input gradient (g 2^q, w 2^q) and the weight gradient (g 2^q, x 2^p) are the base
    case's bits times the power of two."""
    from cplxmodule_amd import Cplx, conv, nn, x3
    rs = X._rs("conv")
    cl = lambda v: T(v).contiguous(memory_format=torch.channels_last)  # noqa: E731
    x = [X.dyadic(rs, (1, 64, 16, 32), -6, 2) for _ in range(2)]
    g = [X.dyadic(rs, (1, 64, 16, 32), -9, -1) for _ in range(2)]
    w = [X.dyadic(rs, (64, 64, 3, 3), -9, -1) for _ in range(2)]
    b = [X.dyadic(rs, (64,), -3, 1) for _ in range(2)]

    def run(p, q):
        layer = nn.CplxConv2d(64, 64, 3, padding=1).cuda()
        with torch.no_grad():
            for dst, src in zip((layer.weight.real, layer.weight.imag, layer.bias.real, layer.bias.imag),
                                X.shifted(w, q) + X.shifted(b, p + q)):
                dst.copy_(T(src))
        xr, xi = (cl(v).requires_grad_(True) for v in X.shifted(x, p))
        with x3.fp32_mode("x2"):
            assert conv._x2_conv_kind(conv._geom(xr.shape, layer.weight.real.shape, 1, 1, 1, 1)[0], xr, xi, layer.weight.real,
                                      layer.weight.imag) == "x2"
            y = layer(Cplx(xr, xi))
            torch.autograd.backward((y.real, y.imag), tuple(cl(v) for v in X.shifted(g, q)))
        return {k: v.detach() for k, v in dict(yr=y.real, yi=y.imag, dxr=xr.grad, dxi=xi.grad, dwr=layer.weight.real.grad,
                                               dwi=layer.weight.imag.grad).items()}

    base, got = run(0, 0), run(p, q)
    shift = dict(yr=p + q, yi=p + q, dxr=2 * q, dxi=2 * q, dwr=p + q, dwi=p + q)
    problems = []
    for k, t in got.items():
        assert bool(torch.isfinite(base[k]).all()) and float(base[k].abs().max()) > 0
        msg = _first_bad(t, base[k] * 2.0 ** shift[k])
        if msg:
            problems.append(f"{k}: {msg}")
    assert not problems, "\n".join(problems)


# ---- E: rows of one operand scaled block by block -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("x2", "x3"))
@pytest.mark.parametrize("side", ("a", "b"))
@pytest.mark.parametrize("cplx", (False, True))
def test_row_range_of_the_raw_products(cplx, side, kind):
    """Blocks of rows of A (then of B) carry 2^-r, r = 0 .. 45: every element inside the derived bound against float64;
    'x2' returns exact zeros where the rows lie 2^-41 and more below the operand's maximum (and nowhere else), 'x3' returns
    the unscaled product's rows times 2^-r bit for bit -- accurate at each row's own magnitude."""
    M, N_, K = X.E_SHAPE
    a0, b0, r = X.row_range_operands(cplx, side)
    a, b = (X.scale_rows(a0, r), b0) if side == "a" else (a0, X.scale_rows(b0, r))
    got = _drive("NN", kind, M, N_, K, a, b)
    ref = X.reference(a, b)
    bd = X.cplx_bound(kind, *a, *b) if cplx else (X.bound(kind, a[0], b[0]),)
    base = _drive("NN", kind, M, N_, K, a0, b0) if kind == "x3" else (None,) * len(got)
    for g, g0, rf, b_ in zip(got, base, ref, bd):
        g = N(g)
        err = np.abs(g.astype(np.float64) - rf)
        assert (err <= b_).all(), (kind, float((err / b_).max()))
        rows = g if side == "a" else g.T
        if kind == "x2":
            assert not rows[r >= X.ZERO_FROM].any() and rows[r < X.ZERO_FROM].all()
        else:
            want = np.ldexp(N(g0) if side == "a" else N(g0).T, -r[:, None])
            assert np.array_equal(rows, want)


# ---- F: the layers, sample by sample ------------------------------------------------------------------------------------------
_F_REF = {}


def _layer_reference(cplx):
    """Inputs of section F and the float64 oracle's outputs and gradients (computed once per process)."""
    if cplx not in _F_REF:
        d = X.layer_inputs(cplx)
        f = lambda t: t.astype(np.float64)  # noqa: E731
        if cplx:
            args = (f(d["x"][0]), f(d["x"][1]), f(d["w"][0]), f(d["w"][1]))
            yr, yi, aux = orc.lrt_cplx_linear(*args, f(d["b"][0]), f(d["b"][1]), f(d["ls2"]), f(d["eps"][0]), f(d["eps"][1]))
            bw = orc.lrt_cplx_linear_bwd(f(d["g"][0]), f(d["g"][1]), *args, f(d["ls2"]), f(d["eps"][0]), f(d["eps"][1]))
            ref = dict(yr=yr, yi=yi, dxr=bw["dxr"], dxi=bw["dxi"], dwr=bw["dwr"], dwi=bw["dwi"], dls2=bw["dlog_sigma2"],
                       dbr=f(d["g"][0]).sum(0), dbi=f(d["g"][1]).sum(0))
        else:
            y, aux = orc.lrt_real_linear(f(d["x"][0]), f(d["w"][0]), f(d["b"][0]), f(d["ls2"]), f(d["eps"][0]))
            bw = orc.lrt_real_linear_bwd(f(d["g"][0]), f(d["x"][0]), f(d["w"][0]), f(d["ls2"]), f(d["eps"][0]))
            ref = dict(y=y, dx=bw["dx"], dw=bw["dw"], dls2=bw["dlog_sigma2"], db=bw["db"])
        assert aux["s2"].min() > 50 * X.CLAMP
        _F_REF[cplx] = (d, ref)
    return _F_REF[cplx]


@pytest.mark.parametrize("mode", ("exact", "x3", "auto"))
@pytest.mark.parametrize("cplx", (True, False))
def test_lrt_layers_per_sample(cplx, mode, monkeypatch):
    """CplxLinearVD(64, 96) / LinearVD(64, 96), batch 128, training mode, explicit noise: y and dx row by row (per sample),
    dW, dlog_sigma2 and db row by row (per output unit) within 1e-5 of that row's own largest reference value.  The samples
    span 2^14 in magnitude (|x|^2: 2^28), the output units' variances 2^21.  'auto' is made to take the split path."""
    from cplxmodule_amd import cplx as cx, x3
    from cplxmodule_amd.nn import relevance as rel
    import test_gpu_x3 as tx
    d, ref = _layer_reference(cplx)
    monkeypatch.setattr(x3, "AUTO_MIN_WORK", 1)
    n = tx._count_splits(monkeypatch)
    if cplx:
        layer = rel.CplxLinearVD(X.F_I, X.F_O).to("cuda")
        layer.load_state_dict({"weight.real": T(d["w"][0]), "weight.imag": T(d["w"][1]), "bias.real": T(d["b"][0]),
                               "bias.imag": T(d["b"][1]), "log_sigma2": T(d["ls2"])})
        xr, xi = T(d["x"][0]).requires_grad_(True), T(d["x"][1]).requires_grad_(True)
        layer.train()
        with x3.fp32_mode(mode):
            y = layer(cx.Cplx(xr, xi), eps=cx.Cplx(T(d["eps"][0]), T(d["eps"][1])))
        torch.autograd.backward((y.real, y.imag), (T(d["g"][0]), T(d["g"][1])))
        got = dict(yr=y.real, yi=y.imag, dxr=xr.grad, dxi=xi.grad, dwr=layer.weight.real.grad, dwi=layer.weight.imag.grad,
                   dls2=layer.log_sigma2.grad, dbr=layer.bias.real.grad, dbi=layer.bias.imag.grad)
    else:
        layer = rel.LinearVD(X.F_I, X.F_O).to("cuda")
        layer.load_state_dict({"weight": T(d["w"][0]), "bias": T(d["b"][0]), "log_sigma2": T(d["ls2"])})
        x = T(d["x"][0]).requires_grad_(True)
        layer.train()
        with x3.fp32_mode(mode):
            y = layer(x, eps=T(d["eps"][0]))
        y.backward(T(d["g"][0]))
        got = dict(y=y, dx=x.grad, dw=layer.weight.grad, dls2=layer.log_sigma2.grad, db=layer.bias.grad)
    problems = []
    if (n["split"] > 0) != (mode != "exact"):                # the split path ran -- and only where asked for
        problems.append(f"x3.split ran {n['split']} times")
    for k, t in got.items():
        worst, bad = X.row_check(N(t), ref[k])
        print(f"{mode} {k}: worst row at {worst:.3f} of the tolerance")
        if len(bad):
            problems.append(f"{k}: {len(bad)} rows miss 1e-5 of their own max|ref| (worst {worst:.1f} x), first rows {bad[:8].tolist()}")
    assert not problems, f"fp32 mode {mode!r}\n" + "\n".join(problems)
