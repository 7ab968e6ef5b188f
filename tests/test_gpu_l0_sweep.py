"""The kernels that draw random numbers in registers -- csrc/l0.hip (hard-concrete gate, LASSO mask) and the index space of
csrc/reparam.hip -- over the cases of tests/l0_sweep_cases.py, against its float64 numpy oracle and its bounds (derived there;
none comes from a kernel's output).  tests/test_l0_sweep_host.py shows without a GPU that every case reaches the branch it is
named for and that a float32 restatement of the gate meets a quarter of the bounds on the same data.

Every wrapped case has one structure: the tape form (uniforms / noise supplied) is held to the oracle over the WHOLE tensor;
the Philox form must equal the tape form fed the materialised stream bit for bit, from a host (seed, offset) and from a
device int64[2] position alike; and the materialised stream equals oracle/philox.py on windows at the head, around every
multiple of the scalar and 8-wide wrap lengths, and at the tail.  Philox cases use seed 2^64 - 1, offset 2^40 + 3.

Groups: A elementwise gate index space; B per-column forward (column step dc != 0 beyond the first trip); C per-column
backward plans; D directed edge values; E dtype routes; F LASSO mask; G LRT noise injection; H empty shapes; I graph replay.
`pytest -m gpu -s` prints the worst error / bound of every case as `l0_sweep <case>: ...`.

Measured worst error / bound on an MI355X (one run of this file; the hardware reciprocal and the device expf /
logf are inside the float32 gate figures):
  A  z 0.044, a z 0.042, d z 0.044, term 0.019 (n = 2 L8 + 24 and L8 - 8, train)
  B  a z 0.044, a z + bias 0.491 (116600 x 72: the rounding of the bias sum), z 0.046, z + bias 0.047, total 0.005
  C  d z 0.040, a z 0.039, column sums 0.006
  D  z 0.018, dz 0.002
  E  float32 outputs 0.41, bf16 outputs 0.994 (their own rounding), column sums 0.001, term 0.017
  G  noise 0.474, float32 y 0.496, g_s2 0.018; bf16 y 0.996 and bf16 g_s2 0.993 (their own rounding); bias sums 0.012
The given-noise forms of G are held to the float32 one-rounding-per-op chain of test_reparam_given_noise, whose tolerances
they take (those tolerances are relative to |y| and do not cover a float64 reference where mu and eps sd cancel).

What the sweep found, and the kernels now handle:
  * cplxamd_l0_gate_bwd returned on rows = 0 before writing anything, so a per-column d log_alpha came back as whatever the
    buffer held (LinearL0(group="input" / "output") on a [0, I] batch: gradients like 1.6e29); it is zeroed on the stream;
  * cplxamd_lrt_reparam_fwd / _bwd and cplxamd_philox_normal launched one idle block on an empty operand; they return first.
With the column step of l0_fwd_kernel off by one vector, or the counter of uniforms8 wrong beyond the first trip, the wrapped
cases of B and A fail.
"""
import numpy as np
import pytest
import torch

import l0_sweep_cases as lc
from gpu_util import DEV, N, T

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
COLS, TRAIN, HARD = 1, 2, 4


@pytest.fixture(scope="module")
def l0():
    from cplxmodule_amd import l0
    return l0


@pytest.fixture(scope="module")
def ops():
    from cplxmodule_amd import ops
    return ops


def _state():
    """the Philox position of every case as a device int64[2] (the same 64 bits of the seed, as int64)"""
    return torch.tensor([lc.SEED - (1 << 64), lc.OFFSET], dtype=torch.int64, device=DEV)


def _f64(t):
    return t.detach().double().cpu().numpy()


def _ratio(got, ref, bound, sel=None):
    """worst |got - ref| / bound over `sel` (all); a non-finite output is a failure wherever it is"""
    got = _f64(got).reshape(np.shape(ref))
    assert np.isfinite(got).all(), "non-finite output"
    err, bound = np.abs(got - ref), np.broadcast_to(bound, np.shape(ref))
    if sel is not None:
        err, bound = err[sel], bound[sel]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def _report(case, **ratios):
    print(f"\nl0_sweep {case}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, (case, over)


_PINNED = {}


def _uniforms(l0, n):
    """the materialised stream of n elements at (SEED, OFFSET), pinned to oracle/philox.py on the windows of n"""
    if n not in _PINNED:
        _PINNED.clear()
        u = l0.philox_uniform(n, lc.SEED, lc.OFFSET, DEV)
        for a, b in lc.windows(n):
            np.testing.assert_array_equal(N(u[a:b]), lc.uniform_window(a, b), err_msg=f"stream window [{a}, {b}) of {n}")
        _PINNED[n] = u
    return _PINNED[n]


def _same(a, b, what):
    for x, y in zip(a, b):
        if x is None and y is None:
            continue
        assert x.dtype == y.dtype and torch.equal(x, y), what


# ---- A: index space of the elementwise gate -----------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n", lc.A_SIZES)
def test_elementwise_index_space(l0, n, train):
    la_h, a_h, d_h = lc.elem_data(n)
    la, a, d = T(la_h), T(a_h), T(d_h)
    mode = TRAIN if train else 0
    u = _uniforms(l0, n) if train else None
    z, dz, pre = lc.gate64(la_h, N(u) if train else None)
    free = ~lc.band(pre)
    tape = dict(u=u) if train else {}
    out = l0.gate_fwd(a, la, 1, n, mode, **tape)
    zz = l0.gate_fwd(None, la, 1, n, mode, **tape)
    da, az, dla = l0.gate_bwd(d, a, la, 1, n, mode, az_dtype=F32, **tape)
    assert out.shape == zz.shape == da.shape == az.shape == (1, n) and dla.shape == (n,)
    ref_out, ref_da, ref_az = lc.fwd_ref(z, a_h), lc.fwd_ref(z, d_h), lc.fwd_ref(z, a_h)
    ref_t = d_h.astype(np.float64) * a_h * dz
    _report(f"A n={n} {'train' if train else 'eval'}",
            z=_ratio(zz, z, lc.TOL_Z), out=_ratio(out, ref_out, lc.out_bound(ref_out, a_h, F32)),
            da=_ratio(da, ref_da, lc.out_bound(ref_da, d_h, F32)), az=_ratio(az, ref_az, lc.out_bound(ref_az, a_h, F32)),
            term=_ratio(dla, ref_t, lc.term_bound(d_h, a_h, ref_t), free))
    assert torch.equal(az, out)                                       # A (.) z is formed the same way in both passes
    if train:
        for pos in (dict(seed=lc.SEED, offset=lc.OFFSET), dict(seed=_state())):
            _same([l0.gate_fwd(a, la, 1, n, mode, **pos), l0.gate_fwd(None, la, 1, n, mode, **pos)], [out, zz],
                  f"forward, Philox form {list(pos)}")
            _same(l0.gate_bwd(d, a, la, 1, n, mode, az_dtype=F32, **pos), [da, az, dla], f"backward, Philox form {list(pos)}")


# ---- B: per-column forward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(lc.B_CASES))
def test_cols_forward(l0, name, train):
    rows, cols = lc.B_CASES[name][:2]
    n = rows * cols
    la_h, a_h, _, bias_h = lc.cols_data(rows, cols)
    la, a, bias = T(la_h), T(a_h), T(bias_h)
    mode = COLS | (TRAIN if train else 0)
    u = _uniforms(l0, n) if train else None
    z, _, pre = lc.gate64(la_h[None, :], N(u).reshape(rows, cols) if train else None)
    z, pre = np.broadcast_to(z, (rows, cols)), np.broadcast_to(pre, (rows, cols))
    inband = lc.band(pre)
    tape = dict(u=u) if train else {}
    positions = (dict(seed=lc.SEED, offset=lc.OFFSET), dict(seed=_state())) if train else ()
    ratios = {}
    for tag, av, ah, bv, bh in (("az", a, a_h, None, None), ("az+b", a, a_h, bias, bias_h), ("z", None, None, None, None),
                                ("z+b", None, None, bias, bias_h)):
        out = l0.gate_fwd(av, la, rows, cols, mode, bias=bv, **tape)
        assert out.shape == (rows, cols) and out.dtype == F32
        ref = lc.fwd_ref(z, ah, bh)
        ratios[tag] = _ratio(out, ref, lc.out_bound(ref, ah, F32))
        for pos in positions:
            assert torch.equal(l0.gate_fwd(av, la, rows, cols, mode, bias=bv, **pos), out), (tag, list(pos))
    # the soft gate's total: the float64 sum of the outputs (8 of them summed in float32 first, then in double)
    soft, tot = l0.gate_fwd(None, la, rows, cols, mode, total=True, **tape)
    s = soft.double()
    assert abs(float(tot) - float(s.sum())) <= 8 * 2.0 ** -24 * float(s.abs().sum())
    ratios["total_z"] = abs(float(tot) - float(z.sum())) / (n * lc.TOL_Z)
    # the hard mask and its count: exact outside the clamp band, one per element inside it
    hard, cnt = l0.gate_fwd(None, la, rows, cols, mode | HARD, total=True, **tape)
    hard_h = N(hard)
    assert ((hard_h == 0) | (hard_h == 1)).all()
    np.testing.assert_array_equal(hard_h[~inband], (pre > 0)[~inband].astype(np.float32))
    assert float(cnt) == float(hard.double().sum())
    assert abs(float(cnt) - float((pre > 0).sum())) <= int(inband.sum())
    for pos in positions:
        h2, c2 = l0.gate_fwd(None, la, rows, cols, mode | HARD, total=True, **pos)
        assert torch.equal(h2, hard) and torch.equal(c2, cnt)
    _report(f"B {name} {rows}x{cols} {'train' if train else 'eval'}", **ratios)


# ---- C: per-column backward plans ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(lc.C_CASES))
def test_cols_backward_plans(l0, name, train):
    rows, cols = lc.C_CASES[name][:2]
    n = rows * cols
    la_h, a_h, d_h, _ = lc.cols_data(rows, cols)
    la, a, d = T(la_h), T(a_h), T(d_h)
    mode = COLS | (TRAIN if train else 0)
    u = _uniforms(l0, n) if train else None
    z, dz, pre = lc.gate64(la_h[None, :], N(u).reshape(rows, cols) if train else None)
    z, dz, pre = (np.broadcast_to(t, (rows, cols)) for t in (z, dz, pre))
    tape = dict(u=u) if train else {}
    da, az, dla = l0.gate_bwd(d, a, la, rows, cols, mode, az_dtype=F32, **tape)
    assert da.shape == az.shape == (rows, cols) and dla.shape == (cols,)
    ref_da, ref_az = lc.fwd_ref(z, d_h), lc.fwd_ref(z, a_h)
    ref_s, bound_s = lc.colsum_ref(d_h, a_h, dz, pre)
    _report(f"C {name} {rows}x{cols} {'train' if train else 'eval'}",
            da=_ratio(da, ref_da, lc.out_bound(ref_da, d_h, F32)), az=_ratio(az, ref_az, lc.out_bound(ref_az, a_h, F32)),
            dla=_ratio(dla, ref_s, bound_s))
    # fixed order: three calls are bit-identical, in every form of the noise position
    forms = [tape] if not train else [tape, dict(seed=lc.SEED, offset=lc.OFFSET), dict(seed=_state())]
    for pos in forms:
        for _ in range(3 if pos is forms[-1] else 1):
            _same(l0.gate_bwd(d, a, la, rows, cols, mode, az_dtype=F32, **pos), [da, az, dla], (name, list(pos)))
    # D (.) z and A (.) z are those of the elementwise kernel run on the expanded log_alpha
    da_e, az_e, _ = l0.gate_bwd(d, a, la.expand(rows, cols).contiguous(), rows, cols, mode & ~COLS, az_dtype=F32, **tape)
    assert torch.equal(da_e, da) and torch.equal(az_e, az)


def test_cols_backward_chunk_cap(l0):
    """rows / 16 > 1024 chunks asked for: the cap.  No float64 oracle at this size: bit-identical reruns, and the column
    sums against the float64 sums of the elementwise kernel's terms (as test_column_reduction_is_deterministic does)."""
    rows, cols = lc.C_CAP
    g = torch.Generator(device=DEV).manual_seed(17)
    d = torch.randn(rows, cols, device=DEV, generator=g)
    a = torch.randn(rows, cols, device=DEV, generator=g).bfloat16()
    la = torch.empty(cols, device=DEV).uniform_(-3, 3, generator=g)
    mode = COLS | TRAIN
    kw = dict(seed=lc.SEED, offset=lc.OFFSET, da_dtype=BF16, az_dtype=BF16)
    first = l0.gate_bwd(d, a, la, rows, cols, mode, **kw)
    for _ in range(2):
        _same(l0.gate_bwd(d, a, la, rows, cols, mode, **kw), first, "rerun")
    da_e, az_e, terms = l0.gate_bwd(d, a, la.expand(rows, cols).contiguous(), rows, cols, TRAIN, **kw)
    assert torch.equal(da_e, first[0]) and torch.equal(az_e, first[1])
    ref = terms.double().sum(0).cpu().numpy()
    np.testing.assert_allclose(N(first[2]), ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()))


# ---- D: directed edge values --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["vector", "scalar"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_edge_values(l0, train, form):
    la_h, u_h, runs = lc.edge_table(train)
    rows, cols = la_h.shape
    if form == "scalar":                                             # the same points through the forward's scalar form
        rows, cols = 1, la_h.size - 3
    n = rows * cols
    la_h = la_h.reshape(-1)[:n]
    u_h = None if u_h is None else u_h.reshape(-1)[:n]
    la = T(la_h)
    tape = dict(u=T(u_h)) if train else {}
    mode = TRAIN if train else 0
    z64, dz64, pre = lc.gate64(la_h, u_h)
    one = torch.ones(n, device=DEV)
    z = N(l0.gate_fwd(None, la, rows, cols, mode, **tape)).reshape(-1)
    hard = N(l0.gate_fwd(None, la, rows, cols, mode | HARD, **tape)).reshape(-1)
    da, az, dz = l0.gate_bwd(one, one, la, rows, cols, mode, az_dtype=F32, **tape)
    dz = N(dz).reshape(-1)
    assert all(np.isfinite(t).all() for t in (z, hard, dz, N(da), N(az)))
    np.testing.assert_array_equal(N(da).reshape(-1), z)
    np.testing.assert_array_equal(N(az).reshape(-1), z)
    inband, outside = lc.band(pre), (pre < -lc.TOL_Z) | (pre > 1 + lc.TOL_Z)
    rz = float(np.abs(z - z64).max()) / lc.TOL_Z
    rdz = float(np.abs(dz - dz64)[~inband].max()) / lc.TOL_DZ
    print(f"\nl0_sweep D {'train' if train else 'eval'} {form}: z {rz:.3f}, dz {rdz:.3f}")
    assert rz <= 1.0 and rdz <= 1.0
    np.testing.assert_array_equal(z[outside], (pre[outside] > 1).astype(np.float32))       # clamped: exactly 0 or 1
    assert (dz[outside] == 0).all()
    np.testing.assert_array_equal(hard[~inband], (pre > 0)[~inband].astype(np.float32))
    for a, b in runs:                                                 # eval: ascending log_alpha across a boundary
        b = min(b, n)
        assert (np.diff(z[a:b]) <= 0).all() and (np.diff(hard[a:b]) <= 0).all()


# ---- E: dtype routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols_mode", [True, False], ids=["cols", "elem"])
@pytest.mark.parametrize("shape", lc.E_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dtype_routes(l0, shape, cols_mode):
    from cplxmodule_amd._lib import CplxAmdError
    rows, cols = shape
    n = rows * cols
    la_c, a_h, d_h, bias_h = lc.cols_data(rows, cols)
    u_h = lc.uniform_window(0, n)
    la_h = la_c if cols_mode else np.broadcast_to(la_c, (rows, cols)).copy()
    la, u = T(la_h), T(u_h)
    mode = TRAIN | (COLS if cols_mode else 0)
    z, dz, pre = lc.gate64(np.broadcast_to(la_c, (rows, cols)), u_h.reshape(rows, cols))
    free = ~lc.band(pre)
    pos = dict(seed=lc.SEED, offset=lc.OFFSET)
    ratios = {}
    name = lambda *ts: ">".join("b" if t == BF16 else "f" for t in ts)  # noqa: E731
    for ta, to in lc.E_FWD:
        ar = lc.rounded(a_h, ta)
        out = l0.gate_fwd(T(ar).to(ta), la, rows, cols, mode, u=u, out_dtype=to, bias=T(bias_h) if cols_mode else None)
        assert out.dtype == to
        ref = lc.fwd_ref(z, ar, bias_h if cols_mode else None)
        ratios["fwd " + name(ta, to)] = _ratio(out, ref, lc.out_bound(ref, ar, to))
        assert torch.equal(l0.gate_fwd(T(ar).to(ta), la, rows, cols, mode, out_dtype=to,
                                       bias=T(bias_h) if cols_mode else None, **pos), out)
    for td, ta, tda, taz in lc.E_BWD:
        dr, ar = lc.rounded(d_h, td), lc.rounded(a_h, ta)
        args = (T(dr).to(td), T(ar).to(ta), la, rows, cols, mode)
        da, az, dla = l0.gate_bwd(*args, u=u, da_dtype=tda, az_dtype=taz)
        assert da.dtype == tda and az.dtype == taz and dla.dtype == F32
        ref_da, ref_az = lc.fwd_ref(z, dr), lc.fwd_ref(z, ar)
        key = "bwd " + name(td, ta, tda, taz)
        ratios[key + " da"] = _ratio(da, ref_da, lc.out_bound(ref_da, dr, tda))
        ratios[key + " az"] = _ratio(az, ref_az, lc.out_bound(ref_az, ar, taz))
        if cols_mode:
            ref_s, bound_s = lc.colsum_ref(dr, ar, dz, pre)
            ratios[key + " dla"] = _ratio(dla, ref_s, bound_s)
        else:
            ref_t = dr.astype(np.float64) * ar * dz
            ratios[key + " term"] = _ratio(dla, ref_t, lc.term_bound(dr, ar, ref_t), free)
        _same(l0.gate_bwd(*args, da_dtype=tda, az_dtype=taz, **pos), [da, az, dla], key)
    td, ta, tda, taz = lc.E_BWD_REFUSED
    with pytest.raises(CplxAmdError):
        l0.gate_bwd(T(d_h).to(td), T(a_h).to(ta), la, rows, cols, mode, u=u, da_dtype=tda, az_dtype=taz)
    _report(f"E {rows}x{cols} {'cols' if cols_mode else 'elem'}", **ratios)


# ---- F: LASSO mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.F_SIZES)
def test_l1_mask(l0, n):
    w_h = lc.l1_pattern(n)
    w = T(w_h)
    for thr in lc.l1_thresholds() + (-1e30, 0.0, float("inf")):
        ref = lc.l1_ref(w_h, thr)
        mask = l0.l1_mask(w, thr)
        mask2, cnt = l0.l1_mask(w, thr, count=True)
        assert mask.dtype == torch.bool and mask.shape == w.shape
        np.testing.assert_array_equal(mask.cpu().numpy(), ref, err_msg=f"threshold {thr!r}")
        assert torch.equal(mask, mask2)
        assert float(cnt) == float(ref.sum())


# ---- G: LRT noise injection ---------------------------------------------------------------------------------------------
_NOISE = {}


def _normals(ops, n, cplx):
    """the materialised noise stream at (SEED, OFFSET), pinned to oracle/philox.py within NOISE_ATOL on the windows of n"""
    key = (n, cplx)
    if key not in _NOISE:
        _NOISE.clear()
        e = ops.philox_normal(n, lc.SEED, lc.OFFSET, DEV, complex_=cplx)
        worst = 0.0
        for a, b in lc.windows(n, seams=(lc.GRID_CAP * lc.RP_THREADS, lc.RP_L8)):
            ref = lc.normal_window(a, b, cplx)
            for got, want in zip(e if cplx else (e,), ref if cplx else (ref,)):
                worst = max(worst, float(np.abs(_f64(got[a:b]) - want).max()))
        assert worst <= lc.NOISE_ATOL, (n, cplx, worst)
        _NOISE[key] = (e, worst / lc.NOISE_ATOL)
    return _NOISE[key]


@pytest.mark.parametrize("form", lc.G_FORMS)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
@pytest.mark.parametrize("n", lc.G_SIZES)
def test_reparam_index_space(ops, n, cplx, form):
    h = lc.reparam_data(n)
    dt, st, gt = lc.reparam_dtypes(form)
    q = lambda k, t: T(h[k]).to(t)  # noqa: E731
    w = lambda t: None if t is None else t.float().cpu().numpy()  # noqa: E731      (the rounded operand, widened)
    mu_r, g_r, s2 = q("mu_r", dt), q("g_r", dt), q("s2", st)
    mu_i, g_i = (q("mu_i", dt), q("g_i", dt)) if cplx else (None, None)
    s2_h = w(s2)
    sd32 = np.sqrt(np.maximum(s2_h, np.float32(1e-8)))
    keep = s2_h >= np.float32(1e-8)
    # given noise: the float32 chain and the tolerances of test_reparam_given_noise
    e_r, e_i = q("eps_r", dt), (q("eps_i", dt) if cplx else None)
    eps = (e_r, e_i) if cplx else e_r
    y_r, y_i = ops.reparam_fwd(mu_r, mu_i, s2, eps)
    assert y_r.dtype == dt and y_r.shape == (n,)
    np.testing.assert_allclose(N(y_r), lc.given_chain32(w(mu_r), w(e_r), sd32), **lc.GIVEN_TOL[form])
    gs = w(g_r) * w(e_r)
    if cplx:
        np.testing.assert_allclose(N(y_i), lc.given_chain32(w(mu_i), w(e_i), sd32), **lc.GIVEN_TOL[form])
        gs = gs + w(g_i) * w(e_i)
    gs2 = ops.reparam_bwd(g_r, g_i, s2, eps, out_dtype=gt)
    assert gs2.dtype == gt and gs2.shape == (n,)
    tol = dict(lc.GIVEN_GS2_TOL)
    tol["rtol"] += lc.EBF if gt == BF16 else 0.0                      # a bf16 gradient: one more rounding
    np.testing.assert_allclose(N(gs2), np.where(keep, gs * np.float32(0.5) / sd32, 0), **tol)
    assert (N(gs2)[~keep] == 0).all()
    # Philox forms against the float64 oracle fed the materialised (pinned) stream
    (noise, pinned) = _normals(ops, n, cplx)
    n_r, n_i = noise if cplx else (noise, None)
    pos = dict(seed=lc.SEED, offset=lc.OFFSET)
    py_r, py_i = ops.reparam_fwd(mu_r, mu_i, s2, None, **pos)
    pgs2 = ops.reparam_bwd(g_r, g_i, s2, None, out_dtype=gt, **pos)
    ref_r, ref_i, ref_g, sd = lc.reparam_ref(w(mu_r), w(mu_i), s2_h, w(n_r), w(n_i), w(g_r), w(g_i))
    by, bg = lc.reparam_bounds(ref_r, ref_g, sd, w(g_r), w(g_i), form)
    ratios = dict(noise=pinned, y_r=_ratio(py_r, ref_r, by), g_s2=_ratio(pgs2, ref_g, bg))
    if cplx:
        ratios["y_i"] = _ratio(py_i, ref_i, lc.reparam_bounds(ref_i, ref_g, sd, w(g_r), w(g_i), form)[0])
    assert (N(pgs2)[~keep] == 0).all()
    if form == "f32":                                                 # float32: nothing is rounded on the way in
        gy_r, gy_i = ops.reparam_fwd(mu_r, mu_i, s2, (n_r, n_i) if cplx else n_r)
        _same([py_r, py_i, pgs2], [gy_r, gy_i, ops.reparam_bwd(g_r, g_i, s2, (n_r, n_i) if cplx else n_r, out_dtype=gt)],
              "Philox form against the given form fed philox_normal")
    sy_r, sy_i = ops.reparam_fwd(mu_r, mu_i, s2, None, seed=_state())
    _same([sy_r, sy_i, ops.reparam_bwd(g_r, g_i, s2, None, out_dtype=gt, seed=_state())], [py_r, py_i, pgs2],
          "device-state position")
    _report(f"G n={n} {'cplx' if cplx else 'real'} {form}", **ratios)


@pytest.mark.parametrize("mode", ["cplx_philox_bf16", "cplx_given_f32", "real_philox_f32", "real_given_bf16"])
@pytest.mark.parametrize("shape", lc.G_COLS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reparam_bias_sums_beyond_the_wrap(ops, shape, mode):
    rows, cols = shape
    cplx, philox_, bf = mode.startswith("cplx"), "philox" in mode, mode.endswith("bf16")
    dt = BF16 if bf else F32
    g = torch.Generator(device=DEV).manual_seed(rows + cols)
    mk = lambda: torch.randn(rows, cols, device=DEV, generator=g).to(dt)  # noqa: E731
    gr, gi = mk(), (mk() if cplx else None)
    s2 = (torch.rand(rows, cols, device=DEV, generator=g) * 2).to(dt)
    s2[0, :4] = 0
    s2[-1, -4:] = 0
    eps = None if philox_ else ((mk(), mk()) if cplx else mk())
    kw = dict(seed=lc.SEED, offset=lc.OFFSET, out_dtype=dt)
    flat = ops.reparam_bwd(gr, gi, s2, eps, **kw)
    got, sr, si = ops.reparam_bwd(gr, gi, s2, eps, bias_sums=(rows, cols), **kw)
    assert torch.equal(got, flat)
    assert bool((flat[0, :4] == 0).all()) and bool((flat[-1, -4:] == 0).all())
    worst = 0.0
    for t, s in ((gr, sr), (gi, si)):
        if t is None:
            continue
        ref = t.double().sum(0)
        scale = t.double().abs().sum(0).max()
        worst = max(worst, float((s.double() - ref).abs().max()) / (lc.COLSUM * float(scale)))
    _report(f"G bias sums {rows}x{cols} {mode}", colsum=worst)


# ---- H: empty shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(0, 24), (5, 0), (0, 0), (0, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_empty_shapes(l0, ops, shape):
    rows, cols = shape
    e = lambda *s, dtype=F32: torch.empty(*s, dtype=dtype, device=DEV)  # noqa: E731
    for train in (TRAIN, 0):
        for cm in (COLS, 0):
            la = torch.zeros(cols if cm else rows * cols, device=DEV)
            out, tot = l0.gate_fwd(e(rows, cols), la, rows, cols, cm | train, seed=3, offset=1, total=True,
                                   bias=torch.ones(cols, device=DEV) if cm else None)
            assert out.shape == (rows, cols) and float(tot) == 0.0
            nan = torch.full_like(la, float("nan"))
            for dla_in in (None, nan):
                da, az, dla = l0.gate_bwd(e(rows, cols), e(rows, cols, dtype=BF16), la, rows, cols, cm | train, seed=3,
                                          offset=1, da_dtype=BF16, az_dtype=BF16, dla=dla_in)
                assert da.shape == az.shape == (rows, cols) and dla.shape == la.shape
                # no rows to sum over: the per-column gradient is zero, whatever the buffer held
                assert bool((dla == 0).all()), (shape, cm, train, dla_in is None)
    mask, cnt = l0.l1_mask(e(rows, cols), 0.0, count=True)
    assert mask.shape == (rows, cols) and mask.dtype == torch.bool and float(cnt) == 0.0
    assert l0.l1_mask(e(rows, cols), 0.0).shape == (rows, cols)
    assert l0.philox_uniform(0, 1, 1, DEV).shape == (0,)
    for cplx in (False, True):
        x = e(rows, cols)
        y_r, y_i = ops.reparam_fwd(x, x.clone() if cplx else None, e(rows, cols), None, seed=3, offset=1)
        assert y_r.shape == (rows, cols) and (y_i is None) == (not cplx)
        gs2 = ops.reparam_bwd(x, x.clone() if cplx else None, e(rows, cols), None, seed=3, offset=1)
        assert gs2.shape == (rows, cols) and gs2.dtype == F32
    torch.cuda.synchronize()


def _records_nothing(fn):
    """fn captured alone in a graph (after one eager run on the capture stream, which creates the cached workspaces
    outside the capture): torch reports an empty graph when no kernel, copy or memset node was recorded"""
    import warnings
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            keep = fn()
    del keep, graph
    return any("Graph is empty" in str(w.message) for w in caught)


@pytest.mark.parametrize("shape", [(0, 24), (5, 0)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_empty_operands_launch_nothing(l0, ops, shape):
    """On an empty operand no entry point launches; the exceptions write a result that exists all the same: the totals
    (one block summing no partials) and the zeroing of the per-column gradient when there are columns but no rows."""
    rows, cols = shape
    x, xb = torch.empty(rows, cols, device=DEV), torch.empty(rows, cols, device=DEV, dtype=BF16)
    x2 = torch.empty(rows, cols, device=DEV)
    lac, lae = torch.zeros(cols, device=DEV), torch.zeros(rows * cols, device=DEV)
    pos = dict(seed=3, offset=1)
    calls = {
        "gate_fwd elem": (lambda: l0.gate_fwd(x, lae, rows, cols, TRAIN, **pos), True),
        "gate_fwd cols": (lambda: l0.gate_fwd(x, lac, rows, cols, COLS | TRAIN, bias=lac, **pos), True),
        "gate_fwd total": (lambda: l0.gate_fwd(None, lac, rows, cols, COLS, total=True), False),
        "gate_bwd elem": (lambda: l0.gate_bwd(x, xb, lae, rows, cols, TRAIN, da_dtype=BF16, az_dtype=BF16, **pos), True),
        "gate_bwd cols": (lambda: l0.gate_bwd(x, xb, lac, rows, cols, COLS | TRAIN, da_dtype=BF16, az_dtype=BF16, **pos),
                          cols == 0),
        "l1_mask": (lambda: l0.l1_mask(x, 0.0), True),
        "l1_mask count": (lambda: l0.l1_mask(x, 0.0, count=True), False),
        "philox_uniform": (lambda: l0.philox_uniform(0, 3, 1, DEV), True),
        "philox_normal": (lambda: ops.philox_normal(0, 3, 1, DEV, complex_=True), True),
        "reparam_fwd": (lambda: ops.reparam_fwd(x, x2, x, None, **pos), True),
        "reparam_fwd given": (lambda: ops.reparam_fwd(xb, None, x, xb), True),
        "reparam_bwd": (lambda: ops.reparam_bwd(x, None, x, None, **pos), True),
        "reparam_bwd given": (lambda: ops.reparam_bwd(xb, xb, xb, (xb, xb), out_dtype=BF16), True),
    }
    for name, (fn, nothing) in calls.items():
        assert _records_nothing(fn) == nothing, name


@pytest.mark.parametrize("group", ["input", "output"])
def test_empty_batch_gives_a_zero_gate_gradient(group):
    """LinearL0 with a per-sample gate on a [0, I] batch: log_alpha's gradient is a sum over no rows"""
    from cplxmodule_amd.nn.relevance import LinearL0
    layer = LinearL0(24, 16, group=group).to(DEV).train()
    x = torch.empty(0, 24, device=DEV, requires_grad=True)
    y = layer(x)
    assert y.shape == (0, 16)
    y.sum().backward()
    g = layer.log_alpha.grad
    assert g is not None and g.shape == layer.log_alpha.shape and bool((g == 0).all())
    assert x.grad.shape == (0, 24)


# ---- I: graph replay ----------------------------------------------------------------------------------------------------
def test_graph_replays_a_wrapped_cols_step(l0, ops):
    """One captured step holding a wrapped per-column forward and backward on the device-resident noise position: each
    replay draws the next offset and equals the eager run at that position bit for bit."""
    from cplxmodule_amd.utils.graphs import GraphedStep
    rows, cols = lc.B_CASES["dc304"][:2]
    la_h, a_h, d_h, bias_h = lc.cols_data(rows, cols)
    la, a, d, bias = T(la_h), T(a_h), T(d_h), T(bias_h)
    mode = COLS | TRAIN
    state = _state()

    def step(a_, d_):
        used = ops.philox_advance(state)
        out = l0.gate_fwd(a_, la, rows, cols, mode, seed=used, bias=bias)
        return (out,) + tuple(l0.gate_bwd(d_, a_, la, rows, cols, mode, seed=used, az_dtype=F32))

    gs = GraphedStep(step, (a, d))
    outs, offs = [], []
    for _ in range(2):
        offs.append(int(state[1].item()))
        res = gs.replay()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in res])
    assert offs[1] == offs[0] + 1 and offs[0] > lc.OFFSET
    assert not torch.equal(outs[0][0], outs[1][0])
    for off, got in zip(offs, outs):
        want = (l0.gate_fwd(a, la, rows, cols, mode, seed=lc.SEED, offset=off, bias=bias),) + tuple(
            l0.gate_bwd(d, a, la, rows, cols, mode, seed=lc.SEED, offset=off, az_dtype=F32))
        _same(got, want, f"replay at offset {off}")
