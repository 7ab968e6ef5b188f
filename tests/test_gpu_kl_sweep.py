"""The KL penalty kernels (csrc/kl.hip) at every branch seam and edge input of tests/kl_sweep_cases.py, against the
cancellation-free float64 reference oracle.cplx_oracle.penalty_exact / penalty_bwd on the float32 inputs.

Per-element bounds (kl_sweep_cases.bounds; the constants are those of tests/test_gpu_vd.py, the conditioning term is new):
  value   2e-6 |f| + 8 eps32 |f'(t)| (|ls2| + |ln(|w|^2 + 1e-24)|) + 1e-37
  d ls2   2e-5 |ref| + 8 eps32 |g|
  d w     2e-5 |ref| + 8 eps32 |g| max(2 / (|w| + 1e-12), 1)
No element is masked out: the case table asserts that no family has a non-finite reference anywhere.

Measured worst error / bound on an MI355X (pytest -m gpu -s prints them; value, d ls2, d w over the three entry points):
  kind               switch                range                 mixed                 edge
  real_vd            0.100 0.088 0.089     0.168 0.080 0.081     0.136 0.054 0.053     0.084 0.019 0.017
  real_ard           0.102 0.064 0.063     0.171 0.073 0.073     0.139 0.046 0.045     0.084 0.016 0.017
  cplx_vd            0.062 0.020 0.018     0.069 0.025 0.023     0.143 0.048 0.050     0.084 0.023 0.025
  cplx_ard           0.092 0.075 0.074     0.170 0.084 0.085     0.140 0.058 0.059     0.084 0.018 0.022
  cplx_vd_approx     0.093 0.083 0.081     0.172 0.091 0.089     0.141 0.063 0.061     0.084 0.021 0.022
  cplx_vd_scalefree  0.463 0.032 0.069     0.737 0.030 0.081     0.133 0.016 0.055     0.030 0.006 0.022
  cplx_vd_bogus      0.093 0.081 0.081     0.087 0.096 0.097     0.137 0.068 0.066     0.046 0.023 0.025
  tail sizes 1 ... 1027, all four entry points: real_vd 0.128, real_ard 0.126, cplx_vd 0.057, cplx_ard 0.144,
  cplx_vd_approx 0.145, cplx_vd_scalefree 0.098, cplx_vd_bogus 0.074, real_l0 0.083, real_l1 0.000
  grid wrap (n = 2 097 167): cplx_vd 0.069 0.025 0.022, real_vd 0.168 0.080 0.079
  packed against generic cplx_vd path, difference / (2 x bound): value 0.071, d ls2 0.020, d w 0.020
With x <= 1 turned into x < 1 in cplx_vd_pair the table does not move; without the -1/4 coefficient cplx_vd fails in every
family.

What the sweep found, and kl.hip now handles:
  * the t > 88.7 elements of the edge family returned +inf on the packed cplx_vd path (x = |w|^2 exp(-ls2) overflows); lanes
    with x >= 2^100 or a non-finite x take the lane's generic redo;
  * the two extension kinds whose VALUE crosses zero while its terms do not missed the value bound there, by an absolute
    float32 ulp of a term: cplx_vd_scalefree, (f - gamma) / 2 - ls2 / 2 near ls2 = f - gamma (range: 3 of 16384 elements,
    error / bound 1.97; mixed: 6.46, an error of 3.3e-9 = half the distance of the float32 constant from Euler's gamma),
    and cplx_vd_bogus, t itself near 0 with |w| ~ 1 and ls2 ~ 0 (switch: 12 of 1200, 6.71, 1.5e-7 from the 1-ulp square
    root).  Those elements redo the cancelling sum in double (kl_elem_value); on the goldens one cplx_vd_scalefree value
    of 480 moves, by 5.6e-9 towards the float64 value, every other output of every kind is bit-identical.
The sub-1e-26 weights never reach a subnormal denominator (|w|^2 underflows to 0 in float32 first: theta is 0 or
>= 3.7e-23) and pass as they are.
"""
import numpy as np
import pytest
import torch

import kl_sweep_cases as kc

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
GRAD_KEYS = ("dlog_sigma2", "dwr", "dwi")
TAIL_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1027)
WRAP_N = 2048 * 256 * 4 + 4 * 3 + 3          # the grid-stride loop wraps above 2048 blocks x 256 threads x 4
SENTINEL = -7777.25


@pytest.fixture(scope="module")
def ops():
    from cplxmodule_amd import ops
    return ops


_REF = {}


def _ref(kind, name, g=None):
    """float64 reference + bounds of one (kind, family, upstream gradient), computed once"""
    key = (kind, name, None if g is None else float(g))
    if key not in _REF:
        d = kc.family(name, kc.is_real(kind))
        r = kc.reference(kind, d, g)
        _REF[key] = (r, kc.bounds(r, d["g"] if g is None else np.full(d["g"].shape, g)))
    return _REF[key]


def _dev(d, kind):
    from gpu_util import T
    return T(np.array(d["wr"])), (None if kc.is_real(kind) else T(np.array(d["wi"]))), T(np.array(d["ls2"]))


def _ratio(got, ref, bound, what):
    """worst error / bound; the kernel's output must be finite wherever the float64 reference is finite and in range"""
    got = got.detach().double().cpu().numpy()
    assert np.isfinite(ref).all(), what                      # (kl_sweep_cases.self_check: nothing to mask out)
    inrange = np.abs(ref) < FLT_MAX
    bad = inrange & ~np.isfinite(got)
    assert not bad.any(), (what, "non-finite output at", np.flatnonzero(bad)[:8].tolist())
    err = np.abs(got - ref)[inrange]
    b = bound[inrange]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= b, np.where(b > 0, err / b, 0.0), np.where(b > 0, err / b, np.inf))   # (bound 0: exact or inf)
    if r.size and r.max() > 1.0:
        k = np.flatnonzero(inrange)[int(r.argmax())]
        print(f"\n{what}: {int((r > 1).sum())} of {r.size} over the bound; worst at element {k}: got {got[k]!r} "
              f"ref {ref[k]!r} bound {bound[k]:.3e}")
    return float(r.max()) if r.size else 0.0


def _check_all(kind, got_val, got_grads, ref, bnd, what):
    """-> {quantity: worst ratio}; asserts every ratio <= 1"""
    worst = {}
    if got_val is not None:
        worst["value"] = _ratio(got_val, ref["value"], bnd["value"], what + " value")
    for key, got in zip(GRAD_KEYS, got_grads or ()):
        if got is not None and key in ref:
            worst[key] = _ratio(got, ref[key], bnd[key], f"{what} {key}")
    assert all(v <= 1.0 for v in worst.values()), (what, worst)
    return worst


def _total_bound(ref, bnd):
    """the block sums are double: what remains is the elements' own error and the final rounding to float32"""
    return float(bnd["value"].sum() + kc.EPS32 * abs(ref["value"].sum()))


# ---- (a) values and gradients: seven kinds x four families x three entry points --------------------------------------------
@pytest.mark.parametrize("name", kc.FAMILIES)
@pytest.mark.parametrize("kind", kc.T_KINDS)
def test_values_and_gradients(ops, kind, name):
    """kl_fwd(elementwise), kl_bwd(g_elem) and kl_fwd_bwd against the float64 reference, every element inside its bound."""
    from gpu_util import T
    d = kc.family(name, kc.is_real(kind))
    wr, wi, ls2 = _dev(d, kind)
    ref, bnd = _ref(kind, name)
    elem, tot = ops.kl_fwd(kind, wr, wi, ls2, elementwise=True)
    grads = ops.kl_bwd(kind, wr, wi, ls2, g_elem=T(np.array(d["g"])))
    w1 = _check_all(kind, elem, grads, ref, bnd, f"{kind}/{name} kl_fwd+kl_bwd(g_elem)")
    assert abs(float(tot) - ref["value"].sum()) <= _total_bound(ref, bnd), (kind, name, float(tot), ref["value"].sum())
    gs = -0.75
    ref2, bnd2 = _ref(kind, name, gs)
    tot2, *grads2 = ops.kl_fwd_bwd(kind, wr, wi, ls2, gscale=gs)
    w2 = _check_all(kind, None, grads2, ref2, bnd2, f"{kind}/{name} kl_fwd_bwd")
    assert abs(float(tot2) - ref["value"].sum()) <= _total_bound(ref, bnd), (kind, name, float(tot2))
    dw = max(max(w.get("dwr", 0), w.get("dwi", 0)) for w in (w1, w2))
    print(f"\nworst error/bound {kind:>18} {name:>7}: value {w1['value']:.3f}  d_ls2 "
          f"{max(w1['dlog_sigma2'], w2['dlog_sigma2']):.3f}  d_w {dw:.3f}")


def test_edge_family_elements_named(ops):
    """The overflowing-x elements one by one (cplx_vd, packed path): t > 88.7 makes x = |w|^2 exp(-ls2) infinite in
    float32 (and for |w| = 30 already exp(-ls2) alone); the penalty gamma + t is finite and must come out so."""
    d, names = kc.family("edge"), kc.edge_names()
    wr, wi, ls2 = _dev(d, "cplx_vd")
    elem, _ = ops.kl_fwd("cplx_vd", wr, wi, ls2, elementwise=True)
    ref, bnd = _ref("cplx_vd", "edge")
    got = elem.double().cpu().numpy()
    seen = 0
    for k, nm in enumerate(names):
        if nm.startswith("t="):
            seen += 1
            assert np.isfinite(got[k]) and abs(got[k] - ref["value"][k]) <= bnd["value"][k], (nm, got[k], ref["value"][k])
    assert seen == 12


# ---- (b) the two cplx_vd paths agree; every element is summed once --------------------------------------------------------
def test_cplx_vd_paths_agree(ops):
    from gpu_util import T
    base = kc.family("range")
    sl = slice(4096, 4096 + 1024)
    d = {k: base[k][sl].copy() for k in ("wr", "wi", "ls2", "g")}
    q = d["wr"].astype(np.float64) ** 2 + d["wi"].astype(np.float64) ** 2
    # healthy quads only (a handful of the range family's weights are below |w|^2 = 1e-8 themselves)
    okq = np.repeat((q.reshape(-1, 4) >= 1.1e-8).all(1), 4)
    assert okq.mean() > 0.9
    d = {k: v[okq] for k, v in d.items()}
    n = d["wr"].shape[0]
    ref = kc.reference("cplx_vd", d)
    bnd = kc.bounds(ref, d["g"])

    def run(dd):
        wr, wi, ls2 = T(dd["wr"]), T(dd["wi"]), T(dd["ls2"])
        elem, tot = ops.kl_fwd("cplx_vd", wr, wi, ls2, elementwise=True)
        return [elem] + list(ops.kl_bwd("cplx_vd", wr, wi, ls2, g_elem=T(dd["g"]))), tot

    packed, _ = run(d)
    rs = np.random.RandomState(5)
    for pos in range(4):
        dd = {k: v.copy() for k, v in d.items()}
        for j, i in enumerate(range(pos, n, 4)):
            dd["wr"][i], dd["wi"][i] = kc.tiny_weight(rs, j)
        generic, _ = run(dd)
        keep = np.ones(n, bool)
        keep[pos::4] = False
        worst = {}
        for key, a, b in zip(("value",) + GRAD_KEYS, packed, generic):
            diff = (a.double() - b.double()).abs().cpu().numpy()[keep]
            assert np.isfinite(diff).all()
            b2 = 2 * bnd[key][keep]
            assert (diff[b2 == 0] == 0).all()                       # (upstream gradient exactly 0: exactly 0 out)
            worst[key] = float((diff[b2 > 0] / b2[b2 > 0]).max())
        print(f"\npacked vs generic path, tiny weight at position {pos}: worst difference / (2 x bound) {worst}")
        assert all(v <= 1.0 for v in worst.values()), (pos, worst)
        assert any(v > 0 for v in worst.values())           # (the second run did take the other path)


def test_cplx_vd_mixed_lanes_summed_once(ops):
    d = kc.family("mixed")
    wr, wi, ls2 = _dev(d, "cplx_vd")
    ref, _ = _ref("cplx_vd", "mixed")
    elem, tot = ops.kl_fwd("cplx_vd", wr, wi, ls2, elementwise=True)
    np.testing.assert_allclose(float(tot), ref["value"].sum(), rtol=1e-6)
    # the kernel's total against ITS OWN elements: an element counted twice or never when a lane switches path
    np.testing.assert_allclose(float(tot), float(elem.double().sum()), rtol=1e-6)
    tot2 = ops.kl_fwd_bwd("cplx_vd", wr, wi, ls2)[0]
    np.testing.assert_allclose(float(tot2), float(elem.double().sum()), rtol=1e-6)
    # per quad layout as well: a miscount confined to one arrangement must not hide in the grand total
    quads = d["tiny"].reshape(-1, 4)
    code = quads @ np.array([1, 2, 4, 8])
    for c in range(16):
        sel = np.repeat(code == c, 4)
        idx = np.flatnonzero(sel)
        e2, t2 = ops.kl_fwd("cplx_vd", wr[idx], wi[idx], ls2[idx], elementwise=True)
        np.testing.assert_allclose(float(t2), float(e2.double().sum()), rtol=1e-6, err_msg=f"layout {c:04b}")
        np.testing.assert_allclose(float(t2), ref["value"][idx].sum(), rtol=1e-6, err_msg=f"layout {c:04b}")


# ---- (c) tail and grid ----------------------------------------------------------------------------------------------------
def _raw_calls(ops, kind, d, n):
    """The four entry points at the C ABI, outputs written into the first n elements of poisoned n + 8 buffers.
    -> {entry: (elem or None, total or None, [g_ls2, g_wr, g_wi])}; asserts every element written, none beyond."""
    from gpu_util import T
    from cplxmodule_amd import _lib
    call, ptr, sp = _lib.call, _lib.ptr, _lib.stream_ptr
    code = _lib.KL_KINDS[kind]
    real = kc.is_real(kind)
    wr, ls2, ge = T(d["wr"]), T(d["ls2"]), T(d["g"])
    wi = None if real else T(d["wi"])
    ws = ops._ws(wr.device)
    bufs = []

    def out():
        b = torch.full((n + 8,), SENTINEL, device=wr.device)
        bufs.append(b)
        return b[:n]

    def outs():
        return [out(), out(), None if real else out()]

    res = {}
    elem, tot = out(), torch.full((), SENTINEL, device=wr.device)
    call("cplxamd_vd_kl_fwd", ptr(wr), ptr(wi), ptr(ls2), code, ptr(elem), ptr(tot), ptr(ws), n, sp())
    res["fwd"] = (elem, tot, None)
    g = outs()
    call("cplxamd_vd_kl_bwd", ptr(wr), ptr(wi), ptr(ls2), code, ptr(ge), None, ptr(g[0]), ptr(g[1]), ptr(g[2]), n, sp())
    res["bwd_g_elem"] = (None, None, g)
    g = outs()
    gsc = torch.tensor(0.37, device=wr.device)
    call("cplxamd_vd_kl_bwd", ptr(wr), ptr(wi), ptr(ls2), code, None, ptr(gsc), ptr(g[0]), ptr(g[1]), ptr(g[2]), n, sp())
    res["bwd_g_scalar"] = (None, None, g)
    g = outs()
    tot2 = torch.full((), SENTINEL, device=wr.device)
    call("cplxamd_vd_kl_fwd_bwd", ptr(wr), ptr(wi), ptr(ls2), code, 0.37, ptr(tot2), ptr(g[0]), ptr(g[1]), ptr(g[2]),
         ptr(ws), n, sp())
    res["fwd_bwd"] = (None, tot2, g)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[n:] == SENTINEL).all()), (kind, n, "wrote past the end")
        assert bool((b[:n] != SENTINEL).all()), (kind, n, "left elements unwritten", int((b[:n] == SENTINEL).sum()))
    assert float(tot) != SENTINEL and float(tot2) != SENTINEL
    return res


@pytest.mark.parametrize("kind", kc.ALL_KINDS)
def test_tail_sizes_every_entry_point(ops, kind):
    base = kc.family("range", kc.is_real(kind))
    worst = 0.0
    for n in TAIL_SIZES:
        off = 4096 + 4 * n                    # (general-phase part of the family, a different window per size)
        d = {k: np.array(base[k][off:off + n]) for k in ("wr", "wi", "ls2", "g")}
        res = _raw_calls(ops, kind, d, n)
        ref = kc.reference(kind, d)
        bnd = kc.bounds(ref, d["g"])
        g037 = float(np.float32(0.37))
        ref_s = kc.reference(kind, d, g037)
        bnd_s = kc.bounds(ref_s, np.full(n, g037))
        w = [_check_all(kind, res["fwd"][0], None, ref, bnd, f"{kind} n={n} kl_fwd"),
             _check_all(kind, None, res["bwd_g_elem"][2], ref, bnd, f"{kind} n={n} kl_bwd(g_elem)"),
             _check_all(kind, None, res["bwd_g_scalar"][2], ref_s, bnd_s, f"{kind} n={n} kl_bwd(g_scalar)"),
             _check_all(kind, None, res["fwd_bwd"][2], ref_s, bnd_s, f"{kind} n={n} kl_fwd_bwd")]
        worst = max([worst] + [v for x in w for v in x.values()])
        for tot in (res["fwd"][1], res["fwd_bwd"][1]):
            assert abs(float(tot) - ref["value"].sum()) <= _total_bound(ref, bnd), (kind, n, float(tot))
        for a, b in zip(res["bwd_g_scalar"][2], res["fwd_bwd"][2]):
            assert (a is None and b is None) or torch.equal(a, b), (kind, n)
    print(f"\nworst error/bound {kind:>18} tail sizes {TAIL_SIZES}: {worst:.3f}")


@pytest.mark.parametrize("kind", ("cplx_vd", "real_vd"))
def test_grid_stride_wrap(ops, kind):
    """More vector indices than the 2048-block grid has threads: the loop's second trip, then three more quads and a
    three-element tail."""
    from gpu_util import T
    base = kc.family("range", kc.is_real(kind))
    idx = (np.arange(WRAP_N) + 4096) % base["wr"].shape[0]
    wr, ls2 = T(base["wr"][idx]), T(base["ls2"][idx])
    wi = None if kc.is_real(kind) else T(base["wi"][idx])
    ref0, bnd0 = _ref(kind, "range", 1.0)
    ref = {k: v[idx] for k, v in ref0.items()}
    bnd = {k: v[idx] for k, v in bnd0.items()}
    elem, tot = ops.kl_fwd(kind, wr, wi, ls2, elementwise=True)
    tot2, *grads = ops.kl_fwd_bwd(kind, wr, wi, ls2)
    w = _check_all(kind, elem, grads, ref, bnd, f"{kind} n={WRAP_N}")
    for t in (tot, tot2):
        assert abs(float(t) - ref["value"].sum()) <= _total_bound(ref, bnd), (kind, float(t), ref["value"].sum())
        np.testing.assert_allclose(float(t), float(elem.double().sum()), rtol=1e-6)
    print(f"\nworst error/bound {kind:>18} grid wrap n={WRAP_N}: {w}")


# ---- (d) prep_kl: the fused pass the bf16 layers train on ------------------------------------------------------------------
def _prep_inputs(n, real):
    base = kc.family("range", real)
    idx = (np.arange(n) + 2048) % 16384
    d = {k: base[k][idx].copy() for k in ("wr", "wi", "ls2")}
    # bf16 rounding: subnormals, signed zeros, ties (1 + 2^-8 -> 1 and 1 + 3 * 2^-8 -> 1 + 2^-6: to even), carries
    special = np.array([1e-39, -0.0, 1.00390625, -1.01171875, 0.0, -1e-39, 1.9990234375, 255.5, 9.2e-41,
                        -1.00390625, 1.0039063692092896, 1.0039061307907104], np.float32)
    mid = kc.bf16_midpoint_ls2()
    if n == 4:
        d["wr"][:], d["wi"][:], d["ls2"][:] = special[:4], special[4:8], mid[:4]
    else:
        d["wr"][:12], d["wi"][4:16] = special, special
        m = min(mid.shape[0], n - 16)
        d["ls2"][16:16 + m] = mid[:m]
    return d


@pytest.mark.parametrize("n", (4, 1024, 4 * 1031))
@pytest.mark.parametrize("with_kl", (False, True))
@pytest.mark.parametrize("kind", ("cplx_vd", "cplx_ard", "real_vd", "real_ard"))
def test_prep_kl(ops, kind, with_kl, n):
    d = _prep_inputs(n, kc.is_real(kind))
    wr, wi, ls2 = _dev(d, kind)
    wb, wib, sb, tot, grads = ops.prep_kl(kind, wr, wi, ls2, with_kl)
    bf = torch.bfloat16
    assert wb.dtype == bf and torch.equal(wb.view(torch.int16), wr.to(bf).view(torch.int16))     # (bits: -0.0 too)
    if wi is None:
        assert wib is None
    else:
        assert torch.equal(wib.view(torch.int16), wi.to(bf).view(torch.int16))
    # S = bf16(exp(ls2)): half a bf16 ulp of the result for the rounding + 4 eps32 for the float32 exp before it
    s = sb.double().cpu().numpy()
    true = np.exp(d["ls2"].astype(np.float64))
    assert (s > 0).all() and np.isfinite(s).all()
    ulp = 2.0 ** (np.floor(np.log2(s)) - 7)
    err = np.abs(s - true)
    bound = 0.5 * ulp + 4 * kc.EPS32 * true
    assert (err <= bound).all(), (kind, n, float((err / bound).max()))
    if with_kl:
        tot2, *g2 = ops.kl_fwd_bwd(kind, wr, wi, ls2, gscale=1.0)
        assert torch.equal(tot, tot2)
        for a, b in zip(grads, g2):
            assert (a is None and b is None) or torch.equal(a, b)
    else:
        assert tot is None and grads is None


@pytest.mark.parametrize("with_kl", (False, True))
def test_prep_kl_rejects_odd_sizes(ops, with_kl):
    """n % 4 != 0 is CPLXAMD_ESHAPE before any launch; it reaches Python as the wrappers' usual exception."""
    from cplxmodule_amd import _lib
    z = torch.zeros(6, device="cuda")
    with pytest.raises(_lib.CplxAmdError, match="unsupported shape"):
        ops.prep_kl("cplx_vd", z, z.clone(), z.clone(), with_kl)


# ---- (e) Ei ----------------------------------------------------------------------------------------------------------------
def _neighbours(c, k=8):
    out, lo, hi = [np.float32(c)], np.float32(c), np.float32(c)
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.array(out, np.float32)


def _expi_inputs():
    x = np.concatenate([-np.logspace(-30, 2.9, 330), np.logspace(-30, np.log10(88.0), 320)]).astype(np.float32)
    x = np.concatenate([x] + [_neighbours(c) for c in (1.0, -1.0, 40.0, -40.0, -745.0)])
    return np.concatenate([x, np.array([0.0, -0.0], np.float32)])


def test_expi_forward_and_backward(ops):
    from scipy.special import expi as scipy_expi
    from gpu_util import T, N
    x = _expi_inputs()
    rs = np.random.RandomState(9)
    g = (rs.uniform(0.5, 2.0, x.shape[0]) * np.where(rs.uniform(size=x.shape[0]) < 0.5, -1, 1)).astype(np.float32)
    tx = T(x).requires_grad_(True)
    y = ops.ExpiFn.apply(tx)
    with np.errstate(divide="ignore", under="ignore"):
        ref = scipy_expi(x.astype(np.float64)).astype(np.float32)       # float64, rounded once
    got = N(y)
    assert np.isneginf(ref[-2:]).all() and np.isneginf(got[-2:]).all()    # Ei(0) = Ei(-0.0) = -inf
    fin = np.isfinite(ref)
    assert fin.sum() == x.shape[0] - 2 and np.isfinite(got[fin]).all()
    # (1e-37: a result below FLT_MIN keeps fewer than 24 bits; no relative statement holds for it)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-6, atol=1e-37)
    y.backward(T(g))
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        dref = g * np.exp(x) / x                                         # the reference's float32 chain
    dgot = N(tx.grad)
    assert not np.isnan(dref).any()
    np.testing.assert_array_equal(np.isinf(dgot), np.isinf(dref))
    np.testing.assert_array_equal(np.sign(dgot[np.isinf(dref)]), np.sign(dref[np.isinf(dref)]))
    f = np.isfinite(dref)
    np.testing.assert_allclose(dgot[f], dref[f], rtol=1e-5, atol=1e-37)


def test_expi_backward_overflow_matches_float32_chain(ops):
    """Above x ~ 88.7 the reference's float32 exp(x) is inf and so is its gradient; parity, not a finite value."""
    from gpu_util import T, N
    x = np.array([88.0, 88.7, 88.73, 89.0, 100.0], np.float32)
    tx = T(x).requires_grad_(True)
    ops.ExpiFn.apply(tx).sum().backward()
    with np.errstate(over="ignore"):
        dref = np.exp(x) / x
    np.testing.assert_array_equal(np.isinf(N(tx.grad)), np.isinf(dref))
    assert np.isinf(dref[-2:]).all() and np.isfinite(dref[0])
