"""The cancellation-free float64 KL reference (oracle.cplx_oracle.penalty_exact) against 50-digit arithmetic, against the
pinned literal oracle where that one is accurate, and the self-checks of the case table tests/kl_sweep_cases.py."""
import numpy as np
import pytest

from oracle import cplx_oracle as orc

import kl_sweep_cases as kc


def _mp_penalty(mp, wr, wi, ls2):
    """euler + t - Ei(-e^t) with t = 2 ln(|w| + 1e-12) - ls2, everything at 50 digits on the float64 inputs"""
    w = mp.sqrt(mp.mpf(float(wr)) ** 2 + mp.mpf(float(wi)) ** 2)
    t = 2 * mp.log(w + mp.mpf("1e-12")) - mp.mpf(float(ls2))
    return mp.euler + t - mp.ei(-mp.exp(t)), t


def test_penalty_exact_vs_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    xs = np.concatenate([np.logspace(-30, 4, 137), [1 / 64, 1 / 4, 1.0, 104.0, np.exp(20.0)]])
    xs = np.concatenate([xs, xs[-5:] * (1 - 1e-9), xs[-5:] * (1 + 1e-9)])
    # three operand magnitudes per x; ls2 follows from the target t
    rows = [(a * 0.6, -a * 0.8, 2 * np.log(a + 1e-12) - np.log(x)) for x in xs for a in (1e-2, 1.0, 30.0)]
    wr, wi, ls2 = (np.array(c, np.float64) for c in zip(*rows))
    got = orc.penalty_exact("cplx_vd", ls2, wr, wi)
    got_sf = orc.penalty_exact("cplx_vd_scalefree", ls2, wr, wi)
    worst = 0.0
    for k in range(len(rows)):
        ref, t = _mp_penalty(mp, wr[k], wi[k], ls2[k])
        rel = abs((mp.mpf(float(got[k])) - ref) / ref)
        worst = max(worst, float(rel))
        assert rel < 1e-13, (xs[k // 3], float(rel))
        # extensions/complex.py:43-46: log|w| - ls2 - Ei(-e^t) / 2
        ref_sf = (t + mp.mpf(float(ls2[k]))) / 2 - mp.mpf(float(ls2[k])) - mp.ei(-mp.exp(t)) / 2
        scale = abs(ref_sf) + abs(t) / 2 + abs(mp.mpf(float(ls2[k]))) / 2      # its O(|t|) terms do cancel
        assert abs(mp.mpf(float(got_sf[k])) - ref_sf) < 1e-13 * scale
    print(f"penalty_exact vs mpmath: worst relative error {worst:.2e} over {len(rows)} points")


@pytest.mark.parametrize("kind", orc.KINDS + orc.EXT_KINDS)
def test_penalty_exact_vs_pinned_oracle_on_goldens(golden, kind):
    """Ties the new reference to the one test_oracle_golden.py pins, on inputs where the literal expression is accurate
    (x >= 1e-5 there: eps64 |t| / x < 1e-10)."""
    if kind in orc.EXT_KINDS:
        g = golden("extras")
        k = f"f32_ext_{kind}_"
        wr, wi, ls2 = g[k + "wr"], g[k + "wi"], g[k + "ls2"]
    else:
        g = golden("penalty")
        wr, ls2 = g["f32_wr"], g["f32_ls2"]
        wi = g["f32_wi"] if kind.startswith("cplx") else None
    f = np.float64
    wr, ls2, wi = wr.astype(f), ls2.astype(f), None if wi is None else wi.astype(f)
    old = orc.penalty(kind, ls2, wr, wi)
    new = orc.penalty_exact(kind, ls2, wr, wi)
    fin = np.isfinite(old)
    assert fin.mean() > 0.99
    x = np.exp(-orc.log_alpha(ls2, wr, wi))
    ok = fin & (x >= 1e-5) if kind == "cplx_vd" else fin      # (the scale-free value is O(|t|): no cancellation to speak of)
    assert ok.sum() > 0.5 * ok.size
    np.testing.assert_allclose(new[ok], old[ok], rtol=1e-10, atol=0)
    # the rest: within the literal expression's own cancellation error eps64 (|gamma| + |t| + |Ei|) ~ 4 eps64 |t|
    t = np.abs(orc.log_alpha(ls2, wr, wi))
    assert (np.abs(new - old)[fin] <= 1e-10 * np.abs(old[fin]) + 8 * np.finfo(f).eps * (1 + t[fin])).all()


def test_penalty_exact_where_the_literal_form_fails():
    """x = 1e-20: the literal expression returns rounding noise, the series returns x (1 - x/4 + ...)."""
    ls2 = np.array([np.log(1e20)])
    wr = np.array([1.0])
    exact = orc.penalty_exact("cplx_vd", ls2, wr, np.zeros(1))
    x = np.exp(2 * np.log(1 + 1e-12) - ls2)
    np.testing.assert_allclose(exact, x, rtol=1e-15)
    assert abs(orc.penalty("cplx_vd", ls2, wr, np.zeros(1))[0] - x[0]) > 0.5 * x[0]
    # the overflow end: E1 underflows, gamma + t remains
    np.testing.assert_allclose(orc.penalty_exact("cplx_vd", np.array([-800.0]), wr, np.zeros(1)),
                               orc.EULER_GAMMA + 800.0 + 2 * np.log(1 + 1e-12), rtol=1e-15)


def test_case_table_self_checks():
    assert kc.self_check()
    for real in (False, True):
        for name in kc.FAMILIES:
            d = kc.family(name, real)
            n = d["wr"].shape[0]
            assert n % 4 == 0 and all(d[k].shape == (n,) and d[k].dtype == np.float32 for k in ("wr", "wi", "ls2", "g"))
            g = d["g"]
            assert (g > 0).any() and (g < 0).any() and (g == 0).any()
    r = kc.family("range")
    assert r["wr"].shape[0] == 16384
    th = np.hypot(r["wr"].astype(np.float64), r["wi"].astype(np.float64))
    assert th.min() >= 0.99e-4 and th.max() <= 30.01 and r["ls2"].min() >= -30 and r["ls2"].max() <= 12
    assert ((r["wi"] == 0) & (r["wr"] != 0)).sum() >= 1024 and ((r["wr"] == 0) & (r["wi"] != 0)).sum() >= 1024
    # every switch-point: points on both sides, at four operand magnitudes
    hits = kc.switch_hits()
    print({f"{k[0]} {'first' if k[1] else 'second'} side": v for k, v in sorted(hits.items())})
    s = kc.family("switch")
    th = np.hypot(s["wr"].astype(np.float64), s["wi"].astype(np.float64))
    for m in kc.MAGNITUDES:
        assert ((th > 0.85 * m) & (th < 1.15 * m)).sum() >= 64, m
    # the edge family: what the issue lists is there
    e, names = kc.family("edge"), kc.edge_names()
    t = 2 * np.log(np.hypot(e["wr"].astype(np.float64), e["wi"].astype(np.float64)) + 1e-12) - e["ls2"]
    for want in (60, 80, 88, 89, 100, 120):
        assert (np.abs(t - want) < 1e-4).sum() >= 2, want
    assert (e["ls2"] == 80).sum() >= 4 and any("1e-36" in n for n in names)
    assert np.signbit(e["wr"][e["wr"] == 0]).any() and np.signbit(e["wi"][e["wi"] == 0]).any()


def test_bf16_midpoint_search_finds_points():
    mid = kc.bf16_midpoint_ls2()
    assert mid.dtype == np.float32 and mid.shape[0] >= 256 and mid.min() > -1 and mid.max() < 1
    e = np.exp(mid.astype(np.float64)).astype(np.float32).view(np.int32)
    assert (np.abs((e & 0xFFFF) - 0x8000) <= 2).all()
