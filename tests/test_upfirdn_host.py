"""cplx.upfirdn / cplx.resample_poly without a GPU: the plan (cplxamd_upfirdn_plan is a pure function), the tile
geometry it lays out -- emulated in numpy from the plan's numbers alone and compared with the naive oracle --, the oracle
and the filter design against the golden scipy outputs, every gradient identity by an inner-product test on the oracle,
every argument error with its exception type, the descriptor and NULL-pointer rejections of the launchers (they return
before any launch), and the headroom of the integer cases of test_gpu_upfirdn.py."""
import ctypes

import numpy as np
import pytest
import torch

import upfirdn_cases as uc

from cplxmodule_amd import Cplx, _lib, cplx
from cplxmodule_amd import upfirdn as hostup
from cplxmodule_amd._lib import CplxAmdError

DT = {"f32": torch.float32, "f64": torch.float64}


def _ints(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, n) + 1j * rng.integers(-4, 5, n)


# ---- the plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(uc.PLAN_TABLE), ids=lambda c: "-".join(map(str, c)))
def test_plan_table(case):
    n, k, up, down, dt, xc, hc = case
    length = uc.length_upfirdn(n, k, up, down)
    p = hostup.plan(n, k, length, up, down, 0, 4, 1, DT[dt], False, xc, hc)
    assert p["path"] == "fused"
    assert (p["T"], p["tiles"], p["vectors_per_workgroup"], p["span"], p["jseg"], p["segs"]) == uc.PLAN_TABLE[case]
    jfull = -(-k // up)
    assert p["phases"] == min(up, k) and p["segs"] == -(-jfull // p["jseg"]) and p["tiles"] == -(-length // p["T"])
    assert p["span"] == ((p["T"] - 1) * down + up - 1) // up + p["jseg"]
    # two workgroups fit the 160 KiB of a CU
    assert p["lds_bytes"] <= 76 * 1024 and p["wgrad_lds_bytes"] <= 76 * 1024
    word = 8 if dt == "f64" else 4
    slice_words = (2 if xc else 1) * (uc.pad(p["span"]) + 1) + (2 if hc else 1) * (uc.pad(p["phases"] * p["jseg"]) + 1)
    assert p["lds_bytes"] == p["vectors_per_workgroup"] * slice_words * word
    assert p["grid"] == -(-4 * p["tiles"] // p["vectors_per_workgroup"])
    assert p["threads"] == min(256, -(-p["T"] * p["vectors_per_workgroup"] // 64) * 64)


def test_plan_paths_chunks_and_rejections():
    assert hostup.plan(100, 4096, 4195, 1, 1)["path"] == "fused"
    assert hostup.plan(100, 4097, 4196, 1, 1)["path"] == "composed"
    # the default resample_poly filter stays fused up to max(up, down) = 204
    assert hostup.plan(1000, 20 * 204 + 1, 1000, 204, 1)["path"] == "fused"
    assert hostup.plan(1000, 20 * 205 + 1, 1000, 205, 1)["path"] == "composed"
    # up > K: only K phases carry a tap
    p = hostup.plan(10, 3, 500, 50, 1)
    assert (p["phases"], p["jseg"], p["segs"]) == (3, 1, 1)
    # the weight gradient of the benchmark's 160/147 conversion with one shared filter: four blocks of taps, 768 / 4 = 192 chunks asked, 191 of 94 pairs needed
    p = hostup.plan(65536, 3201, 71332, 160, 147, 1600, 256, 1)
    assert (p["wgrad_Tn"], p["wgrad_tiles"], p["wgrad_kb"], p["wgrad_kblocks"]) == (1024, 70, 1024, 4)
    assert p["wgrad_per_chunk"] == -(-256 * 70 // 192) == 94 and p["wgrad_chunks"] == -(-256 * 70 // 94) == 191
    assert p["wgrad_ws_bytes"] == 191 * 3201 * 8 + (-(191 * 3201 * 8) % 256)
    assert p["wgrad_span"] == (1023 * 147 + 1023) // 160 + 2
    # a filter per row: one chunk each
    p = hostup.plan(4096, 33, 2048, 1, 2, 0, 1024, 1024)
    assert p["wgrad_chunks"] == 1 and p["wgrad_per_chunk"] == p["wgrad_tiles"]
    out = (ctypes.c_int64 * len(_lib.UPFIRDN_PLAN_FIELDS))()
    lib = _lib.load()
    ok = [100, 5, 104, 3, 2, 0, 1, 1, _lib.F32, 0, 1, 1, out]
    assert lib.cplxamd_upfirdn_plan(*ok) == 0
    for at, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (6, -1), (7, -1), (8, 99), (9, 2), (10, 2), (11, -1), (12, None)):
        args = list(ok)
        args[at] = bad
        assert lib.cplxamd_upfirdn_plan(*args) == -1, at
    for at, bad in ((3, (1 << 30) + 1), (4, (1 << 30) + 1), (0, (1 << 40) + 1), (5, (1 << 48) + 1), (5, -(1 << 48) - 1)):
        args = list(ok)
        args[at] = bad
        assert lib.cplxamd_upfirdn_plan(*args) == -3, at
    with pytest.raises(CplxAmdError, match="2\\^30"):
        hostup.plan(100, 5, 104, 1 << 31, 1)


# ---- the geometry, from the plan's numbers alone ---------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.geometry_cases(), ids=lambda c: "x".join(map(str, c)))
def test_tile_emulation_equals_the_oracle(case):
    n, k, up, down = case
    x, h = _ints(n, 100 * n + k), _ints(k, 7 * k + up)
    for off, length in ((0, uc.length_upfirdn(n, k, up, down)), ((k - 1) // 2, -(-n * up // down)), (-3, 7)):
        for conj in (False, True):
            p = hostup.plan(n, k, length, up, down, off, conj=conj)
            got = uc.emulate_p1(x, h, up, down, off, length, conj, p)
            assert np.abs(got - uc.p1(x, h, up, down, off, length, conj)).max() < 1e-9, (off, length, conj, p)
    for off in (0, 5, -2):
        c = _ints(uc.length_upfirdn(n, k, up, down), 3)
        p = hostup.plan(n, k, len(c), up, down, off)
        assert np.abs(uc.emulate_p2(x, c, up, down, off, k, p) - uc.p2(x, c, up, down, off, k)).max() < 1e-9, (off, p)


# the tile seam: N = T down / up -+ 1 at T = 1024 outputs; segments (float64, a long filter and a decimation); packing
SEAMS = [(n, k, up, down, "f32") for up, down, k in ((1, 2, 5), (3, 2, 8), (2, 3, 7), (7, 5, 16), (160, 147, 325))
         for n in (1024 * down // up - 1, 1024 * down // up, 1024 * down // up + 1)]
SEAMS += [(4100, 1281, 1, 64, "f64"), (300, 4096, 1, 1, "f64"), (200, 4096, 3, 2, "f64")]


@pytest.mark.parametrize("case", SEAMS, ids=lambda c: "x".join(map(str, c)))
def test_tile_seams_and_segments(case):
    n, k, up, down, dt = case
    x, h = _ints(n, n + k), _ints(k, k + up)
    length = uc.length_upfirdn(n, k, up, down)
    for conj in (False, True):
        p = hostup.plan(n, k, length, up, down, 0, dtype=DT[dt], conj=conj)
        if dt == "f64":
            assert p["segs"] > 1 and p["T"] <= 64
        else:
            assert p["T"] == min(1024, length) and p["tiles"] == -(-length // 1024) and 1022 <= length <= 1028
        got = uc.emulate_p1(x, h, up, down, 0, length, conj, p)
        assert np.abs(got - uc.p1(x, h, up, down, 0, length, conj)).max() < 1e-9, (conj, p)
    c = _ints(length, 5)
    p = hostup.plan(n, k, length, up, down, 0, dtype=DT[dt])
    assert np.abs(uc.emulate_p2(x, c, up, down, 0, k, p) - uc.p2(x, c, up, down, 0, k)).max() < 1e-9, p


# ---- the oracle and the design against scipy's recorded outputs ---------------------------------------------------------
def test_oracle_equals_golden_scipy():
    g = uc.golden()
    for i, (n, k, up, down) in enumerate(uc.GOLDEN_UPFIRDN):
        x, h = uc.golden_input(n, 1000 + i), uc.golden_input(k, 2000 + i)
        ref = g[f"upfirdn_{n}_{k}_{up}_{down}"]
        assert ref.shape == (uc.length_upfirdn(n, k, up, down),)
        assert np.abs(uc.p1(x, h, up, down, 0, len(ref)) - ref).max() <= 1e-12 * np.abs(ref).max()
        ref = g[f"upfirdn_real_{n}_{k}_{up}_{down}"]
        got = uc.p1(x.real, h.real, up, down, 0, len(ref))
        assert not got.imag.any() and np.abs(got.real - ref).max() <= 1e-12 * np.abs(ref).max()
    for i, (n, up, down) in enumerate(uc.GOLDEN_RESAMPLE):
        x = uc.golden_input(n, 3000 + i)
        gcd = int(np.gcd(up, down))
        u, d = up // gcd, down // gcd
        ref = g[f"resample_{n}_{up}_{down}"]
        assert ref.shape == (-(-n * u // d),)
        # the whole resampling is ONE P1 with off = half: nothing padded, nothing sliced
        got = uc.p1(x, uc.design(u, d), u, d, 10 * max(u, d), len(ref))
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (n, up, down)
        got = uc.p1(x.real, uc.design(u, d), u, d, 10 * max(u, d), len(ref))
        assert np.abs(got.real - g[f"resample_real_{n}_{up}_{down}"]).max() <= 1e-12 * np.abs(ref).max()
    for i, (n, up, down, k) in enumerate(uc.GOLDEN_WINDOW):
        x, w = uc.golden_input(n, 4000 + i), uc.golden_input(k, 5000 + i, cplx=False)
        ref = g[f"window_{n}_{up}_{down}_{k}"]
        got = uc.p1(x, w * up, up, down, (k - 1) // 2, -(-n * up // down))
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("rates", uc.GOLDEN_FIRWIN, ids=lambda c: f"{c[0]}_{c[1]}")
def test_design_equals_golden_firwin(rates):
    up, down = rates
    ref = uc.golden()[f"firwin_{up}_{down}"]
    for name, h in (("numpy", uc.design(up, down)), ("package", hostup.design(up, down).numpy())):
        assert h.shape == ref.shape == (20 * max(up, down) + 1,)
        assert np.abs(h - ref).max() <= 1e-12 * np.abs(ref).max(), name
        assert abs(h.sum() - up) <= 1e-12 * up
    assert hostup.design(up, down) is hostup.design(up, down)                  # cached
    assert hostup.design(up, down, dtype=torch.float32).dtype == torch.float32


# ---- every gradient identity, by inner products on the oracle -----------------------------------------------------------
def _ip(u, v):
    return float(np.real(np.sum(np.conj(u) * v)))


@pytest.mark.parametrize("rates", [(3, 2, 4), (2, 3, -1), (7, 5, 0), (4, 6, 3), (1, 1, 2), (1, 2, 0), (2, 1, 1), (160, 147, 40)],
                         ids=lambda c: "_".join(map(str, c)))
def test_gradient_identities(rates):
    """<g, F(d)> == <grad, d> for every operand of every primitive, F linear or antilinear over the reals in it"""
    up, down, off = rates
    n, k, length = 13, 9 if up < 100 else 330, 11
    x, h, g = _ints(n, 1), _ints(k, 2), _ints(length, 3)
    dx, dh = _ints(n, 4), _ints(k, 5)
    for conj in (False, True):
        gx = uc.p1(g, h, down, up, -off, n, not conj)
        assert abs(_ip(g, uc.p1(dx, h, up, down, off, length, conj)) - _ip(gx, dx)) < 1e-9, ("dx", conj)
        gh = uc.p2(g, x, down, up, -off, k) if conj else uc.p2(x, g, up, down, off, k)
        assert abs(_ip(g, uc.p1(x, dh, up, down, off, length, conj)) - _ip(gh, dh)) < 1e-9, ("dh", conj)
    a, c, gk = _ints(n, 6), _ints(length, 7), _ints(k, 8)
    da, dc = _ints(n, 9), _ints(length, 10)
    ga = uc.p1(c, gk, down, up, -off, n, True)
    gc = uc.p1(a, gk, up, down, off, length, False)
    assert abs(_ip(gk, uc.p2(da, c, up, down, off, k)) - _ip(ga, da)) < 1e-9
    assert abs(_ip(gk, uc.p2(a, dc, up, down, off, k)) - _ip(gc, dc)) < 1e-9


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors():
    x, h = torch.zeros(2, 16), torch.zeros(3)
    for up, down in ((0, 1), (1, 0), (-2, 1), (1.5, 1)):
        with pytest.raises(ValueError, match="up and down"):
            cplx.upfirdn(h, x, up, down)
        with pytest.raises(ValueError, match="up and down"):
            cplx.resample_poly(x, up, down)
    with pytest.raises(ValueError, match="0-d"):
        cplx.upfirdn(torch.tensor(1.0), x)
    with pytest.raises(ValueError, match="0-d"):
        cplx.resample_poly(torch.tensor(1.0), 3, 2)
    with pytest.raises(ValueError, match="empty"):
        cplx.upfirdn(h, torch.zeros(2, 0))
    with pytest.raises(ValueError, match="empty"):
        cplx.upfirdn(torch.zeros(0), x)
    for window in ("hamming", ("hann", 1.0), ("kaiser",), 5.0):
        with pytest.raises(ValueError, match="window"):
            cplx.resample_poly(x, 3, 2, window)
    with pytest.raises(ValueError, match="1-d"):
        cplx.resample_poly(x, 3, 2, torch.zeros(2, 5))
    with pytest.raises(RuntimeError):
        cplx.upfirdn(torch.zeros(4, 3), torch.zeros(2, 3, 16))
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.upfirdn(h.double(), x)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.upfirdn(h, Cplx(x, x.double()))
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.upfirdn(h.half(), x.half())
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.resample_poly(x.half(), 3, 2)
    with pytest.raises(CplxAmdError, match="complex"):
        cplx.upfirdn(h, torch.zeros(4, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="complex"):
        cplx.resample_poly(torch.zeros(4, dtype=torch.complex64), 3, 2)
    with pytest.raises(CplxAmdError, match="no CPU path"):             # there is no host path
        cplx.upfirdn(h, x, 3, 2)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.resample_poly(x, 3, 2)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.resample_poly(Cplx(x, x), 2, 3, torch.ones(7))
    # equal rates after the gcd: the input comes back, whatever the device
    y = cplx.resample_poly(x, 6, 6)
    assert torch.equal(y, x) and y is not x


# ---- the launchers reject before they launch -----------------------------------------------------------------------------
def _desc(**kw):
    d = _lib.UpfirdnDesc(a_len=100, k=5, c_len=152, up=3, down=2, off=0, a_es=1, b_es=1, runs=1, conj=0)
    d.size[0], d.a_stride[0], d.b_stride[0], d.y_stride[0] = 3, 100, 0, 152
    for key, v in kw.items():
        setattr(d, key, v)
    return d


@pytest.mark.parametrize("name", ["cplxamd_upfirdn", "cplxamd_upfirdn_wgrad"])
def test_launchers_reject_bad_arguments_without_a_launch(name):
    fn = getattr(_lib.load(), name)
    wgrad = name.endswith("wgrad")
    assert ctypes.sizeof(_lib.UpfirdnDesc) == 168
    p = ctypes.c_void_p(4096)                             # never dereferenced: every call below returns before a launch
    d = _desc()
    if wgrad:
        d.y_stride[0] = 0
    tail = [p, 1 << 30, None] if wgrad else [None]        # the workspace, its size, the stream
    ok = [p, None, p, None, p, None, ctypes.byref(d), _lib.F32] + tail
    for null in (0, 2, 4, 6) + ((8,) if wgrad else ()):   # a_r, b_r, y_r, the descriptor, the workspace
        args = list(ok)
        args[null] = None
        assert fn(*args) == -1, null
    assert fn(*(ok[:7] + [99] + ok[8:])) == -1            # dtype
    if wgrad:
        assert fn(*(ok[:9] + [64] + ok[10:])) == -4       # a workspace that is too small
    bad = [dict(a_len=0), dict(k=0), dict(c_len=-1), dict(up=0), dict(down=-1), dict(a_es=-1), dict(b_es=-1), dict(runs=4),
           dict(k=4097), dict(conj=1) if wgrad else dict(conj=2)]
    for kw in bad:
        d2 = _desc(**kw)
        args = list(ok)
        args[6] = ctypes.byref(d2)
        assert fn(*args) == -1, kw
    d2 = _desc(up=(1 << 30) + 1)
    args = list(ok)
    args[6] = ctypes.byref(d2)
    assert fn(*args) == -3
    d2 = _desc()
    d2.size[0] = -3
    args[6] = ctypes.byref(d2)
    assert fn(*args) == -1
    d2 = _desc()
    d2.size[0] = 0                                        # no rows: nothing to do
    args[6] = ctypes.byref(d2)
    assert fn(*args) == 0


# ---- the integer cases are exact in float32 --------------------------------------------------------------------------
def test_integer_cases_have_headroom():
    cases = uc.exact_cases()
    assert {c[3:] for c in cases} == set(uc.RATES)        # every rate pair reaches the tile seam
    for rows, n, k, up, down in cases + uc.PACKED:
        xr, xi, hr, hi = uc.exact_case(rows, n, k)
        assert float(torch.stack([t.abs().max() for t in (xr, xi, hr, hi)]).max()) <= 4
        length = uc.length_upfirdn(n, k, up, down)
        # an output sums at most ceil(K / up) products; a tap of the filter's gradient at most `length` per row, an entry
        # of the signal's gradient at most ceil(K / down) (the rates swap)
        terms = max(-(-k // up), rows * length, -(-k // down))
        assert uc.partial_sum_bound(terms) < 2 ** 24
    for rows, n, k, up, down in uc.PACKED:
        p = hostup.plan(n, k, uc.length_upfirdn(n, k, up, down), up, down, 0, rows, 1)
        assert p["T"] == 100 and p["tiles"] == 1 and p["vectors_per_workgroup"] == min(10, rows)
