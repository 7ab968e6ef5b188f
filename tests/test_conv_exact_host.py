"""Host-side checks of the bit-exact convolution cases (conv_exact_cases.py): every case selects the route it was written
for, stays exactly representable, and -- where its sums are large enough -- actually exercises the bf16 rounding."""
import numpy as np
import pytest
import torch

import conv_exact_cases as K
from conv_exact_cases import CASES

TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


# ---- the dispatcher of cplxmodule_amd/conv.py, re-read as a pure function of the geometry -------------------------------------
# Only the predicates come from conv.py; the order they are asked in, and the shape limits the entry points document
# (CPLXAMD_ESHAPE -> the next kernel), are written out here so that a case's `fwd` / `dgrad` / `wgrad` is checked against
# what the dispatcher will do, not copied from it.
def _patch(c, C, N):
    """cplxamd_conv2d_cl2: 3 x 3, dilation 1, C % 32 == 0, N % 64 == 0 (else the row kernel cplxamd_conv2d_cl)."""
    return c["patch"] and c["k"] == (3, 3) and c["dilation"] == (1, 1) and C % 32 == 0 and N % 64 == 0


def _cl_entry(c, dgrad):
    C, N = (c["Co"], c["Ci"]) if dgrad else (c["Ci"], c["Co"])
    return "cl2" if _patch(c, C, N) else "cl"


def _planar(c, geom, cplx):
    from cplxmodule_amd import conv
    dt = TORCH_DTYPE[c["dtype"]]
    bf16 = dt == torch.bfloat16
    kh, kw = c["k"]
    g = c["groups"]
    if conv._rows_fwd_ok(geom, dt):
        fwd = "rows" if bf16 else "rows32"
    elif bf16 and ((c["Ci"] // g) * kh * kw) % 32 == 0:
        fwd = "g16f"
    else:
        fwd = "genf"
    if conv._rows_dgrad_ok(geom, dt):
        dgrad = "rows" if bf16 else "rows32"
    elif bf16 and c["stride"] == (1, 1) and ((c["Co"] // g) * kh * kw) % 32 == 0:
        dgrad = "g16d"
    else:
        dgrad = "gend"
    if conv._rows_wgrad_ok(geom, cplx, dt):
        wgrad = ("lin" if (kh, kw) == (1, 1) else "rowsw") if bf16 else "rowsw32"
    else:
        wgrad = "g16w" if bf16 else "genw"
    return fwd, dgrad, wgrad


def host_route(c):
    from cplxmodule_amd import conv
    with K.switches(c):
        geom = K.geom_of(c)
        api, bf16 = c["api"], c["dtype"] == "bf16"
        cl_f, cl_d, cl_w = conv._cl_ok(geom), conv._cl_ok(geom, dgrad=True), conv._cl_wgrad_ok(geom)
        if api in ("cplx", "conv1d"):
            if c["dtype"] == "f32" and conv._x2_conv_kind(geom) == "x2":
                return "x2", "x2", "x2w"
            if bf16 and cl_f and cl_w:
                return _cl_entry(c, False), (_cl_entry(c, True) if cl_d else _planar(c, geom, True)[1]), "clw"
            return _planar(c, geom, True)
        if api == "real":
            if bf16 and cl_f and cl_d and cl_w:
                return "clr", "clr", "clrw"
            return _planar(c, geom, False)
        if api == "direct":
            assert bf16 and not (cl_f and cl_w), "this layer is channels-last as a whole: test it through cplx.conv2d"
            return (_cl_entry(c, False) if cl_f else None, _cl_entry(c, True) if cl_d else None, "clw" if cl_w else None)
        if api == "cl_real":
            assert bf16
            return ("clr" if cl_f else None, "clr" if cl_d else None, "clrw" if cl_w else None)
        assert api == "transpose"
        f, d, w = _planar(c, geom, True)
        if bf16 and d == "g16d":            # the bias joins float32 sums: the shifted-row and the gather kernel store those
            d = "g16d32"
        elif bf16 and d != "rows":          # from bf16 operands, else the float32 kernels on the widened operands
            d = "rows32" if conv._rows_dgrad_ok(geom, torch.float32) else "gend"
        return d, f, w                      # forward = the convolution's data gradient, data gradient = its forward


@pytest.mark.parametrize("name", list(CASES))
def test_case_takes_the_route_it_names(name):
    c = CASES[name]
    assert all(r is None or r in K.ENTRY for r in (c["fwd"], c["dgrad"], c["wgrad"]))
    assert (c["fwd"], c["dgrad"], c["wgrad"]) == host_route(c)
    assert c["fwd"] or c["dgrad"]
    if c["api"] == "conv1d":
        assert c["H"] == 1 and c["k"][0] == 1


def test_every_conv_entry_point_has_a_case():
    used = {(r, c["dtype"]) for c in CASES.values() for r in (c["fwd"], c["dgrad"], c["wgrad"]) if r}
    for r in K.ENTRY:
        assert any(u[0] == r for u in used), r
    assert {("genf", "f32"), ("genf", "bf16"), ("gend", "f32"), ("gend", "bf16"), ("rowsw", "bf16"), ("rowsw32", "f32")} <= used
    # the switches are restored
    from cplxmodule_amd import conv
    assert (conv._ROWS_FORCE, conv._CL_FORCE, conv._CL_PATCH) == (False, False, True)


@pytest.mark.parametrize("name", list(CASES))
def test_magnitude_bound_and_exact_representation(name):
    """Every partial sum is an integer (half-integer with the bias) below 2^24: float32 holds it whatever the order."""
    c = CASES[name]
    bound = K.magnitude_bound(c)
    assert bound < 2 ** 24
    d, ref = K.reference(c)
    for k, v in ref.items():
        assert np.abs(v).max() <= bound, k
        assert np.array_equal(np.round(2 * v), 2 * v), k            # an integer or a half-integer
        K.expected(v, "f32")                                         # (asserts float32 holds it)
    for k, v in d.items():
        if k != "emul":
            assert np.array_equal(np.round(2 * v), 2 * v) and np.abs(v).max() <= (8 if k[0] == "b" else 2 if k[0] == "w" else 3)
            assert np.array_equal(torch.tensor(v).bfloat16().double().numpy(), v)       # the cast to bf16 is exact


# ---- do the bf16 results exercise the rounding? ------------------------------------------------------------------------------
# A stored bf16 value tests the rounding only if one rounding changes it; a tie also tells round-half-even from
# round-half-away.  Whether a case CAN have such values follows from its geometry alone, by this model: an element of y or dx
# that sees `taps` kernel taps inside the image sums T = planes * channels * taps products of independent x in [-3, 3] and w in
# [-2, 2] (E x^2 = 4, E w^2 = 2), i.e. an integer of standard deviation sqrt(8 T), plus, for y, a bias uniform in {k/2}.
# bf16 holds half-integers below 128 and integers below 256, so small sums never change.  The model is evaluated exactly
# (every integer within 6 sd, every bias, torch's own rounding), per number of valid taps, and agrees with the references to
# about a tenth of its value.  Hence: the 5 % criterion is asserted wherever the model predicts 6.5 % or more, and at least one
# tie wherever it expects ten or more (a Poisson count of mean 10 is zero with probability 5e-5).  What is left over is listed
# by name below, with the reason, and the list is checked against the model.
def _valid_taps(n_out, n_in, k, s, p, d, on_input):
    """Kernel taps inside the image per output position (forward) / contributions per input position (data gradient)."""
    per_out, per_in = np.zeros(n_out, int), np.zeros(n_in, int)
    for o in range(n_out):
        for t in range(k):
            i = o * s - p + t * d
            if 0 <= i < n_in:
                per_out[o] += 1
                per_in[i] += 1
    return per_in if on_input else per_out


def predicted_rounding(c, out):
    """(fraction of the bf16 elements of `out` = 'y' | 'dx' that one rounding changes, fraction that are exact ties)."""
    Ho, Wo = K.out_hw(c)
    on_input = (out == "dx") != (c["api"] == "transpose")        # the elements live on the convolution's input image
    taps = np.outer(*(_valid_taps(o, i, c["k"][a], c["stride"][a], c["padding"][a], c["dilation"][a], on_input)
                      for a, (o, i) in enumerate(((Ho, c["H"]), (Wo, c["W"]))))).ravel()
    chans = (2 if K.is_cplx(c) else 1) * (c["Co"] if on_input else c["Ci"]) // c["groups"]
    bias = np.arange(-16, 17) / 2 if out == "y" else np.zeros(1)
    changed = tie = 0.0
    for n, count in zip(*np.unique(taps, return_counts=True)):
        sd = np.sqrt(8.0 * chans * n)
        ints = np.arange(-int(6 * sd) - 1, int(6 * sd) + 2, dtype=np.float64)
        w = np.exp(-0.5 * (ints / sd) ** 2) if sd else (ints == 0).astype(np.float64)
        w = w / w.sum() * count / taps.size / len(bias)
        low = torch.tensor(ints[:, None] + bias[None, :], dtype=torch.float32).view(torch.int32) & 0xffff
        changed += float((w[:, None] * (low != 0).double().numpy()).sum())
        tie += float((w[:, None] * (low == 0x8000).double().numpy()).sum())
    return changed, tie


def _bf16_outputs(c):
    """[(kind, reference planes)] of the bf16 results the case's kernels store."""
    if c["dtype"] != "bf16":
        return []
    ref = K.reference(c)[1]
    outs = []
    if c["fwd"]:
        outs.append(("y", np.stack([v for k, v in ref.items() if k[0] == "y"])))
    if c["dgrad"]:
        outs.append(("dx", np.stack([v for k, v in ref.items() if k.startswith("dx")])))
    return outs


def _asserted(c):
    """{(kind, 'five_percent' | 'tie')}: what the model says the case can show."""
    want = set()
    for kind, planes in _bf16_outputs(c):
        changed, tie = predicted_rounding(c, kind)
        if changed >= 0.065:
            want.add((kind, "five_percent"))
        if tie * planes.size >= 10:
            want.add((kind, "tie"))
    return want


# bf16 cases in which neither result can show a single rounding: the shapes that cross the kernels' seams are too small for it.
_FEW = "at most 8 or 24 channels: sums stay below 128, every value is representable"
_ROW = "a one-row image: two of the three kernel rows fall on the padding, the sums of 64 channels x 3 taps rarely pass 128"
NO_ROUNDING_POSSIBLE = {
    "cl2_one_pixel": "1 x 1 image: one tap of nine inside the image", "cl_one_pixel": "1 x 1 image: one tap of nine inside the image",
    "clw_one_row_w1": "1 x 1 image: one tap of nine inside the image",
    "rows_grid_321": "one-row image, 32 channels", "clr_one_row_w31": _ROW + " (real: half the products)",
    "clr_one_row_w33": _ROW + " (real: half the products)",
    **{f"rowsw_real_bf16_kw{k}": _FEW for k in (1, 2, 3, 4)}, **{f"rowsw_cplx_bf16_kw{k}": _FEW for k in (3, 4)},
    "rowsw_1x1_is_linear": "1 x 1 kernel: 128 products, sd 32",
    "g16_stride2": "3 x 1 kernel on 32 channels, stride 2: 192 products at most, a fraction of them per input pixel",
    **{f"g16_pixels_{n}_co72": "K is ONE 32-tile by construction: 8 channels x 2 x 2 taps" for n in (63, 64, 65)},
    "gen_bf16_stride23": "Ci = 3, Co = 5", "gen_bf16_groups": "3 and 5 channels per group", "gen_bf16_one_pixel": "Ci = 3, 1 x 1 image",
    "real_generic_bf16": "Ci = 3, Co = 5, real",
    "transpose_stride2_outpad_bf16": "stride 2: an output pixel sees a quarter of the 9 x 32 taps (transpose_stride1_widened "
                                     "covers this route's rounding)",
}

_BF16 = [n for n, c in CASES.items() if c["dtype"] == "bf16"]


def test_cases_without_rounding_are_the_listed_ones():
    assert {n for n in _BF16 if not _asserted(CASES[n])} == set(NO_ROUNDING_POSSIBLE)


@pytest.mark.parametrize("name", [n for n in _BF16 if n not in NO_ROUNDING_POSSIBLE])
def test_bf16_case_exercises_the_rounding(name):
    c = CASES[name]
    want = _asserted(c)
    assert want
    for kind, planes in _bf16_outputs(c):
        changed, ties = K.rounding_content(planes)
        if (kind, "five_percent") in want:
            assert changed >= 0.05, (kind, changed)
        if (kind, "tie") in want:
            assert ties >= 1, kind


def test_every_kernel_that_stores_bf16_has_a_rounding_case():
    """Forward kernels through y, data-gradient kernels through dx, the transposed operator's forward (the data-gradient
    kernels + bias) apart: each has a case that meets the 5 % criterion and has ties."""
    have, rich = set(), set()
    for n in _BF16:
        c = CASES[n]
        want = _asserted(c)
        for kind, route in (("y", c["fwd"]), ("dx", c["dgrad"])):
            if route:
                key = (c["api"] == "transpose", kind, route)
                have.add(key)
                if {(kind, "five_percent"), (kind, "tie")} <= want:
                    rich.add(key)
    # (the transposed operator's data gradient is the forward kernels without a bias: covered as (False, 'y', ...))
    assert {k for k in have - rich if not (k[0] and k[1] == "dx")} == set()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if K.uses_oracle(c)])
def test_oracle_equals_torch_float64(name):
    c = CASES[name]
    d = K.make_inputs(c)
    a, b = K._oracle_reference(c, d), K._torch_reference(c, d)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def test_float32_aten_equals_float64_on_such_data():
    c = CASES["cl2_ci96"]
    d, ref = K.reference(c)
    f = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    conv = lambda x, w: torch.nn.functional.conv2d(f(x), f(w), padding=1)  # noqa: E731
    yr = conv(d["xr"], d["wr"]) - conv(d["xi"], d["wi"]) + f(d["br"]).view(1, -1, 1, 1)
    assert np.array_equal(yr.double().numpy(), ref["yr"])


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["fp32"] == "x2"])
def test_x2_split_is_exact_on_these_operands(name):
    """The half pieces of integer operands: the scaled value is representable (second piece zero), and every piece product
    sum is (s_a s_b) times an integer below 2^24 -- float32 holds it, and the power-of-two scales come off exactly."""
    c = CASES[name]
    d, ref = K.reference(c)
    sc = {}
    for op in ("x", "w", "g"):
        both = np.stack([d[op + "r"], d[op + "i"]])                 # the planes of a complex operand share one scale
        s, p0, p1 = K.emulate_x2_split(both)
        assert not p1.any() and np.array_equal(p0, both * s)
        assert 2 ** 14 <= np.abs(p0).max() < 2 ** 15
        sc[op] = s
    bias = {"yr": d["br"], "yi": d["bi"]}
    for out, (a, b) in dict(yr="xw", yi="xw", dxr="gw", dxi="gw", dwr="gx", dwi="gx").items():
        v = ref[out] - (bias[out][None, :, None, None] if out in bias else 0)
        assert np.array_equal(np.round(v), v) and np.abs(v).max() < 2 ** 24
        scaled = v * (sc[a] * sc[b])
        f32 = scaled.astype(np.float32)
        assert np.array_equal(f32.astype(np.float64), scaled)
        assert np.array_equal((f32 * np.float32(1 / sc[a]) * np.float32(1 / sc[b])).astype(np.float64), v)


def test_describe_mismatch_names_the_seam():
    c = CASES["cl2_tile_plus_one"]
    _, ref = K.reference(c)
    want = K.expected(ref["yr"], "bf16")
    assert K.describe_mismatch(want, want, c, "yr") == ""
    assert K.describe_mismatch(-0.0 * want, 0.0 * want, c, "yr") == ""           # by value
    got = want.copy()
    got[1, 63, 16, 32] += 1
    got[0, 5, 3, 4] += 1
    msg = K.describe_mismatch(got, want, c, "yr")
    assert msg.startswith("yr: 2 of ") and "(1, 63, 16, 32)" in msg and "image border" in msg and "tile border" in msg
    assert "(0, 5, 3, 4)" in msg and "16-channel slice 0" in msg
    c = CASES["rows_co40"]
    want = K.expected(K.reference(c)[1]["dwr"], "f32")
    got = want.copy()
    got[39, 0, 2, 1] = np.nan
    msg = K.describe_mismatch(got, want, c, "dwr")
    assert "1 of" in msg and "Co channel-tile tail" in msg and "tap 2,1" in msg
