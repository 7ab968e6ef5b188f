"""Case table, operand generator and exact reference of the CplxConvTranspose3d tests (test_conv_transpose3d_host.py,
test_gpu_conv_transpose3d.py).

As in conv_exact_cases.py the operands are small integers -- activations and output gradients in [-3, 3], weights in
[-2, 2], biases in {k/2 : |k| <= 16} -- so every product and every partial sum is an integer (or a half-integer) far below
2^24: exactly representable in float32 in any order of accumulation, any split-K schedule, any tiling.  csrc/conv3d.hip must
therefore give

    float32 results   exactly the float64 reference,
    bf16 results      exactly reference.float().bfloat16(): ONE round-to-nearest-even of a known value,

over the whole tensor.  The reference is the reference package's own formula (cplx.conv_transposend_naive + bias,
cplxmodule/cplx.py:860-873, 931-943) on torch's CPU float64 F.conv_transpose3d and its autograd.

Shapes are in the transposed layer's terms (cin -> cout channels, input D x H x W) and are the smallest at which the kernel
can go wrong; its tile is 64 channels x 64 voxels x 16 K (csrc/conv3d.hip).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

TILE = 64
CASES = {}


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def case(name, B, cin, cout, dhw, k, stride=1, padding=0, output_padding=0, dilation=1, groups=1, bias=True,
         padding_mode="zeros"):
    assert name not in CASES, name
    CASES[name] = dict(name=name, B=B, cin=cin, cout=cout, dhw=tuple(dhw), k=_triple(k), stride=_triple(stride),
                       padding=_triple(padding), output_padding=_triple(output_padding), dilation=_triple(dilation),
                       groups=groups, bias=bias, padding_mode=padding_mode)


FIRST = dict(B=2, cin=3, cout=5, dhw=(3, 4, 5), k=(2, 3, 4))
# all of D, H, W and kd, kh, kw differ (an axis swap cannot cancel); 60 voxels per image, 120 in all: a 64-voxel tile of
# the backward's forward-correlation straddles two images, and so do the tiles of the 4 x 6 x 8 = 192-voxel outputs;
# K = 3 * 24 = 72 and 5 * 24 = 120: no multiples of 16
case("all_different", **FIRST)
# M crosses a tile: 70 rows in the forward pass (6 -> 70) and in dx (70 -> 6); dw rows cross a tile in both
case("m_70_to_6", B=1, cin=70, cout=6, dhw=(2, 3, 4), k=3, padding=1)
case("m_6_to_70", B=1, cin=6, cout=70, dhw=(2, 3, 4), k=3, padding=1)
# stride 2 in every dimension: eight phases
_S2 = dict(B=2, cin=4, cout=3, dhw=(3, 4, 5), stride=2)
case("s2_k2_one_tap_each", k=2, **_S2)
case("s2_k4_p1", k=4, padding=1, **_S2)
case("s2_k3_p1_op1_unequal_taps", k=3, padding=1, output_padding=1, **_S2)
# mixed strides: 4 phases, one dimension on the unit-stride progression
case("mixed_122", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=(3, 2, 3), stride=(1, 2, 2))
case("mixed_212", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=(3, 2, 3), stride=(2, 1, 2))
# an empty phase: kernel 1, stride 2 -- seven of eight classes have no tap and must hold the bias / zeros
case("empty_phase_bias", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=1, stride=2, output_padding=1)
case("empty_phase_nobias", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=1, stride=2, output_padding=1, bias=False)
# stride 3: the plain path (divisibility tested per tap)
case("plain_s3", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=(2, 3, 4), stride=3, padding=(0, 1, 2), output_padding=(2, 1, 0))
# dilation with stride; dilation 2 at stride 2 has gcd(d, s) != 1: every tap lands in ONE residue class
case("dil_213_s1", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=(2, 3, 2), dilation=(2, 1, 3))
case("dil2_s2", B=2, cin=4, cout=3, dhw=(3, 4, 5), k=3, stride=2, dilation=2, padding=1, output_padding=1)
# groups; 70 -> 70 in two groups: M = 35 per group is narrower than a tile, which must not read into the next group
case("groups2", B=2, cin=4, cout=6, dhw=(3, 4, 5), k=(2, 3, 2), groups=2)
case("depthwise", B=2, cin=4, cout=4, dhw=(3, 4, 5), k=(2, 3, 2), groups=4, stride=(1, 2, 1))
case("groups2_70_70", B=1, cin=70, cout=70, dhw=(2, 3, 4), k=3, padding=1, groups=2)
# minimal input: one voxel, one image
case("one_voxel", B=1, cin=3, cout=5, dhw=(1, 1, 1), k=3)
# split-K weight gradient: K = 2 * 8 * 16 * 16 = 4096 voxels against 4 tiles -> several slabs
# (test_conv_transpose3d_host.py asserts it from the workspace query)
case("splitk", B=2, cin=8, cout=8, dhw=(8, 16, 16), k=3, padding=1)
# circular padding (1, 2, 3): padding[0] wraps W, padding[2] wraps D (the reference's F.pad order)
case("circular", padding=(1, 2, 3), padding_mode="circular", **FIRST)

RANDOM_CASES = ("mixed_122", "m_70_to_6")


def pads_of(c):
    """The reference's symmetric circular padding, F.pad order (cplxmodule/cplx.py:701-714)."""
    out = []
    for p in c["padding"]:
        out.extend(((p + 1) // 2, p // 2))
    return tuple(out)


def in_dhw(c):
    """Input extents the kernel sees (circular mode pads the input first)."""
    if c["padding_mode"] != "circular":
        return c["dhw"]
    p = c["padding"]
    return (c["dhw"][0] + p[2], c["dhw"][1] + p[1], c["dhw"][2] + p[0])


def eff_padding(c):
    return (0, 0, 0) if c["padding_mode"] == "circular" else c["padding"]


def out_dhw(c):
    return tuple((L - 1) * s - 2 * p + d * (k - 1) + o + 1 for L, s, p, d, k, o in zip(
        in_dhw(c), c["stride"], eff_padding(c), c["dilation"], c["k"], c["output_padding"]))


def shapes(c):
    """x (input), w [cin, cout / groups, kd, kh, kw], y (output)."""
    return ((c["B"], c["cin"]) + c["dhw"], (c["cin"], c["cout"] // c["groups"]) + c["k"], (c["B"], c["cout"]) + out_dhw(c))


def geom_of(c):
    """int[19] geometry of the equivalent forward correlation (its input is the layer's OUTPUT)."""
    return [c["B"], c["cout"], c["cin"], *out_dhw(c), *c["k"], *c["stride"], *eff_padding(c), *c["dilation"], c["groups"]]


def terms(c):
    """(forward, data gradient, weight gradient): complex products summed into one output element, at most."""
    taps = c["k"][0] * c["k"][1] * c["k"][2]
    D, H, W = in_dhw(c)
    return (c["cin"] // c["groups"]) * taps, (c["cout"] // c["groups"]) * taps, c["B"] * D * H * W


def magnitude_bound(c):
    """Largest magnitude a partial sum can reach: 2 K real products per complex sum, |x w| <= 6 (+ a bias of at most 8),
    |g x| <= 9 in the weight gradient."""
    tf, td, tw = terms(c)
    return max(2 * tf * 6 + 8, 2 * td * 6 + 8, 2 * tw * 9)


def make_inputs(c, gaussian=False):
    """float64 numpy operands, planar, seeded by the case name: integer-valued (biases half-integers), or Gaussian."""
    rs = np.random.RandomState(zlib.crc32((c["name"] + ("/g" if gaussian else "")).encode()) & 0x7fffffff)
    xs, ws, ys = shapes(c)
    if gaussian:
        ints = lambda lo, hi, s: rs.standard_normal(s) * (0.3 if hi == 2 else 1.0)  # noqa: E731
    else:
        ints = lambda lo, hi, s: rs.randint(lo, hi + 1, size=s).astype(np.float64)  # noqa: E731
    d = {}
    for p in "ri":
        d["x" + p], d["w" + p], d["g" + p] = ints(-3, 3, xs), ints(-2, 2, ws), ints(-3, 3, ys)
        if c["bias"]:
            d["b" + p] = ints(-16, 16, (c["cout"],)) / 2
    return d


def torch_reference(c, d):
    """re = ct(xr, wr) - ct(xi, wi), im = ct(xr, wi) + ct(xi, wr), plus the bias; gradients by autograd.  float64, CPU."""
    t = {k: torch.tensor(np.asarray(v, dtype=np.float64)).requires_grad_(k[0] in "xwb") for k, v in d.items()}
    a, b = t["xr"], t["xi"]
    if c["padding_mode"] == "circular":
        a, b = F.pad(a, pads_of(c), mode="circular"), F.pad(b, pads_of(c), mode="circular")
    kw = dict(stride=c["stride"], padding=eff_padding(c), output_padding=c["output_padding"], groups=c["groups"],
              dilation=c["dilation"])
    ct = lambda u, w: F.conv_transpose3d(u, w, None, **kw)  # noqa: E731
    yr = ct(a, t["wr"]) - ct(b, t["wi"])
    yi = ct(a, t["wi"]) + ct(b, t["wr"])
    if c["bias"]:
        yr, yi = yr + t["br"].view(1, -1, 1, 1, 1), yi + t["bi"].view(1, -1, 1, 1, 1)
    torch.autograd.backward((yr, yi), (t["gr"], t["gi"]))
    out = dict(yr=yr, yi=yi, dxr=t["xr"].grad, dxi=t["xi"].grad, dwr=t["wr"].grad, dwi=t["wi"].grad)
    if c["bias"]:
        out.update(dbr=t["br"].grad, dbi=t["bi"].grad)
    return {k: v.detach().numpy() for k, v in out.items()}


_cache = {}


def reference(c):
    """-> (inputs, exact float64 results yr, yi, dxr, dxi, dwr, dwi(, dbr, dbi)).  Computed once per case and read-only:
    the dtypes and layouts of a case share it."""
    hit = _cache.get(c["name"])
    if hit is None:
        d = make_inputs(c)
        ref = torch_reference(c, d)
        for v in list(d.values()) + list(ref.values()):
            v.setflags(write=False)
        hit = _cache[c["name"]] = (d, ref)
    return hit


def expected(ref, dtype):
    """What the kernel must return for the exact value `ref`: the value itself in float32, its one rounding in bf16."""
    t = torch.tensor(np.ascontiguousarray(ref), dtype=torch.float32)
    assert np.array_equal(t.double().numpy(), ref), "the reference is not exactly representable in float32"
    return (t.bfloat16().float() if dtype == "bf16" else t).numpy()


def describe_mismatch(got, ref, which):
    """'' if got == ref everywhere (by value), else the count and the first few coordinates."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"{which}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(~(got == ref))
    if bad.size == 0:
        return ""
    lines = [f"{which}: {len(bad)} of {ref.size} values differ (shape {ref.shape})"]
    for idx in bad[:6]:
        idx = tuple(int(i) for i in idx)
        lines.append(f"  {idx}: got {got[idx]!r}, want {ref[idx]!r}")
    return "\n".join(lines)


# geometries of cplxamd_conv3d_out_shape beyond the cases: (D, H, W), kernel, stride, padding, dilation
EXTRA_GEOMETRIES = (
    ((7, 8, 9), (3, 3, 3), (1, 1, 1), (0, 0, 0), (1, 1, 1)),
    ((7, 8, 9), (3, 2, 1), (2, 3, 1), (1, 0, 0), (1, 2, 1)),
    ((16, 5, 11), (5, 3, 4), (3, 2, 2), (2, 1, 3), (2, 1, 2)),
    ((1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1)),
    ((4, 4, 4), (4, 4, 4), (4, 4, 4), (0, 0, 0), (1, 1, 1)),
    ((9, 10, 11), (2, 2, 2), (2, 2, 2), (3, 3, 3), (5, 5, 5)),
)
