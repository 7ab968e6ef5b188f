"""Case table, operand generator and exact reference of the bit-exact convolution tests (test_conv_exact_host.py,
test_gpu_conv_exact.py).

The operands are small integers -- activations and output gradients in [-3, 3], weights in [-2, 2], biases in
{k/2 : |k| <= 16} -- so every product and every partial sum of a convolution is an integer (or a half-integer) far below
2^24: exactly representable in float32 whatever the order of accumulation, the split-K schedule, the MFMA shape or the
tiling.  Every route of the dispatcher (cplxmodule_amd/conv.py) must therefore give

    float32 outputs   exactly the float64 reference,
    bf16 outputs      exactly torch.tensor(ref, dtype=float32).bfloat16(): ONE round-to-nearest-even of a known value,

over the whole tensor.  A case names the entry points its forward, data gradient and weight gradient are expected to run
(`fwd`, `dgrad`, `wgrad`: keys of ENTRY); the GPU test records what `conv.call` / `conv.try_call` ran and fails a case that
fell through to another kernel.

Tile constants the shapes are built around (read from the kernels):
    conv_cl2.hip        3 x 3, dilation 1: 16 x 32-pixel tiles (TH, TW), 64-channel column tiles, C % 32 == 0
    conv_cl.hip         rows of TM = 512 pixels of which tm_out = 512 - (KW - 1) dil_w are written, KH (C / 16) % 6 == 0
    conv_cl_wgrad.hip   3 x 3, Ci % 64 == Co % 64 == 0, 32-pixel stages per image row, >= 16 stages per split
    conv_nhwc*.hip      256-row tiles of the padded grid staged through 320-row windows, 64-channel column tiles,
                        at most 32 halo columns, 32 (bf16) / 16 (float32) channels per stage
    conv_bf16.hip       64 x 64 tiles, K = (Ci / groups) KH KW in 32-tiles
"""
import contextlib
import zlib

import numpy as np
import torch
import torch.nn.functional as F

ENTRY = {
    "cl2": "cplxamd_conv2d_cl2_fl", "cl": "cplxamd_conv2d_cl_fl", "clw": "cplxamd_conv2d_cl_wgrad_fl",
    "rows": "cplxamd_conv2d_nhwc", "rows32": "cplxamd_conv2d_nhwc_f32",
    "rowsw": "cplxamd_conv2d_nhwc_wgrad", "rowsw32": "cplxamd_conv2d_nhwc_wgrad_f32", "lin": "cplxamd_cgemm_fl",
    "g16f": "cplxamd_conv2d_bf16_fwd", "g16d": "cplxamd_conv2d_bf16_dgrad", "g16d32": "cplxamd_conv2d_bf16_dgrad_f32",
    "g16w": "cplxamd_conv2d_bf16_wgrad",
    "genf": "cplxamd_conv2d_fwd", "gend": "cplxamd_conv2d_dgrad", "genw": "cplxamd_conv2d_wgrad_bias",
    "x2": "cplxamd_conv2d_cl2h_wrap_fl", "x2w": "cplxamd_conv2d_clh_wgrad_skip_fl",
    "clr": "cplxamd_conv2d_clr_fl", "clrw": "cplxamd_conv2d_clr_wgrad_fl",
}
COMPUTE = frozenset(ENTRY.values())          # everything else conv.py calls is data movement (pads, packs, tables, sums)

CL2_TH, CL2_TW, CL_TM, CLW_KR, ROWS_BM, GATHER_BN = 16, 32, 512, 32, 256, 64

CASES = {}


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def case(name, api, B, Ci, Co, H, W, k=3, stride=1, padding=0, dilation=1, groups=1, dtype="bf16", layouts=("nchw",),
         rows=False, cl=False, patch=True, fp32="exact", fwd=None, dgrad=None, wgrad=None, output_padding=0):
    """api: 'cplx' cplx.conv2d + autograd | 'direct' conv.cl_conv / conv.cl_wgrad (a layer that stays planar as a whole) |
    'real' RealConv2dFn | 'cl_real' conv.cl_conv_real / conv.cl_wgrad_real | 'transpose' cplx.conv_transpose2d |
    'conv1d' cplx_conv1d (H must be 1).  For 'transpose' Ci / Co are the channels of the equivalent convolution (the
    operator maps Co -> Ci channels) and H, W its INPUT image, i.e. the transposed operator's output.
    rows / cl / patch / fp32: conv._ROWS_FORCE, conv._CL_FORCE, conv._CL_PATCH, x3.fp32_mode.
    fwd / dgrad / wgrad: ENTRY keys the operator's forward, data gradient and weight gradient must run (None: not run)."""
    assert name not in CASES, name
    CASES[name] = dict(name=name, api=api, B=B, Ci=Ci, Co=Co, H=H, W=W, k=_pair(k), stride=_pair(stride),
                       padding=_pair(padding), dilation=_pair(dilation), groups=groups, dtype=dtype, layouts=tuple(layouts),
                       rows=rows, cl=cl, patch=patch, fp32=fp32, fwd=fwd, dgrad=dgrad, wgrad=wgrad,
                       output_padding=_pair(output_padding))


BOTH = ("nchw", "channels_last")

# ---- 1. conv_cl2.hip: forward and data gradient (+ conv_cl_wgrad.hip where the whole layer is channels-last) ------------------
_cl_layer = dict(api="cplx", cl=True, fwd="cl2", dgrad="cl2", wgrad="clw")
_TILE_EDGE = {                                        # name -> (B, H, W, padding): the tile-edge images
    "one_tile": (2, 16, 32, 1), "tile_plus_one": (2, 17, 33, 1), "one_pixel": (2, 1, 1, 1), "three_by_two": (5, 3, 2, 1),
    "valid_one_tile": (2, 18, 34, 0), "pad_1_0": (2, 17, 35, (1, 0)), "tiles_cross_images": (3, 20, 40, 1),
}
for _n, (_B, _H, _W, _p) in _TILE_EDGE.items():
    case(f"cl2_{_n}", B=_B, Ci=64, Co=64, H=_H, W=_W, padding=_p, layouts=BOTH, **_cl_layer)
case("cl2_ci128_co64", B=2, Ci=128, Co=64, H=17, W=33, padding=1, **_cl_layer)
case("cl2_ci64_co128", B=2, Ci=64, Co=128, H=6, W=33, padding=1, layouts=BOTH, **_cl_layer)
# 2 * 256 * 9 = 4608 products per dx element (sd 192): the data gradient's rounding, which has no bias to help it
case("cl2_dgrad_co256_rounding", B=1, Ci=64, Co=256, H=8, W=33, padding=1, **_cl_layer)
# Ci % 64 != 0: no channels-last weight gradient, the layer stays planar as a whole -> the kernel directly
case("cl2_three_by_two_c32", "direct", B=5, Ci=32, Co=64, H=3, W=2, padding=1, cl=True, fwd="cl2", layouts=BOTH)
case("cl2_ci32_co128", "direct", B=2, Ci=32, Co=128, H=17, W=33, padding=1, cl=True, fwd="cl2")
case("cl2_ci96", "direct", B=3, Ci=96, Co=64, H=40, W=37, padding=1, cl=True, fwd="cl2", layouts=BOTH)
# 80 * 2 * 2 = 320 tiles > 256 workgroups: the ring and the bias DMA run through tile boundaries
case("cl2_many_tiles", "direct", B=80, Ci=32, Co=64, H=17, W=33, padding=1, cl=True, fwd="cl2", layouts=BOTH)

# ---- 2. conv_cl.hip, the row kernel ---------------------------------------------------------------------------------------------
_row_layer = dict(api="cplx", cl=True, patch=False, fwd="cl", dgrad="cl", wgrad="clw")
for _n, (_B, _H, _W, _p) in _TILE_EDGE.items():
    case(f"cl_{_n}", B=_B, Ci=64, Co=64, H=_H, W=_W, padding=_p, **_row_layer)
case("cl_dgrad_co256_rounding", B=1, Ci=64, Co=256, H=8, W=33, padding=1, **_row_layer)
case("cl_ci96", "direct", B=3, Ci=96, Co=64, H=40, W=37, padding=1, cl=True, patch=False, fwd="cl")
case("cl_ci32_co128", "direct", B=2, Ci=32, Co=128, H=17, W=33, padding=1, cl=True, patch=False, fwd="cl")
# shapes it alone takes
case("cl_1x3", "direct", B=2, Ci=96, Co=64, H=9, W=30, k=(1, 3), padding=(0, 1), cl=True, fwd="cl", layouts=BOTH)
case("cl_1x3_dgrad", "direct", B=2, Ci=64, Co=192, H=9, W=30, k=(1, 3), padding=(0, 1), cl=True, dgrad="cl")
case("cl_5x3_dil23", "direct", B=2, Ci=96, Co=64, H=14, W=15, k=(5, 3), padding=(4, 3), dilation=(2, 3), cl=True, fwd="cl")
case("cl_3x3_dil2", B=2, Ci=64, Co=64, H=12, W=20, padding=2, dilation=2, api="cplx", cl=True, fwd="cl", dgrad="cl",
     wgrad="clw", layouts=BOTH)
# pixel counts tm_out - 1, tm_out, tm_out + 1 (tm_out = 512 - 2 = 510)
case("cl_pixels_509", B=1, Ci=64, Co=64, H=1, W=509, padding=1, **_row_layer)
case("cl_pixels_510", B=1, Ci=64, Co=64, H=2, W=255, padding=1, **_row_layer)
case("cl_pixels_511", B=1, Ci=64, Co=64, H=7, W=73, padding=1, **_row_layer)
case("cl_width_1", B=3, Ci=64, Co=64, H=5, W=1, padding=1, **_row_layer)
case("cl_width_2", B=3, Ci=64, Co=64, H=5, W=2, padding=1, **_row_layer)
case("cl_row_spans_tiles", B=1, Ci=64, Co=64, H=2, W=520, padding=1, **_row_layer)

# ---- 3. conv_cl_wgrad.hip (through the whole channels-last layer) -------------------------------------------------------------
for _W in (1, 31, 32, 33, 64):
    case(f"clw_one_row_w{_W}", B=3, Ci=64, Co=64, H=1, W=_W, padding=1, **_cl_layer)
_dil_layer = dict(api="cplx", cl=True, fwd="cl", dgrad="cl", wgrad="clw")
for _d, _H, _W in ((2, 9, 40), (4, 12, 45)):
    for _tag, _p in (("pad0", 0), ("pad_below", (_d // 2, _d - 1)), ("pad_same", _d)):
        case(f"clw_dil{_d}_{_tag}", B=2, Ci=64, Co=64, H=_H, W=_W, padding=_p, dilation=_d, **_dil_layer)
case("clw_ci128_co64", B=2, Ci=128, Co=64, H=6, W=33, padding=1, **_cl_layer)
case("clw_ci64_co128", B=2, Ci=64, Co=128, H=6, W=33, padding=1, **_cl_layer)
# 2 * 10 * 2 = 40 stages -> at most ceil(40 / 16) = 3 splits of 14, 14, 12 stages
case("clw_three_splits_remainder", B=2, Ci=64, Co=64, H=10, W=64, padding=1, **_cl_layer)

# ---- 4. conv_nhwc.hip / conv_nhwc_f32.hip / conv_nhwc_wgrad.hip (shifted rows of the padded grid, _ROWS_FORCE) ----------------
_rows = dict(api="cplx", rows=True, fwd="rows", dgrad="rows", wgrad="rowsw")
case("rows_grid_319", B=1, Ci=32, Co=64, H=9, W=27, padding=1, **_rows)           # 11 * 29 padded rows
case("rows_grid_320", B=1, Ci=32, Co=64, H=14, W=18, padding=1, **_rows)          # 16 * 20
case("rows_grid_321", B=1, Ci=32, Co=64, H=1, W=105, padding=1, **_rows)          # 3 * 107
case("rows_co40", "cplx", B=3, Ci=32, Co=40, H=17, W=16, rows=True, fwd="rows", dgrad="gend", wgrad="rowsw")
case("rows_co72", "cplx", B=2, Ci=64, Co=72, H=10, W=11, padding=1, rows=True, fwd="rows", dgrad="gend", wgrad="rowsw")
case("rows_1x5", "cplx", B=5, Ci=96, Co=64, H=11, W=10, k=(1, 5), padding=(0, 4), rows=True, fwd="rows", dgrad="rows",
     wgrad="g16w")          # (KW = 5: the shifted-row weight gradient stops at KW = 4)
case("rows_3x2", "cplx", B=2, Ci=64, Co=32, H=14, W=37, k=(3, 2), padding=(1, 0), rows=True, fwd="rows", dgrad="rows",
     wgrad="g16w")          # (complex, KW = 2: more staging pieces than the shifted-row weight gradient has)
case("rows_halo_limit_dil16", B=2, Ci=32, Co=64, H=8, W=40, padding=(1, 16), dilation=(1, 16), **_rows)
case("rows_ci96_rounding", B=2, Ci=96, Co=64, H=12, W=13, padding=1, **_rows)
case("rows_dgrad_co256_rounding", B=2, Ci=32, Co=256, H=9, W=10, padding=1, **_rows)
case("rows_f32_ci16", "cplx", B=2, Ci=16, Co=32, H=12, W=11, padding=1, dtype="f32", rows=True, fwd="rows32", dgrad="rows32",
     wgrad="rowsw32")
case("rows_f32_ci16_co40", "cplx", B=3, Ci=16, Co=40, H=12, W=11, k=(3, 2), padding=(2, 0), dilation=(2, 1), dtype="f32",
     rows=True, fwd="rows32", dgrad="gend", wgrad="genw")
# the shifted-row weight gradient, KW = 1..4, channel counts 8 and 24 (complex planes fit its 8 staging pieces from KW = 3 on)
for _kw in (1, 2, 3, 4):
    for _api in ("real", "cplx")[:1 if _kw < 3 else 2]:
        _g = lambda C: (C * 2 * _kw) % 32 == 0  # noqa: E731  (K of the gather kernels in whole 32-tiles)
        case(f"rowsw_{_api}_bf16_kw{_kw}", _api, B=2, Ci=8, Co=24, H=9, W=14, k=(2, _kw), padding=(1, _kw - 1), rows=True,
             fwd="g16f" if _g(8) else "genf", dgrad="g16d" if _g(24) else "gend", wgrad="rowsw")
        case(f"rowsw_{_api}_f32_kw{_kw}", _api, B=2, Ci=24, Co=8, H=9, W=14, k=(2, _kw), padding=(1, _kw - 1), dtype="f32",
             rows=True, fwd="genf", dgrad="gend", wgrad="rowsw32")
case("rowsw_1x1_is_linear", "cplx", B=1, Ci=64, Co=96, H=9, W=9, k=1, rows=True, fwd="rows", dgrad="rows", wgrad="lin")

# ---- 5. conv_bf16.hip gather kernels -------------------------------------------------------------------------------------------
case("g16_stride2", "cplx", B=2, Ci=32, Co=32, H=15, W=14, k=(3, 1), stride=2, padding=(1, 0), fwd="g16f", dgrad="gend",
     wgrad="g16w")
case("g16_groups2_dil2", "cplx", B=2, Ci=64, Co=64, H=12, W=13, padding=2, dilation=2, groups=2, fwd="g16f", dgrad="g16d",
     wgrad="g16w")
for _px, (_H, _W) in ((63, (8, 10)), (64, (9, 9)), (65, (6, 14))):      # output pixels of a 2 x 2 kernel; K = one 32-tile
    case(f"g16_pixels_{_px}_co72", "cplx", B=1, Ci=8, Co=72, H=_H, W=_W, k=2, fwd="g16f", dgrad="g16d", wgrad="g16w")
case("g16_k_several_tiles_co40", "cplx", B=3, Ci=32, Co=40, H=10, W=20, fwd="g16f", dgrad="gend", wgrad="g16w")
case("g16_groups2_rounding", "cplx", B=2, Ci=192, Co=64, H=9, W=10, padding=1, groups=2, fwd="g16f", dgrad="g16d",
     wgrad="g16w")

case("g16_dgrad_co256_rounding", "cplx", B=2, Ci=32, Co=256, H=9, W=10, padding=1, fwd="g16f", dgrad="g16d", wgrad="g16w")

# ---- 6. the generic kernels (conv.hip) ------------------------------------------------------------------------------------------
for _dt, _w in (("f32", "genw"), ("bf16", "g16w")):
    _gen = dict(api="cplx", dtype=_dt, fwd="genf", dgrad="gend", wgrad=_w)
    case(f"gen_{_dt}_stride23", B=2, Ci=3, Co=5, H=11, W=13, stride=(2, 3), padding=1, **_gen)
    case(f"gen_{_dt}_groups", B=2, Ci=6, Co=10, H=7, W=9, padding=1, groups=2, **_gen)
    case(f"gen_{_dt}_one_pixel", B=3, Ci=3, Co=5, H=1, W=1, padding=1, **_gen)
case("gen_bf16_ci100_rounding", "cplx", B=2, Ci=100, Co=8, H=7, W=8, padding=1, fwd="genf", dgrad="gend", wgrad="g16w")
case("gen_bf16_dgrad_co280_rounding", "cplx", B=2, Ci=32, Co=280, H=7, W=8, padding=1, fwd="g16f", dgrad="gend", wgrad="g16w")

# ---- 7. float32 on IEEE-half pieces (fp32_mode 'x2': conv_cl2_f16.hip, conv_cl_wgrad_f16.hip) -----------------------------------
_x2 = dict(api="cplx", dtype="f32", fp32="x2", fwd="x2", dgrad="x2", wgrad="x2w")
for _n, (_B, _H, _W, _p) in _TILE_EDGE.items():
    case(f"x2_{_n}", B=_B, Ci=64, Co=64, H=_H, W=_W, padding=_p, layouts=BOTH if _n == "tile_plus_one" else ("nchw",), **_x2)
case("x2_ci128_co64", B=2, Ci=128, Co=64, H=17, W=33, padding=1, **_x2)

# ---- 8. real kernels --------------------------------------------------------------------------------------------------------------
_clr = dict(api="cl_real", cl=True, fwd="clr", dgrad="clr", wgrad="clrw")
for _n in ("one_tile", "tile_plus_one", "valid_one_tile", "tiles_cross_images"):
    _B, _H, _W, _p = _TILE_EDGE[_n]
    case(f"clr_{_n}", B=_B, Ci=64, Co=64, H=_H, W=_W, padding=_p, **_clr)
case("clr_dil2_pad_below", B=2, Ci=128, Co=64, H=11, W=32, padding=(1, 2), dilation=2, **_clr)
case("clr_pixels_509", B=1, Ci=64, Co=64, H=1, W=509, padding=1, **_clr)
case("clr_pixels_510", B=1, Ci=64, Co=64, H=2, W=255, padding=1, **_clr)
case("clr_pixels_511", B=1, Ci=64, Co=64, H=7, W=73, padding=1, **_clr)
case("clr_one_row_w31", B=3, Ci=64, Co=64, H=1, W=31, padding=1, **_clr)
case("clr_one_row_w33", B=3, Ci=64, Co=128, H=1, W=33, padding=1, **_clr)
case("clr_three_splits_remainder", B=2, Ci=64, Co=64, H=10, W=64, padding=1, **_clr)
case("clr_ci192_rounding", B=2, Ci=192, Co=64, H=17, W=33, padding=1, **_clr)
case("clr_dgrad_co512_rounding", B=1, Ci=64, Co=512, H=8, W=33, padding=1, **_clr)
case("real_cl_layer", "real", B=2, Ci=64, Co=64, H=17, W=33, padding=1, cl=True, fwd="clr", dgrad="clr", wgrad="clrw",
     layouts=BOTH)
case("real_rows", "real", B=2, Ci=32, Co=64, H=16, W=18, padding=1, rows=True, fwd="rows", dgrad="rows", wgrad="rowsw")
case("real_rows_ci192_rounding", "real", B=2, Ci=192, Co=64, H=9, W=10, padding=1, rows=True, fwd="rows", dgrad="rows",
     wgrad="rowsw")
case("real_gather", "real", B=2, Ci=32, Co=64, H=16, W=18, padding=1, fwd="g16f", dgrad="g16d", wgrad="g16w")
case("real_gather_ci192_rounding", "real", B=2, Ci=192, Co=64, H=9, W=10, padding=1, fwd="g16f", dgrad="g16d", wgrad="g16w")
case("real_generic_f32", "real", B=2, Ci=3, Co=5, H=11, W=13, stride=(2, 3), padding=1, dtype="f32", fwd="genf", dgrad="gend",
     wgrad="genw")
case("real_generic_bf16", "real", B=2, Ci=3, Co=5, H=11, W=13, stride=(2, 3), padding=1, fwd="genf", dgrad="gend", wgrad="g16w")
case("real_generic_bf16_ci200_rounding", "real", B=2, Ci=200, Co=8, H=7, W=8, padding=1, fwd="genf", dgrad="gend",
     wgrad="g16w")

# ---- 9. transposed and 1-d ------------------------------------------------------------------------------------------------------
# (the transposed operator's forward IS the data gradient of the equivalent convolution, its data gradient that
#  convolution's forward; Co = 96 input channels, Ci = 64 output channels)
case("transpose_stride1_rows", "transpose", B=2, Ci=64, Co=96, H=10, W=11, padding=1, rows=True, fwd="rows", dgrad="rows",
     wgrad="rowsw")
# (the bias joins float32 sums: off the shifted-row kernel those come from the gather kernel's float32 store or, where that
#  declines -- K = 100 * 9 is no multiple of 32; stride 2 --, from the float32 kernels on the widened operands)
case("transpose_stride1_gather", "transpose", B=2, Ci=64, Co=96, H=10, W=11, padding=1, fwd="g16d32", dgrad="g16f",
     wgrad="g16w")
case("transpose_stride1_widened", "transpose", B=2, Ci=64, Co=100, H=10, W=11, padding=1, fwd="gend", dgrad="g16f",
     wgrad="g16w")
case("transpose_stride2_outpad_bf16", "transpose", B=2, Ci=32, Co=32, H=14, W=12, stride=2, padding=1, output_padding=1,
     fwd="gend", dgrad="g16f", wgrad="g16w")
case("transpose_stride2_outpad_f32", "transpose", B=2, Ci=32, Co=32, H=14, W=12, stride=2, padding=1, output_padding=1,
     dtype="f32", fwd="gend", dgrad="genf", wgrad="genw")
case("conv1d_k5", "conv1d", B=2, Ci=32, Co=64, H=1, W=50, k=(1, 5), padding=(0, 2), fwd="g16f", dgrad="g16d", wgrad="g16w")


# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switches(c):
    """The dispatcher switches of a case, for the duration of the block (forward AND backward)."""
    from cplxmodule_amd import conv, x3
    old = conv._ROWS_FORCE, conv._CL_FORCE, conv._CL_PATCH
    conv._ROWS_FORCE, conv._CL_FORCE, conv._CL_PATCH = c["rows"], c["cl"], c["patch"]
    try:
        with x3.fp32_mode(c["fp32"]):
            yield
    finally:
        conv._ROWS_FORCE, conv._CL_FORCE, conv._CL_PATCH = old


def geom_of(c):
    from cplxmodule_amd import conv
    xs, ws, _ = shapes(c)
    return conv._geom(xs, ws, c["stride"], c["padding"], c["dilation"], c["groups"])[0]


def is_cplx(c):
    return c["api"] not in ("real", "cl_real")


def out_hw(c):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c["k"], c["stride"], c["padding"], c["dilation"]
    return ((c["H"] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (c["W"] + 2 * pw - dw * (kw - 1) - 1) // sw + 1)


def shapes(c):
    """x (the convolution's input image side), w, g (its output side).  The transposed operator takes the g-shaped tensor
    as its input and returns an x-shaped one; its weight [Co, Ci / groups, KH, KW] has the same shape."""
    Ho, Wo = out_hw(c)
    if c["api"] == "transpose":          # the image must be the one the operator produces from (Ho, Wo)
        (kh, kw), (sh, sw), (ph, pw), (dh, dw), (oh, ow) = c["k"], c["stride"], c["padding"], c["dilation"], c["output_padding"]
        assert c["H"] == (Ho - 1) * sh - 2 * ph + dh * (kh - 1) + oh + 1 and c["W"] == (Wo - 1) * sw - 2 * pw + dw * (kw - 1) + ow + 1
    return ((c["B"], c["Ci"], c["H"], c["W"]), (c["Co"], c["Ci"] // c["groups"]) + c["k"], (c["B"], c["Co"], Ho, Wo))


def terms(c):
    """(forward, data gradient, weight gradient): the number of products summed into one output element."""
    kh, kw = c["k"]
    n = 2 if is_cplx(c) else 1
    Ho, Wo = out_hw(c)
    t_in, t_out = n * (c["Ci"] // c["groups"]) * kh * kw, n * (c["Co"] // c["groups"]) * kh * kw
    if c["api"] == "transpose":
        t_in, t_out = t_out, t_in
    return t_in, t_out, n * c["B"] * Ho * Wo


def magnitude_bound(c):
    """Largest magnitude any partial sum can reach: |x w| <= 6 per product (+ a bias of at most 8) for the forward and the
    data gradient, |g x| <= 9 for the weight gradient, 3 per pixel for the bias gradient."""
    tf, td, tw = terms(c)
    return max(tf * 6 + 8, td * 6 + 8, tw * 9)


def make_inputs(c):
    """float64 numpy operands (integer-valued; biases half-integers), planar, seeded by the case name."""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7fffffff)
    xs, ws, gs = shapes(c)
    ints = lambda lo, hi, s: rs.randint(lo, hi + 1, size=s).astype(np.float64)  # noqa: E731
    d = {}
    planes = ("r", "i") if is_cplx(c) else ("",)
    for p in planes:
        d["x" + p], d["w" + p], d["g" + p] = ints(-3, 3, xs), ints(-2, 2, ws), ints(-3, 3, gs)
        nb = c["Ci"] if c["api"] == "transpose" else c["Co"]
        d["b" + p] = ints(-16, 16, (nb,)) / 2
    if c["api"] == "cl_real":
        d["emul"] = 2.0 ** ints(-3, 3, ws)
    return d


def _kw(c):
    return dict(stride=c["stride"], padding=c["padding"], dilation=c["dilation"], groups=c["groups"])


def _torch_reference(c, d):
    kw = _kw(c)
    if c["api"] == "transpose":
        kw["output_padding"] = c["output_padding"]
        op, xin, gout = F.conv_transpose2d, "g", "x"      # the operator's input is g-shaped, its output gradient x-shaped
    else:
        op, xin, gout = F.conv2d, "x", "g"
    t = {k: torch.tensor(v).requires_grad_(k[0] in xin + "wb") for k, v in d.items() if k != "emul"}
    if is_cplx(c):
        a, b, wr, wi = t[xin + "r"], t[xin + "i"], t["wr"], t["wi"]
        yr = op(a, wr, **kw) - op(b, wi, **kw) + t["br"].view(1, -1, 1, 1)
        yi = op(a, wi, **kw) + op(b, wr, **kw) + t["bi"].view(1, -1, 1, 1)
        torch.autograd.backward((yr, yi), (t[gout + "r"], t[gout + "i"]))
        out = dict(yr=yr, yi=yi, dxr=a.grad, dxi=b.grad, dwr=wr.grad, dwi=wi.grad, dbr=t["br"].grad, dbi=t["bi"].grad)
    else:
        y = op(t["x"], t["w"], **kw) + t["b"].view(1, -1, 1, 1)
        y.backward(t["g"])
        out = dict(y=y, dx=t["x"].grad, dw=t["w"].grad, db=t["b"].grad)
    return {k: v.detach().numpy() for k, v in out.items()}


def _oracle_reference(c, d):
    from oracle import cplx_oracle as orc
    kw = _kw(c)
    if c["api"] == "transpose":
        kw["output_padding"] = c["output_padding"]
        yr, yi = orc.cplx_conv_transpose2d(d["gr"], d["gi"], d["wr"], d["wi"], d["br"], d["bi"], **kw)
        bw = orc.cplx_conv_transpose2d_bwd(d["xr"], d["xi"], d["gr"], d["gi"], d["wr"], d["wi"], **kw)
        return dict(yr=yr, yi=yi, **bw)
    if is_cplx(c):
        yr, yi = orc.cplx_conv2d(d["xr"], d["xi"], d["wr"], d["wi"], d["br"], d["bi"], **kw)
        bw = orc.cplx_conv2d_bwd(d["gr"], d["gi"], d["xr"], d["xi"], d["wr"], d["wi"], **kw)
        return dict(yr=yr, yi=yi, **bw)
    y = orc.real_conv2d(d["x"], d["w"], **kw) + d["b"][None, :, None, None]
    dx, dw = orc.real_conv2d_bwd(d["g"], d["x"], d["w"], **kw)
    return dict(y=y, dx=dx, dw=dw, db=d["g"].sum((0, 2, 3)))


ORACLE_MAX_MACS = 3e7         # the numpy oracle (im2col + einsum) takes a fraction of a second below this


def macs(c):
    Ho, Wo = out_hw(c)
    kh, kw = c["k"]
    return (4 if is_cplx(c) else 1) * c["B"] * Ho * Wo * c["Co"] * (c["Ci"] // c["groups"]) * kh * kw


def uses_oracle(c):
    return macs(c) <= ORACLE_MAX_MACS


_cache = {}


def reference(c):
    """-> (inputs, exact float64 results): y, dx, dw, db (real) or yr, yi, dxr, dxi, dwr, dwi, dbr, dbi.  For the
    transposed operator 'y' is x-shaped and 'dx' g-shaped.  The numpy oracle where it is quick, torch's float64 CPU
    convolution otherwise (test_conv_exact_host.py shows the two identical on such data).  Cached per case: the planar and
    the channels-last variant of a case share it, and nobody writes to it."""
    hit = _cache.get(c["name"])
    if hit is None:
        d = make_inputs(c)
        ref = _oracle_reference(c, d) if uses_oracle(c) else _torch_reference(c, d)
        for v in list(d.values()) + list(ref.values()):
            v.setflags(write=False)
        hit = _cache[c["name"]] = (d, ref)
    return hit


def expected(ref, dtype):
    """What a kernel must return for the exact value `ref`: the value itself in float32, its one round-to-nearest-even in bf16."""
    t = torch.tensor(np.ascontiguousarray(ref), dtype=torch.float32)
    assert np.array_equal(t.double().numpy(), ref), "the reference is not exactly representable in float32"
    return (t.bfloat16().float() if dtype == "bf16" else t).numpy()


def rounding_content(ref):
    """(fraction of values one bf16 rounding changes, number of exact ties among them)."""
    t = torch.tensor(np.ascontiguousarray(ref), dtype=torch.float32)
    bits = t.view(torch.int32)
    low = bits & 0xffff
    changed = float((low != 0).float().mean())
    ties = int((low == 0x8000).sum())
    return changed, ties


def emulate_x2_split(a):
    """numpy emulation of x3.split_planes(kind='x2') (csrc/split.hip): scale s = 2^(15 - e) with max|a| = f 2^e, f in [0.5, 1);
    first piece = half(a s), second piece = half(a s - first).  -> (s, first, second) as float64."""
    m = float(np.abs(a).max())
    s = 1.0 if m == 0 else 2.0 ** (15 - np.frexp(np.float32(m))[1])
    xs = (a.astype(np.float32) * np.float32(s)).astype(np.float32)
    p0 = xs.astype(np.float16)
    p1 = (xs - p0.astype(np.float32)).astype(np.float16)
    return s, p0.astype(np.float64), p1.astype(np.float64)


# ---- mismatch reports that name the seam ----------------------------------------------------------------------------------------
def _seams(c, which, idx, shape):
    """Words for one mismatching coordinate of an image-shaped result [B, C, H, W]."""
    b, ch, h, w = idx
    _, C, H, W = shape
    out = []
    if h in (0, H - 1) or w in (0, W - 1):
        out.append("image border")
    route = c["dgrad"] if which.startswith("dx") else c["fwd"]
    p = (b * H + h) * W + w
    pg = (b * c["H"] + h) * c["W"] + w       # conv_cl.hip, complex and real, walks the LARGER image's grid (the convolution's input)
    if route in ("cl2", "x2"):
        if h % CL2_TH in (0, CL2_TH - 1) or w % CL2_TW in (0, CL2_TW - 1):
            out.append(f"tile border (16 x 32 tile {h // CL2_TH},{w // CL2_TW})")
    elif route in ("cl", "clr"):
        tm = CL_TM - (c["k"][1] - 1) * c["dilation"][1]
        if pg % tm in (0, tm - 1):
            out.append(f"tile border (row tile {pg // tm} of {tm} pixels)")
    elif route in ("rows", "rows32"):
        Hp, Wp = c["H"] + 2 * c["padding"][0], c["W"] + 2 * c["padding"][1]
        off = (0, 0) if which.startswith("y") else c["padding"]
        r = (b * Hp + h + off[0]) * Wp + w + off[1]
        if r % ROWS_BM in (0, ROWS_BM - 1):
            out.append(f"tile border (grid row {r}, 256-row tile {r // ROWS_BM})")
    elif route in ("g16f", "g16d"):
        if p % GATHER_BN in (0, GATHER_BN - 1):
            out.append(f"tile border (pixel {p}, 64-pixel tile {p // GATHER_BN})")
    if C % 64 and ch >= C - C % 64:
        out.append("channel-tile tail")
    out.append(f"16-channel slice {ch // 16}")
    return ", ".join(out)


def describe_mismatch(got, ref, c=None, which="y", limit=6):
    """'' if got == ref everywhere (by value, so +0 == -0), else the count and the first few coordinates with the seam each
    lies on (image border, tile border of the route's tiling, channel-tile tail)."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"{which}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(~(got == ref))
    if bad.size == 0:
        return ""
    lines = [f"{which}: {len(bad)} of {ref.size} values differ (shape {ref.shape})"]
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        where = ""
        if c is not None and ref.ndim == 4 and (which[0] == "y" or which.startswith("dx")):
            where = "  [" + _seams(c, which, idx, ref.shape) + "]"
        elif ref.ndim == 4:                      # a weight gradient [Co, Ci / g, KH, KW]
            tail = [n for n, C_, i in (("Co", ref.shape[0], idx[0]), ("Ci", ref.shape[1], idx[1])) if C_ % 64 and i >= C_ - C_ % 64]
            where = f"  [tap {idx[2]},{idx[3]}" + "".join(f", {n} channel-tile tail" for n in tail) + "]"
        lines.append(f"  {idx}: got {got[idx]!r}, want {ref[idx]!r}{where}")
    return "\n".join(lines)
