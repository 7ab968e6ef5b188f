"""Ill-conditioned inputs for the complex batch-norm kernels: one table for scripts/gen_bn_stress_golden.py (which records
the reference's own float32 error on them), tests/test_bn_stress_host.py and tests/test_gpu_bn_stress.py.

Conditions vary PER FEATURE, so one tensor is a sweep: feature f of a case takes condition (f + offset) mod len(tier).
A condition is (ratio, kind, scale):
  ratio  mean / std of the real part (the imaginary part gets -ratio / 2)
  kind   "r0" / "r9" / "r999": correlation 0 / 0.9 / 0.999 between the parts; "lin": xi = -0.5 xr exactly (the batch
         covariance is singular, eps alone keeps it invertible); "im0": xi == 0; "const": both parts constant
  scale  multiplies the whole feature
Everything is numpy from fixed seeds (RandomState: the same stream on every machine); no torch, no GPU.

Which conditions are in which tier follows from the cap tests/test_bn_stress_host.py sets on the REFERENCE's float32
error (4 e_ref <= 1e-2): a tolerance above that would make the GPU assertion vacuous.  What had to move, with the
reference's measured float32 error (scripts/gen_bn_stress_golden.py -v on probe conditions):
  * "lin" at scale 1 (variance ~2): the determinant is eps (a + d) ~ 1e-5 a d and the reference forms a d - b b in float32;
    its dX is off by 3e-4 ... 3e-3 depending on the count, 4 x that is at or past the cap; at scale 1e3 its float32
    determinant is noise of either sign and the outputs are NaN.  Kept: "lin" at scale 0.3 and 0.1 (det / (a d) = 2.5e-4,
    reference 5e-5 ... 2e-4) and at 1e-3, 1e-6 where eps carries the determinant.
  * the position counts 1, 2, 3 (two points are always perfectly correlated: every feature is a "lin" one) only at scales
    1e-6 and 1e-3, for the same reason: at scale 1 the reference's dX is 3e-3 off with two positions.
  * ratio 1000 not together with correlation 0.999: the reference is 4e-4 ... 7e-3 off in y and 3e-3 in dweight (its
    float32 mean is off by ~1e-7 * 1000 std, and the whitening of a 0.999-correlated pair stretches the small axis by
    ~30).  Ratio 1000 is kept with correlation <= 0.9, correlation 0.999 with ratio <= 100.
"""
from collections import namedtuple

import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
SCALES = (1e-6, 1e-3, 1.0, 1e3, 1e6)
LIN_C = -0.5

Cond = namedtuple("Cond", "ratio kind scale")


def _tier_mild():
    out = [Cond(r, k, s) for r in (0, 10) for k in ("r0", "r9") for s in SCALES]
    out += [Cond(r, "lin", s) for r in (0, 10) for s in (1e-6, 1e-3)]
    out += [Cond((0, 10)[j & 1], "im0", s) for j, s in enumerate(SCALES)]
    out += [Cond(0, "const", 1e-3), Cond(0, "const", 1.0), Cond(0, "const", 1e3)]
    return out


def _tier_hard():
    out = [Cond(r, k, s) for r in (100, 1000) for k in ("r0", "r9") for s in SCALES]
    out += [Cond(r, "r999", s) for r in (0, 10, 100) for s in SCALES]
    out += [Cond(0, "lin", 0.3), Cond(10, "lin", 0.3), Cond(100, "lin", 0.1), Cond(100, "lin", 1e-3)]
    out += [Cond(100, "im0", 1.0), Cond(1000, "im0", 1e3)]
    return out


def _tier_tiny():
    """Position counts 1, 2, 3: every kind, at the scales where eps carries the determinant (module docstring)."""
    return [Cond(r, k, s) for s in (1e-6, 1e-3) for r in (0, 10) for k in ("r0", "r9", "r999", "lin", "im0", "const")]


def _tier_bf16():
    out = [Cond(r, k, s) for r in (0, 2, 8, 32) for k in ("r0", "r9", "r999") for s in (1e-3, 1.0, 1e3)]
    out += [Cond(8, "lin", 1e-3), Cond(2, "im0", 1.0), Cond(0, "const", 1.0), Cond(32, "im0", 1e6), Cond(0, "r9", 1e-6)]
    return out


TIERS = {"mild": _tier_mild(), "hard": _tier_hard(), "tiny": _tier_tiny(), "bf16": _tier_bf16()}

# name, shape [B, F, *spatial], dtype, channels_last, tier, offset into the tier, store64 (the float64 reference results
# go into the fixture: small cases only), route the case is there for
Case = namedtuple("Case", "name shape dtype cl tier offset store64 route")

CASES = [
    # ---- float32, against the float64 oracle with the reference's own float32 error as the margin
    Case("host_mild", (40, 60), "f32", False, "mild", 0, True, "cols"),
    Case("host_hard", (64, 36), "f32", False, "hard", 0, True, "cols"),
    Case("cols_mild", (257, 60), "f32", False, "mild", 7, False, "cols, F % 64 != 0"),
    Case("cols_hard", (1024, 44), "f32", False, "hard", 0, False, "cols, several chunks"),
    Case("small_mild", (6, 34, 7, 9), "f32", False, "mild", 0, False, "small planes, scalar apply (S = 63)"),
    Case("small_hard", (16, 44, 12, 12), "f32", False, "hard", 0, False, "small planes, vector apply (S = 144)"),
    Case("large_mild", (2, 17, 40, 40), "f32", False, "mild", 3, False, "large planes, vector path (S = 1600)"),
    Case("large_hard", (3, 11, 33, 37), "f32", False, "hard", 20, False, "large planes, scalar path (S = 1221)"),
    Case("large_hard_seg", (1, 5, 128, 130), "f32", False, "hard", 25, False, "large planes cut into segments"),
    Case("rows_mild", (2, 40, 48, 48), "f32", True, "mild", 0, False, "channels-last rows, F % 64 != 0"),
    Case("rows_hard", (3, 48, 40, 40), "f32", True, "hard", 0, False, "channels-last rows"),
    Case("clcols_hard", (2, 12, 10, 9), "f32", True, "hard", 18, True, "channels-last, F % 8 != 0: cols"),
    # ---- position counts 1, 2, 3
    Case("count1", (1, 24), "f32", False, "tiny", 0, True, "cols, B S = 1"),
    Case("count2", (2, 24), "f32", False, "tiny", 0, True, "cols, B S = 2"),
    Case("count3", (3, 24), "f32", False, "tiny", 0, True, "cols, B S = 3"),
    Case("count2_planes", (1, 24, 2), "f32", False, "tiny", 5, True, "small planes, B S = 2"),
    Case("count3_planes", (1, 24, 1, 3), "f32", False, "tiny", 11, True, "small planes, B S = 3"),
    # ---- bf16 planes: the oracle on the bf16-rounded values, the bars of test_batchnorm_channels_last_rows_kernels
    Case("rows_bf16", (2, 64, 64, 40), "bf16", True, "bf16", 0, False, "channels-last rows, bf16"),
    Case("small_bf16", (4, 41, 16, 16), "bf16", False, "bf16", 0, False, "small planes, bf16"),
    Case("large_bf16", (2, 9, 36, 35), "bf16", False, "bf16", 4, False, "large planes, scalar path, bf16"),
    Case("cols_bf16", (300, 41), "bf16", False, "bf16", 0, False, "cols, bf16"),
]
BY_NAME = {c.name: c for c in CASES}
F32_CASES = [c.name for c in CASES if c.dtype == "f32"]
BF16_CASES = [c.name for c in CASES if c.dtype == "bf16"]
COUNT_CASES = [c.name for c in CASES if c.tier == "tiny"]
STORED_CASES = [c.name for c in CASES if c.store64]
QUANTITIES = ("y", "dx", "dweight", "dbias", "running_mean", "running_var")
EVAL_QUANTITIES = ("y", "dx", "dweight", "dbias")


def conditions(case):
    tier = TIERS[case.tier]
    return [tier[(f + case.offset) % len(tier)] for f in range(case.shape[1])]


def bf16_round(a):
    """float32 -> the nearest bfloat16 value (ties to even), as float32; finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _seed(case):
    return 20261016 + 97 * [c.name for c in CASES].index(case.name)


def features(conds, n, rs, dtype="f32"):
    """-> xr, xi [n, F] float32 (bf16-representable for dtype "bf16")."""
    F = len(conds)
    xr, xi = np.empty((n, F), np.float32), np.empty((n, F), np.float32)
    for f, c in enumerate(conds):
        z1, z2 = rs.randn(n), rs.randn(n)
        rho = {"r0": 0.0, "r9": 0.9, "r999": 0.999}.get(c.kind, 0.0)
        u = 1.5 * (z1 + c.ratio)
        v = 0.8 * (rho * z1 + np.sqrt(1.0 - rho * rho) * z2 - 0.5 * c.ratio)
        if c.kind == "const":
            u, v = np.full(n, 1.25), np.full(n, -0.75)
        u, v = (c.scale * u).astype(np.float32), (c.scale * v).astype(np.float32)
        if dtype == "bf16":
            u, v = bf16_round(u), bf16_round(v)
        if c.kind == "lin":
            v = np.float32(LIN_C) * u                    # exact: a power of two
        if c.kind == "im0":
            v = np.zeros(n, np.float32)
        xr[:, f], xi[:, f] = u, v
    return xr, xi


def _to_shape(a, shape):
    """[n, F] -> [B, F, *spatial] (position index = (b, spatial) in C order)."""
    B, F = shape[0], shape[1]
    sp = shape[2:]
    a = a.reshape((B,) + tuple(sp) + (F,))
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))


def build(case):
    """-> dict of float32 arrays: xr, xi, gr, gi [B, F, ...]; weight [2, 2, F], bias [2, F]; running_mean [2, F] and
    running_var [2, 2, F] for the evaluation-mode run: the batch's own mean and (near-singular) covariance + eps on the
    diagonal, rounded to float32."""
    if isinstance(case, str):
        case = BY_NAME[case]
    rs = np.random.RandomState(_seed(case))
    shape = case.shape
    F = shape[1]
    n = int(np.prod(shape)) // F
    conds = conditions(case)
    xr, xi = features(conds, n, rs, case.dtype)
    gr, gi = rs.randn(n, F).astype(np.float32), rs.randn(n, F).astype(np.float32)
    if case.dtype == "bf16":
        gr, gi = bf16_round(gr), bf16_round(gi)
    W = (np.eye(2)[:, :, None] + 0.2 * rs.randn(2, 2, F)).astype(np.float32)
    b = (0.3 * rs.randn(2, F)).astype(np.float32)
    u, v = xr.astype(np.float64), xi.astype(np.float64)
    mu, mv = u.mean(0), v.mean(0)
    cu, cv = u - mu, v - mv
    a, d, c = (cu * cu).mean(0) + EPS, (cv * cv).mean(0) + EPS, (cu * cv).mean(0)
    return dict(xr=_to_shape(xr, shape), xi=_to_shape(xi, shape), gr=_to_shape(gr, shape), gi=_to_shape(gi, shape),
                weight=W, bias=b, running_mean=np.stack([mu, mv]).astype(np.float32),
                running_var=np.stack([a, c, c, d]).reshape(2, 2, F).astype(np.float32), conds=conds)


def rel_per_feature(got, ref, floor=None):
    """-> [F]: ||got_f - ref_f|| / ||ref_f|| for arrays whose feature axis is 1 ([B, F, ...] planes, [k, F] parameters).
    Where the reference vanishes IDENTICALLY (floors() says where that happens) the error is taken against floor[f], the
    size of the terms that cancel; without a floor: 0 where both vanish, inf where only the reference does."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ax = (0,) + tuple(range(2, ref.ndim))
    num, den = np.sqrt(((got - ref) ** 2).sum(ax)), np.sqrt((ref ** 2).sum(ax))
    if floor is not None:
        den = np.where(den > 0, den, floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / den
    r = np.where((den == 0) & (num == 0), 0.0, r)
    return np.where((den == 0) & (num != 0), np.inf, r)


def floors(d):
    """Two quantities are exactly zero in exact arithmetic for some features, and a relative error against them says
    nothing: dx of a feature with ONE position (x - mean = 0: dx = E g - E g) and dweight of a constant feature (the
    whitened value is 0).  Their errors are measured against the size of what cancels instead: ||E g|| (E the whitening
    times the affine matrix, i.e. the evaluation-mode gradient at the batch statistics) and ||g|| sqrt(count) (the
    whitened values of an ordinary feature have unit variance).  Used ONLY where the reference norm is exactly 0."""
    gr, gi = d["gr"].astype(np.float64), d["gi"].astype(np.float64)
    F = gr.shape[1]
    n = gr.size // F
    ax = (0,) + tuple(range(2, gr.ndim))
    shp = (1, F) + (1,) * (gr.ndim - 2)
    a, b, _, dd = d["running_var"].astype(np.float64).reshape(4, F)
    s = np.sqrt(a * dd - b * b)
    t = s * np.sqrt(a + dd + 2 * s)
    p, q, w = ((dd + s) / t).reshape(shp), (-b / t).reshape(shp), ((a + s) / t).reshape(shp)
    W = d["weight"].astype(np.float64).reshape(2, 2, *shp)
    gzu, gzv = gr * W[0, 0] + gi * W[1, 0], gr * W[0, 1] + gi * W[1, 1]
    eg = np.sqrt(((gzu * p + gzv * q) ** 2 + (gzu * q + gzv * w) ** 2).sum(ax))
    return {"dx": eg, "dweight": np.sqrt((gr * gr + gi * gi).sum(ax) * n)}


def stack_planes(re, im):
    """Both planes of a complex quantity as one array [2 B, F, ...]: the per-feature norm runs over both."""
    return np.concatenate([np.asarray(re, np.float64), np.asarray(im, np.float64)], axis=0)


def as_feature_rows(name, value):
    """A result of QUANTITIES as an array with the feature axis at 1 (parameters [.., F] -> [k, F])."""
    v = np.asarray(value, np.float64)
    if name in ("dweight", "running_var"):
        return v.reshape(4, -1)
    if name in ("dbias", "running_mean"):
        return v.reshape(2, -1)
    return v


def oracle_results(orc, d, dtype=np.float64, training=True):
    """The project's numpy oracle on a built case -> dict over QUANTITIES (y, dx as stacked planes)."""
    f = dtype
    xr, xi, gr, gi = (d[k].astype(f) for k in ("xr", "xi", "gr", "gi"))
    W, b = d["weight"].astype(f), d["bias"].astype(f)
    F = W.shape[-1]
    out = {}
    if training:
        rm = np.zeros((2, F), f)
        rv = np.stack([np.ones(F), np.zeros(F), np.zeros(F), np.ones(F)]).reshape(2, 2, F).astype(f)
    else:
        rm, rv = d["running_mean"].astype(f), d["running_var"].astype(f)
    yr, yi = orc.cplx_batch_norm(xr, xi, rm, rv, W, b, training, MOMENTUM, EPS)
    bw = orc.cplx_batch_norm_bwd(gr, gi, xr, xi, rm, rv, W, training, EPS)
    out["y"], out["dx"] = stack_planes(yr, yi), stack_planes(bw["dxr"], bw["dxi"])
    out["dweight"], out["dbias"] = bw["dweight"], bw["dbias"]
    if training:
        out["running_mean"], out["running_var"] = rm, rv
    return out
