"""Case tables and references of the elementwise sweep (tests/test_elementwise_host.py, tests/test_gpu_elementwise_sweep.py):
numpy and torch on the CPU, fixed seeds, no GPU.

A. value seams of csrc/cplxfn.hip: families of (s, t) points, s the coordinate that feeds chsh / the tanh saturation (Re z
   for exp, log, sinh, cosh, tanh; Im z for sin, cos, tan) and t the other one (the trigonometric argument); the complex128
   reference; the bounds; a float32 numpy restatement of the file's formulas (written from its header) that the host test
   holds against the same bounds, so the bounds are known to be attainable before a kernel runs.
B. index space of the streaming kernels: sizes around the vector body / tail / grid wrap, edge-value tables, float32
   chains of the ops whose kernels document the reference's operation order.
D. abs-max pooling: Gaussian-integer planes with exact ties, the configuration product, the torch CPU reference.
u = 2^-24 throughout."""
import itertools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cplxmodule_amd", "csrc")

U = 2.0 ** -24
LO, HI = 2.0 ** -100, 2.0 ** 127        # the mask: a modulus (or part) outside is neither asserted nor counted as kept
FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")
PRODUCT_FORM = ("exp", "sin", "cos", "sinh", "cosh")    # each part = two factors taken at exactly-given arguments
S_IS_IM = ("sin", "cos", "tan")
F32 = np.float32


# ---- source constants -------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


GRID_CAP = _const(_src("common.h"), r"if \(g > (\d+)\) g = \1;")            # common.h stream_grid: blocks per launch
BLOCK = {"cplxfn": _const(_src("cplxfn.hip"), r"constexpr int kFT = (\d+);"),    # threads per block of each file's kernels
         "layout": _const(_src("layout.hip"), r"constexpr int kLT = (\d+);"),
         "util": _const(_src("util.hip"), r"constexpr int kUT = (\d+);")}


def vec(group, dtype):
    """elements per lane and grid-stride trip: cplxfn.hip moves one 16-byte vector of T (v16<T>::N = 16 / sizeof(T)), layout.hip
    and util.hip four elements whatever the dtype (n >> 2, ld4 / st4)"""
    return 16 // (2 if dtype == torch.bfloat16 else 4) if group == "cplxfn" else 4


def wrap_length(group, dtype):
    """L: the number of elements past which the grid-stride loop makes a second trip = GRID_CAP blocks x BLOCK threads x V"""
    return GRID_CAP * BLOCK[group] * vec(group, dtype)


def sizes(group, dtype):
    L, V = wrap_length(group, dtype), vec(group, dtype)
    return (0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 1027, L - 1, L + V + 3)


SMALL_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 1027)
PERIOD = 1027                            # the large sizes repeat a 1027-element pattern (odd: no multiple of a vector)
ROLLS = (1, 2, 3, 5)


# ---- A: families ------------------------------------------------------------------------------------------------------
def _neighbours(x, k):
    """x and its k float32 neighbours on each side"""
    out, lo, hi = [F32(x)], F32(x), F32(x)
    for _ in range(k):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.array(out, F32)


def _sign(rs, n):
    return np.where(rs.rand(n) < 0.5, -1.0, 1.0)


def _loguniform(rs, lo, hi, n):
    return np.exp(rs.uniform(np.log(lo), np.log(hi), n))


def _family_st(name):
    rs = np.random.RandomState({"seam11": 11, "seam88": 88, "part_overflow": 89, "tiny": 3, "halfpi": 5, "bigtrig": 7,
                                "gauss": 2, "unit": 1}[name])
    if name == "seam11":
        s = np.concatenate([_neighbours(11.0, 4), _neighbours(-11.0, 4)]).repeat(64)
        return s, 3 * rs.randn(s.size)
    if name == "seam88":
        s = np.concatenate([_neighbours(88.0, 4), _neighbours(-88.0, 4)]).repeat(32)
        band = _sign(rs, 1024) * (88.72 - (88.72 - 85.0) * rs.rand(1024))          # |s| in (85, 88.72]
        s = np.concatenate([s, band])
        return s, 3 * rs.randn(s.size)
    if name == "part_overflow":
        k = np.arange(-4, 5).repeat(256)
        s = _sign(rs, k.size) * rs.uniform(88.72, 104.0, k.size)
        s = np.where(np.abs(s) <= 88.72, np.sign(s) * 88.73, s)
        return s, (k * (np.pi / 2)).astype(F32).astype(np.float64) + rs.uniform(-1e-3, 1e-3, k.size)
    if name == "tiny":
        s = np.concatenate([_sign(rs, 1022) * _loguniform(rs, 1e-30, 1e-3, 1022), [1e-40, -1e-40]])
        t = 3 * rs.randn(1024)
        both = _sign(rs, 512) * _loguniform(rs, 1e-30, 1e-3, 512)
        return np.concatenate([s, both]), np.concatenate([t, _sign(rs, 512) * _loguniform(rs, 1e-30, 1e-3, 512)])
    if name == "halfpi":
        t = np.concatenate([_neighbours(F32(k * (np.pi / 2)), 2) for k in range(-8, 9)])
        tg, tt = t.repeat(16), t.repeat(8)
        return (np.concatenate([2 * rs.randn(tg.size), _sign(rs, tt.size) * _loguniform(rs, 1e-30, 1e-3, tt.size)]),
                np.concatenate([tg, tt]))
    if name == "bigtrig":
        return 2 * rs.randn(1024), _sign(rs, 1024) * _loguniform(rs, 1e2, 1e30, 1024)
    if name == "gauss":
        return 2 * rs.randn(2048), 2 * rs.randn(2048)
    raise KeyError(name)


FAMILIES = ("seam11", "seam88", "part_overflow", "tiny", "halfpi", "bigtrig", "gauss")


def families(fn):
    return FAMILIES + (("unit",) if fn == "log" else ())


_POINTS = {}


def points(fn, name, dtype=torch.float32):
    """(zr, zi, gr, gi) CPU tensors of `dtype` (float32 values rounded to it), computed once.  g: standard Gaussian."""
    key = (fn in S_IS_IM, fn == "exp" and name == "part_overflow", name, dtype)
    if key not in _POINTS:
        if name == "unit":                  # |z| = 1 (rounded), and the negative real axis with Im z = +-0.0
            rs = np.random.RandomState(1)
            th = rs.uniform(-np.pi, np.pi, 1024)
            x = np.concatenate([np.cos(th), -_loguniform(rs, 1e-3, 1e3, 64), -_loguniform(rs, 1e-3, 1e3, 64)])
            y = np.concatenate([np.sin(th), np.zeros(64), -np.zeros(64)])
        else:
            s, t = _family_st(name)
            if key[1]:
                s = np.abs(s)                # e^s with s < -88.72 is subnormal: nothing to assert on that half
            x, y = (t, s) if fn in S_IS_IM else (s, t)
        rs = np.random.RandomState(1000 + len(name))
        f = lambda a: torch.from_numpy(np.asarray(a, np.float64).astype(F32)).to(dtype)  # noqa: E731
        _POINTS[key] = (f(x), f(y), f(rs.randn(len(x))), f(rs.randn(len(x))))
    return _POINTS[key]


# ---- A: reference and bounds ------------------------------------------------------------------------------------------
def for_autograd(fn, z):
    """f(z) in a spelling whose complex128 autograd does not cancel (tests/test_gpu_cplx_fn.py::_for_autograd): torch's
    tanh / tan backward forms 1 - tanh^2, which is 0 in float64 once |s| passes ~19 while |f'| ~ 4 e^{-2|s|} is not."""
    if fn == "tanh":
        return 1 - 2 / (torch.exp(2 * z) + 1)
    if fn == "tan":
        return -1j * (1 - 2 / (torch.exp(2j * z) + 1))
    return getattr(torch, fn)(z)


def deriv(fn, z):
    """f'(z) in complex128, cancellation-free: sech^2 z = 4 e^{-2z} / (1 + e^{-2z})^2 on the side where e^{-2z} is small"""
    if fn in ("tan", "tanh"):
        w = z if fn == "tanh" else 1j * z                 # sec^2 z = sech^2(iz)
        w = torch.where(w.real < 0, -w, w)                # sech^2 is even
        e = torch.exp(-2 * w)
        return 4 * e / (1 + e) ** 2
    return {"exp": torch.exp, "log": lambda z: 1 / z, "sin": torch.cos, "cos": lambda z: -torch.sin(z),
            "sinh": torch.cosh, "cosh": torch.sinh}[fn](z)


_REF = {}


def reference(fn, name, dtype=torch.float32):
    """dict: f (complex128 forward), d (the backward conj(f') g as complex128), scale (|f'| |g|), of the float64 of the
    values the kernel is given.  Computed once per (fn, family, dtype)."""
    key = (fn, name, dtype)
    if key not in _REF:
        zr, zi, gr, gi = (t.double() for t in points(fn, name, dtype))
        z = torch.complex(zr, zi)
        f = getattr(torch, fn)(z)
        g = torch.complex(gr, gi)
        d = deriv(fn, z)
        _REF[key] = dict(f=f.numpy(), d=(d.conj() * g).numpy(), scale=(d.abs() * g.abs()).numpy())
    return _REF[key]


def autograd_backward(fn, name, dtype=torch.float32):
    """the backward through complex128 autograd of for_autograd, as a cross-check of reference()['d']"""
    zr, zi, gr, gi = (t.double() for t in points(fn, name, dtype))
    zr, zi = zr.requires_grad_(True), zi.requires_grad_(True)
    w = for_autograd(fn, torch.complex(zr, zi))
    rr, ri = torch.autograd.grad((w.real * gr).sum() + (w.imag * gi).sum(), (zr, zi))
    return (rr + 1j * ri).numpy()


def _in_mask(a):
    a = np.abs(a)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (a > LO) & (a < HI)


def _mean(mask):
    return float(mask.mean()) if mask.size else 1.0


def forward_ratios(fn, dtype, got_re, got_im, ref):
    """(worst modulus-wise error / bound, worst per-part error / bound or None, kept fraction, kept fraction of parts).
    Modulus-wise: 16 u |ref| (float32; log also passes with |d re| <= 4 u and |d im| <= 16 u |ref|, the existing test's
    clause for the cancelling log a + log1p(.) / 2 near |z| = 1), 2^-8 |ref| (bf16), where LO < |ref| < HI.  Per part, for
    the product-form functions: 16 u |ref part| (float32), 2^-8 |ref part| (bf16: the one rounding on store is below 2^-8 / (1 + 2^-8) of
    the part, which leaves 1.5e-5 of it, 250 u, for the float32 arithmetic before), where LO < |ref part| < HI; a part that is not finite there has ratio inf."""
    got_re, got_im = np.asarray(got_re, np.float64), np.asarray(got_im, np.float64)
    rel = 16 * U if dtype == torch.float32 else 2.0 ** -8
    keep = _in_mask(ref)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((got_re - ref.real) + 1j * (got_im - ref.imag))
        ratio = err / (rel * np.abs(ref))
        if fn == "log" and dtype == torch.float32:
            alt = np.maximum(np.abs(got_re - ref.real) / (4 * U), np.abs(got_im - ref.imag) / (rel * np.abs(ref)))
            ratio = np.minimum(ratio, alt)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio[keep].max()) if keep.any() else 0.0
    part, pkeep = None, 0.0
    if fn in PRODUCT_FORM:
        pk = np.stack([_in_mask(ref.real), _in_mask(ref.imag)])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            pr = np.stack([np.abs(got_re - ref.real) / (rel * np.abs(ref.real)),
                           np.abs(got_im - ref.imag) / (rel * np.abs(ref.imag))])
        pr = np.where(np.isnan(pr), np.inf, pr)
        part, pkeep = (float(pr[pk].max()) if pk.any() else 0.0), _mean(pk)
    return worst, part, _mean(keep), pkeep


def backward_ratios(dtype, got_re, got_im, r):
    """(worst error / bound, kept fraction, small): 32 u |f'| |g| (float32), 2^-7 |f'| |g| (bf16), where LO < |f'| |g| < HI;
    small: every result whose |f'| |g| <= LO is at most 2 LO in modulus"""
    rel = 32 * U if dtype == torch.float32 else 2.0 ** -7
    keep = _in_mask(r["scale"]) & np.isfinite(r["d"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ratio = np.abs((np.asarray(got_re, np.float64) - r["d"].real) + 1j * (np.asarray(got_im, np.float64) - r["d"].imag)) \
            / (rel * r["scale"])
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    low = np.isfinite(r["scale"]) & (r["scale"] <= LO)       # below the mask: nothing to compare, but the result is that small
    small = bool(np.all(np.hypot(np.asarray(got_re, np.float64), np.asarray(got_im, np.float64))[low] <= 2 * LO))
    return (float(ratio[keep].max()) if keep.any() else 0.0), _mean(keep), small


# Kept fractions that the reference alone guarantees (test_elementwise_host.py checks them, the GPU test asserts them again
# on what it compared): 0.9, except where the true value leaves (LO, HI) on part of a family by construction.
#   forward, exp / seam88: e^-88 = 6e-39 < LO on the negative half, e^s > HI = e^88.03 on a fifth of the positive band
#   forward, product forms / part_overflow: |f| >= e^88.72 / 2 > HI everywhere; the family is judged per part, and counted
#     by the points that have a representable part: >= 0.4 (float32: 0.47 ... 0.53; bf16, whose rounding moves t off
#     k pi / 2 by up to 0.004: 0.40 ... 0.44, floor 0.35)
#   backward, exp / seam88: as forward, times |g|;  other product forms / seam88: |f'| |g| > HI where |g| > 1 near the top
#   backward, tan and tanh / seam88: |f'| = 4 e^{-2|s|} < 1e-73 < LO: nothing to compare (the result must be that small)
KEEP_MIN = 0.9
_PF = ("sin", "cos", "sinh", "cosh")
KEEP_MIN_FWD = {("exp", "seam88"): 0.35, **{(f, "part_overflow"): 0.0 for f in PRODUCT_FORM}}
KEEP_MIN_BWD = {("exp", "seam88"): 0.25, **{(f, "seam88"): 0.85 for f in _PF}, ("tan", "seam88"): 0.0, ("tanh", "seam88"): 0.0}


def keep_min(fn, name, backward=False):
    return (KEEP_MIN_BWD if backward else KEEP_MIN_FWD).get((fn, name), KEEP_MIN)


def part_keep_min(dtype):
    return 0.4 if dtype == torch.float32 else 0.35


def has_part(ref):
    """fraction of the points with at least one part inside the mask"""
    return float((_in_mask(ref.real) | _in_mask(ref.imag)).mean())


# ---- A: the formulas of csrc/cplxfn.hip in float32 numpy ----------------------------------------------------------------
# Every elementary function is evaluated in float64 and rounded once to float32 (a stand-in for a correctly rounded float32
# function); every arithmetic operation is a float32 numpy operation.  Written from the header of cplxfn.hip.
def _r(a):
    return np.asarray(a, np.float64).astype(F32)


def _f(fun):
    return lambda *a: _r(fun(*[np.asarray(x, np.float64) for x in a]))


_exp, _expm1, _sin, _cos, _tan, _log, _log1p, _atan2, _sqrt = (_f(g) for g in (
    np.exp, np.expm1, np.sin, np.cos, np.tan, np.log, np.log1p, np.arctan2, np.sqrt))
K_SAT = F32(11.0)
_H, _1, _2, _4 = F32(0.5), F32(1.0), F32(2.0), F32(4.0)


def _chsh(t):
    a = np.abs(t)
    em = _expm1(np.minimum(a, F32(88.0)))
    e = em + _1
    c, s = _H * e + _H / e, _H * (em + em / e)
    h = _exp(_H * a)
    big = (_H * h) * h
    c, s = np.where(a <= 88.0, c, big), np.where(a <= 88.0, s, big)
    return c.astype(F32), np.copysign(s, t).astype(F32)


def _chsh_mul(t, p, q, fixed=True):
    """(cosh t * p, sinh t * q); past 88 the factor goes in between the two e^{|t|/2} (fixed), or after them (the old form)"""
    c, s = _chsh(t)
    cp, sq = c * p, s * q
    if fixed:
        a = np.abs(t)
        h = _exp(_H * a)
        hh = _H * h
        cp = np.where(a <= 88.0, cp, (hh * p) * h)
        sq = np.where(a <= 88.0, sq, (np.copysign(hh, t) * q) * h)
    return cp.astype(F32), sq.astype(F32)


def emulate(fn, x, y, fixed=True):
    """float32 (re, im) of f(x + iy) by the kernel's formulas; fixed=False: the forms before the part-overflow fix"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        if fn == "exp":
            s, c = _sin(y), _cos(y)
            e = _exp(x)
            re, im = e * c, e * s
            if fixed:
                h = _exp(_H * x)
                re, im = np.where(x > 88.0, (h * c) * h, re), np.where(x > 88.0, (h * s) * h, im)
            return re.astype(F32), im.astype(F32)
        if fn == "log":
            ax, ay = np.abs(x), np.abs(y)
            a, b = np.maximum(ax, ay), np.minimum(ax, ay)
            r = b / np.where(a == 0, _1, a)
            re = _log(a) + _H * _log1p(r * r)
            re = np.where(np.isinf(a), F32(np.inf), np.where(a == 0, F32(-np.inf), re))
            return re.astype(F32), _atan2(y, x)
        if fn == "sin":
            ch, sh = _chsh_mul(y, _sin(x), _cos(x), fixed)
            return ch, sh
        if fn == "cos":
            ch, sh = _chsh_mul(y, _cos(x), _sin(x), fixed)
            return ch, -sh
        if fn == "sinh":
            ch, sh = _chsh_mul(x, _sin(y), _cos(y), fixed)
            return sh, ch
        if fn == "cosh":
            return _chsh_mul(x, _cos(y), _sin(y), fixed)
        if fn == "tan":
            re, im = emulate("tanh", -y, x)
            return im, -re
        assert fn == "tanh"
        sy, cy = _sin(y), _cos(y)
        sat_im = _4 * sy * cy * _exp(-_2 * np.abs(x))
        _, s = _chsh(x)
        t = _tan(y)
        beta, rho = _1 + t * t, _sqrt(_1 + s * s)
        den = _1 + beta * s * s
        re, im = beta * rho * s / den, t / den
        sat = np.abs(x) > K_SAT
        return np.where(sat, np.copysign(_1, x), re).astype(F32), np.where(sat, sat_im, im).astype(F32)


def _sech2(x, y):
    sy, cy = _sin(y), _cos(y)
    m, sg = _4 * _exp(-_2 * np.abs(x)), np.copysign(_1, x)
    c2, s2 = (cy - sy) * (cy + sy), _2 * sy * cy
    ch, sh = _chsh(x)
    d = sh * sh + cy * cy
    wr, wi = ch * cy / d, -(sh * sy) / d
    sat = np.abs(x) > K_SAT
    return (np.where(sat, m * c2, (wr - wi) * (wr + wi)).astype(F32), np.where(sat, -sg * m * s2, _2 * wr * wi).astype(F32))


def emulate_backward(fn, x, y, gr, gi):
    """float32 conj(f'(z)) g by the kernel's formulas"""
    x, y, gr, gi = (np.asarray(a, F32) for a in (x, y, gr, gi))
    with np.errstate(all="ignore"):
        if fn == "log":                      # 1 / z = conj(z) / |z|^2 after scaling by a power of two
            a = np.maximum(np.abs(x), np.abs(y))
            k = np.where((a > 0) & np.isfinite(a), -np.floor(np.log2(np.where(a > 0, a, 1).astype(np.float64))), 0).astype(int)
            xs, ys = np.ldexp(x, k).astype(F32), np.ldexp(y, k).astype(F32)
            d = xs * xs + ys * ys
            dr, di = np.ldexp(xs / d, k).astype(F32), np.ldexp(-ys / d, k).astype(F32)
        elif fn == "tan":
            dr, di = _sech2(-y, x)
        elif fn == "tanh":
            dr, di = _sech2(x, y)
        elif fn == "cos":
            dr, di = emulate("sin", x, y)
            dr, di = -dr, -di
        else:
            dr, di = emulate({"exp": "exp", "sin": "cos", "sinh": "cosh", "cosh": "sinh"}[fn], x, y)
        return (dr * gr + di * gi).astype(F32), (dr * gi - di * gr).astype(F32)


# ---- A: signed zeros and infinities ------------------------------------------------------------------------------------
def special_table():
    """[(fn, re, im)]: every entry is compared with torch complex128 on the CPU, signbit included.  No entry on which the
    reference project's own formula decides nothing else (exp(+inf + 0i) = inf * 0 and the like are left out)."""
    z, inf = (0.0, -0.0), float("inf")
    t = [(fn, a, b) for fn in ("sin", "sinh", "tan", "tanh") for a in z for b in z]
    t += [("log", 0.0, 0.0), ("log", -0.0, 0.0), ("log", -1.0, 0.0), ("log", -1.0, -0.0), ("log", inf, 1.0), ("log", -inf, 1.0)]
    t += [("exp", -inf, y) for y in (0.5, -0.5, 2.0, -2.0, 4.0)]
    t += [("tanh", s * inf, y) for s in (1, -1) for y in (0.5, -0.5, 2.0, -2.0)]
    t += [("tan", x, s * inf) for s in (1, -1) for x in (0.5, -0.5, 2.0, -2.0)]
    return t


def special_reference(table):
    out = []
    for fn, a, b in table:
        w = getattr(torch, fn)(torch.tensor([complex(a, b)], dtype=torch.complex128))[0]
        out.append((float(w.real), float(w.imag)))
    return out


def same_special(got, ref):
    """a float32 result equals a float64 reference value: zeros and infinities with their sign, else within 2 u"""
    if ref == 0 or np.isinf(ref):
        return got == ref and np.signbit(got) == np.signbit(ref)
    return abs(got - ref) <= 2 * U * abs(ref)


# ---- B: inputs ----------------------------------------------------------------------------------------------------------
def pattern(seed, n=PERIOD, scale=2.0):
    return (scale * np.random.RandomState(seed).randn(n)).astype(F32)


def tile_to(p, n):
    """the first n elements of p repeated (numpy or torch, 1-d)"""
    reps = -(-n // len(p)) if n else 0
    return (np.tile(p, reps) if isinstance(p, np.ndarray) else p.repeat(reps))[:n]


_NA = np.nextafter
TAU = F32(0.5)
_e20, _sub, _inf, _nan = F32(1e20), F32(1e-40), F32(np.inf), F32(np.nan)
# (re, im) of z: +-0, a subnormal, |z| on either side of the 1e-5 clamp, |z| within 2 ulps of tau = 0.5 (the 1 - tau / m sign
# change), 1e20 (the squares overflow), +-inf, NaN, and two plain values.  19 entries: odd, so cycling the table through an
# array puts four different entries into every aligned quad and some into every tail (the plain ones sit where no
# one-element tail of the sweep's sizes lands: test_elementwise_host.py).
EDGE_Z = np.array([
    (0.0, 0.0), (-0.0, 0.0), (3.0, -4.0), (_sub, 0.0), (_sub, -_sub), (6e-6, 0.0), (0.0, 1.2e-5), (1e-5, 0.0),
    (TAU, 0.0), (_NA(TAU, F32(1)), 0.0), (0.0, _NA(TAU, F32(0))), (0.0, -_NA(_NA(TAU, F32(1)), F32(1))), (_e20, _e20),
    (-_e20, 3.0), (_inf, 1.0), (1.0, -_inf), (_nan, 1.0), (0.0, -0.0), (-1.5, 2.5)], F32)
# thresholds for the full-shape variant: 0.5 mostly (so the entries above meet their tau), a negative one, the clamp itself
EDGE_TAU = np.array([0.5, 0.5, -0.5, 0.5, 1e-5, 0.5, -2.0], F32)
# second operand of mul / div: c^2 + d^2 overflows (1e20) and underflows (1e-30) on purpose
EDGE_W = np.array([(1.0, 0.0), (_e20, 1.0), (0.0, 1.0), (1e-30, 1e-30), (-3.0, 0.5), (0.0, 0.0), (_sub, 1.0), (-0.0, 0.0),
                   (0.25, -0.75), (_inf, 0.0), (2.0, _nan)], F32)
EDGE_MASK = np.array([1.0, 0.0, -0.0, 0.5, _inf, _nan, -2.0], F32)


def edge_planes(n):
    """(zr, zi, tau, wr, wi, mask) of n elements, each table cycled from its start"""
    cyc = lambda tab: tab[np.arange(n) % len(tab)]  # noqa: E731
    z, w = cyc(EDGE_Z), cyc(EDGE_W)
    return z[:, 0].copy(), z[:, 1].copy(), cyc(EDGE_TAU).copy(), w[:, 0].copy(), w[:, 1].copy(), cyc(EDGE_MASK).copy()


def is_special(zr, zi):
    """the elements of an edge plane pair that are one of the special values (not the two plain entries)"""
    m = np.sqrt(zr.astype(np.float64) ** 2 + zi.astype(np.float64) ** 2)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(m) | (m < 2e-5) | (np.abs(m - 0.5) < 1e-6) | (m > 1e19)


def bf16(a):
    """float32 numpy -> the float32 values of its bfloat16 rounding"""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.bfloat16).float().numpy()


# ---- B: float32 chains (one rounding per operation, the order the kernels document) ------------------------------------
def mul_chain(a, b, c, d, div=False):
    """csrc/layout.hip cplx_mul_kernel / cplxmodule/cplx.py:135-165"""
    with np.errstate(all="ignore"):
        if div:
            den = c * c + d * d
            c, d = c / den, -d / den
        return a * c - b * d, b * c + a * d


def split_relu_chain(a):
    with np.errstate(invalid="ignore"):
        return np.where((a > 0) | np.isnan(a), a, F32(0.0)).astype(F32)


def abs2_chain(x, y=None):
    with np.errstate(all="ignore"):
        return x * x if y is None else x * x + y * y


def to_dtype(a, dtype):
    """float32 numpy -> CPU tensor of dtype (round to nearest even: the kernels' one rounding on store)"""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(dtype)


# ---- D: pooling ---------------------------------------------------------------------------------------------------------
POOL_SHAPE = (2, 3, 7, 6)


def pool_planes(nan=False):
    """Gaussian integers a + ib with a, b in -5 ... 5 (exact ties: 3+4i, 4+3i, 5, 5i all have modulus 5), float32; and
    integer upstream gradients, so the sums over overlapping windows are exact in bf16 as well"""
    rs = np.random.RandomState(17)
    zr, zi = rs.randint(-5, 6, POOL_SHAPE).astype(F32), rs.randint(-5, 6, POOL_SHAPE).astype(F32)
    if nan:
        for b, c, h, w in ((0, 0, 0, 0), (0, 1, 3, 2), (1, 2, 6, 5), (1, 0, 3, 3), (0, 2, 2, 4)):
            zr[b, c, h, w] = np.nan
    return zr, zi


def pool_configs():
    """every (kernel, stride, padding, dilation, ceil_mode) of the product that torch accepts on the CPU"""
    kernels, strides, dilations = (1, 2, 3, (3, 2)), (1, 2, 3, (2, 1)), (1, 2, (1, 2))
    pair = lambda v: (v, v) if isinstance(v, int) else v  # noqa: E731
    out = []
    probe = torch.zeros(POOL_SHAPE)
    for k, s, half, d, ceil in itertools.product(kernels, strides, (False, True), dilations, (False, True)):
        p = tuple(x // 2 for x in pair(k)) if half else (0, 0)
        try:
            torch.nn.functional.max_pool2d(probe, pair(k), pair(s), p, pair(d), ceil)
        except RuntimeError:
            continue
        cfg = (pair(k), pair(s), p, pair(d), ceil)
        if cfg not in out:
            out.append(cfg)
    return out


def pool_modulus(zr, zi):
    """|z| in float32 in the form oracle.cplx_oracle.cplx_abs states"""
    from oracle import cplx_oracle as orc
    return orc.cplx_abs(zr, zi)


def pool_grads(shape):
    """integer-valued upstream gradients (gr, gi) of an output shape"""
    rs = np.random.RandomState(int(np.prod(shape)) % 1000 + 5)
    return torch.from_numpy(rs.randint(-3, 4, shape).astype(F32)), torch.from_numpy(rs.randint(-3, 4, shape).astype(F32))


def pool_reference(zr, zi, cfg):
    """(yr, yi, idx, gr, gi, dzr, dzi): F.max_pool2d(|z|, return_indices=True) on the CPU plus two gathers; gradients =
    scatter-add of the upstream gradients pool_grads(output shape) at the selected positions."""
    k, s, p, d, ceil = cfg
    B, C, H, W = zr.shape
    mod = torch.from_numpy(pool_modulus(zr, zi))
    _, idx = torch.nn.functional.max_pool2d(mod, k, s, p, d, ceil, return_indices=True)
    flat = idx.reshape(B, C, -1)
    take = lambda a: torch.from_numpy(a).reshape(B, C, -1).gather(2, flat).reshape(idx.shape)  # noqa: E731
    gr, gi = pool_grads(tuple(idx.shape))
    scat = lambda g: torch.zeros(B, C, H * W).scatter_add_(2, flat, g.reshape(B, C, -1)).reshape(B, C, H, W)  # noqa: E731
    return take(zr), take(zi), idx, gr, gi, scat(gr), scat(gi)
