"""Case tables, numpy emulation and error model of the operand-range tests of the float32 split products
(test_x2_range_host.py, test_gpu_x2_range.py; cplxmodule_amd/x3.py, csrc/split.hip).

The emulation restates csrc/split.hip operation by operation in numpy float32 / float16, so that the kernels' pieces can be
compared with it bit for bit:

    absmax_scale     m = max |op(x)|;  s = 2^k, k = clip(15 - e, -120, 120) with m = f 2^e, f in [0.5, 1);  s = 1 for m = 0 and
                     for a tensor that holds (or whose op produces) an inf or a NaN.  Returns (s, 1 / s).
    split2h          v = op(x) * s in float32;  h0 = half(v) (round to nearest even; inf beyond 65520);  h1 = half(v - h0)
                     where |v| <= 65504, else 0.
    split3           x0 = bf16(x);  x1 = bf16(x - x0) where |x| <= the largest finite bf16, else 0;  x2 = bf16(x - x0 - x1).
    ops              OP_ID x;  OP_ABS2 fl(fl(a a) + fl(b b)) -- one rounding per operation, no fused multiply-add;  OP_EXP
                     expf(x) (the device's expf is not numpy's to the last bit: the GPU tests hand the device's values in as
                     `value`);  OP_MAX2 max(|a|, |b|), a NaN in either plane counting as non-finite (scale only).

The error model.  C = A B^T from the pieces, in one float32 accumulator chain over the K-concatenated piece products,
obeys element by element

    |C - A B^T|[m, n] <= sum_k (da |b| + |a| db + da db) + gamma(3 K + extra) (sum_k |a| |b| + |head|) + 2^-149

    'x2':  da = max(2^-22 |a s|, 2^-25) / s  per element, s the one scale of the whole operand (the numbers in the header
           comment of split.hip: two 11-bit pieces, the second one losing bits to half's subnormals below 2^-25);
    'x3':  da = 2^-24 |a|  (the three bf16 pieces are exact; the three dropped piece products are below 2^-24 |a b| each);
    gamma(n) = n u / (1 - n u),  u = 2^-24:  the worst case of a float32 chain of n additions.  `extra` / `head`: what else
           sits in the chain -- a bias (one more addition), beta * C_old (two more) -- 0 for a raw product;
    2^-149: the undo's rounding where the result is a float32 subnormal (else the undo is exact: powers of two).

The bound is derived from the formats, not measured.  A complex product is the real product of the K-concatenations
[Ar | -+Ai] [Br | Bi]^T (real plane) and [Ar | Ai] [+-Bi | Br]^T (imaginary plane): the same formula at twice the K.

What 'x2' promises row by row follows from da: a row of A whose elements lie below 2^-41 max|A| is all zeros in half
(|a s| < 2^-26, under half of the smallest subnormal) and its row of C comes back exactly 0; 'x3' has no scale, so C of a
row scaled by a power of two is the scaled row of C bit for bit.
"""
import zlib

import numpy as np

OP_ID, OP_ABS2, OP_EXP, OP_MAX2 = 0, 1, 2, 3
U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
BF16_MAX = 3.3895313892515355e38
CLIP = 120


# ---- emulation of csrc/split.hip ------------------------------------------------------------------------------------------------
def op_value(op, a, b=None, value=None):
    """op(a[, b]) as the kernels form it, float32.  `value`: precomputed values (OP_EXP on the device)."""
    if value is not None:
        return np.asarray(value, dtype=np.float32)
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if op == OP_ABS2:
            bb = np.zeros_like(a) if b is None else np.asarray(b, dtype=np.float32)
            return ((a * a).astype(np.float32) + (bb * bb).astype(np.float32)).astype(np.float32)
        if op == OP_EXP:
            return np.exp(a.astype(np.float64)).astype(np.float32)
        return a


def emulate_absmax_scale(a, b=None, op=OP_ID, value=None):
    """cplxamd_absmax_scale -> (s, 1 / s) as float32."""
    if op == OP_MAX2:
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        v = np.maximum(np.abs(a), np.abs(b))
        v = np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), v)
    else:
        v = np.abs(op_value(op, a, b, value))
    return scale_from_max(np.float32(np.inf) if (v.size and np.isnan(v).any()) else (v.max() if v.size else np.float32(0)))


def scale_from_max(m):
    """The second stage (cplxamd_absmax_scale_partials): the maximum -> (s, 1 / s)."""
    m = np.float32(m)
    k = 0
    if m > 0 and m <= np.float32(FLT_MAX):
        k = int(np.clip(15 - int(np.frexp(m)[1]), -CLIP, CLIP))
    return np.float32(2.0 ** k), np.float32(2.0 ** -k)


def emulate_split2h(a, s, b=None, op=OP_ID, value=None):
    """cplxamd_split2h -> (h0, h1) as float16 arrays (first = leading piece)."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = (op_value(op, a, b, value) * np.float32(s)).astype(np.float32)
        h0 = v.astype(np.float16)
        fin = np.abs(v) <= np.float32(65504.0)
        r1 = np.where(fin, v - h0.astype(np.float32), np.float32(0)).astype(np.float32)
        return h0, r1.astype(np.float16)


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even; NaN stays NaN), returned as float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32)


def emulate_split3(a, b=None, op=OP_ID, value=None):
    """cplxamd_split3 -> (x0, x1, x2) as float32 arrays holding bf16 values (first = leading piece)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = op_value(op, a, b, value)
        x0 = bf16_round(x)
        fin = np.abs(x) <= np.float32(BF16_MAX)
        r1 = np.where(fin, x - x0, np.float32(0)).astype(np.float32)
        x1 = bf16_round(r1)
        return x0, x1, bf16_round((r1 - x1).astype(np.float32))


def emulated_pieces(kind, a, s=None):
    """float64 pieces of one plane, leading piece first ('x2': in scaled units)."""
    if kind == "x2":
        return [p.astype(np.float64) for p in emulate_split2h(a, s)]
    return [p.astype(np.float64) for p in emulate_split3(a)]


# (term of A, term of B) of the piece products each arithmetic forms (x3.py _SEQ / _TT_ORDER)
TERMS = {"x2": ((0, 0), (0, 1), (1, 0)), "x3": ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))}


def emulated_product(kind, A, B, sa=None, sb=None):
    """C = A B^T of real planes as the split arithmetic defines it: the emulated pieces multiplied and summed in float64, the
    scale undo and the store rounded to float32.  sa, sb: (s, 1 / s) pairs ('x2'; None: emulate_absmax_scale of the plane)."""
    if kind == "x2":
        sa = sa or emulate_absmax_scale(A)
        sb = sb or emulate_absmax_scale(B)
    pa = emulated_pieces(kind, A, sa and sa[0])
    pb = emulated_pieces(kind, B, sb and sb[0])
    acc = sum(pa[i] @ pb[j].T for i, j in TERMS[kind])
    if kind == "x2":
        acc = acc * float(sa[1]) * float(sb[1])
    with np.errstate(over="ignore"):
        return acc.astype(np.float32)


# ---- the error model ----------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


def piece_error(kind, a, s=None):
    """da of the module docstring, float64, per element."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    if kind == "x3":
        return a * 2.0 ** -24
    s = float(s)
    return np.maximum(a * s * 2.0 ** -22, 2.0 ** -25) / s


def bound(kind, A, B, sa=None, sb=None, head=None, extra=0):
    """The element-wise bound of the module docstring for C = A B^T, A [M, K], B [N, K] real planes (float64 [M, N]).
    sa, sb: the scales s of 'x2' (None: emulate_absmax_scale of the plane).  head / extra: |bias| or |beta C_old| (broadcast to
    [M, N]) and the additions it adds to the chain."""
    A64, B64 = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(B, dtype=np.float64))
    if kind == "x2":
        sa = emulate_absmax_scale(A)[0] if sa is None else sa
        sb = emulate_absmax_scale(B)[0] if sb is None else sb
    da, db = piece_error(kind, A, sa), piece_error(kind, B, sb)
    mag = A64 @ B64.T + (0.0 if head is None else np.abs(head))
    return da @ B64.T + A64 @ db.T + da @ db.T + gamma(3 * A.shape[1] + extra) * mag + 2.0 ** -149


def cplx_as_real(Ar, Ai, Br, Bi, conj_b):
    """A complex product C = A op(B)^T as two real ones at twice the K: -> ((A', B') of the real plane, (A'', B'') of the
    imaginary plane) with Cr = A' B'^T, Ci = A'' B''^T."""
    sg = -1.0 if conj_b else 1.0
    return ((np.hstack([Ar, -sg * Ai]), np.hstack([Br, Bi])), (np.hstack([Ar, Ai]), np.hstack([sg * Bi, Br])))


def cplx_bound(kind, Ar, Ai, Br, Bi, head=None, extra=0):
    """The bound for both planes of a complex product: one scale per operand, shared by its planes (x3.split_planes)."""
    sa = sb = None
    if kind == "x2":
        sa, sb = emulate_absmax_scale(Ar, Ai, OP_MAX2)[0], emulate_absmax_scale(Br, Bi, OP_MAX2)[0]
    (a1, b1), (a2, b2) = cplx_as_real(Ar, Ai, Br, Bi, False)        # (the bound reads magnitudes only)
    h = (None, None) if head is None else head
    return bound(kind, a1, b1, sa, sb, h[0], extra), bound(kind, a2, b2, sa, sb, h[1], extra)


def reference(planes_a, planes_b, conj_b=False):
    """float64 A op(B)^T per plane from float32 operands (tuples of 1 or 2 planes)."""
    f = [np.asarray(p, dtype=np.float64) for p in planes_a]
    g = [np.asarray(p, dtype=np.float64) for p in planes_b]
    if len(f) == 1:
        return (f[0] @ g[0].T,)
    (a1, b1), (a2, b2) = cplx_as_real(f[0], f[1], g[0], g[1], conj_b)
    return a1 @ b1.T, a2 @ b2.T


# ---- section D: power-of-two invariance -------------------------------------------------------------------------------------
# (p, q): A carries 2^p, B carries 2^q.  Every pair keeps both scale exponents inside the clip and the result normal.
PAIRS = ((0, 0), (-40, -40), (-52, -52), (-60, -45), (-100, 60), (58, 58))
BEYOND_CLIP = (-125, 0)                 # k = 137 clips to 120: no invariance, the bound with the clipped scale
# 'x3' (the control) has no scales: its accumulators hold the products at their true magnitude.  Every nonzero piece of the
# base operands is a multiple of 2^-29 (A) or 2^-32 (B), so every partial sum of piece products is at least 2^-61, and
# from p + q = -65 down the smallest ones are float32 subnormals, which the matrix pipe may flush to zero on the way: each
# of the 6 K accumulation steps per real product then loses less than 2^-126.  Above that sum the identity is bit-exact
# for 'x3' too; below it 'x3' is held to that many flushes plus one rounding of the result.  ('x2' accumulates in scaled
# units, around 2^30 whatever p and q are: bit-exact on every pair.)
X3_EXACT_FROM = -65


def x3_flush_allowance(K, cplx):
    return 6 * K * (2 if cplx else 1) * 2.0 ** -126
TINY = (-52, -52)                       # with a bias of order 1, or 0: the result is the bias
# (M, N, K).  The first two are ragged / sub-tile shapes: every family's launcher hands them to the eight-wave one-tile kernel
# (kind 1).  The one-wave-per-SIMD family takes whole 256 x 128 (complex) / 256 x 256 (real) tiles and K % 64 == 0, K >= 128
# per launch: the third shape is its smallest.
SHAPES = ((64, 96, 64), (264, 136, 96), (256, 256, 128))
FAMILIES = ("eight-wave", "one-wave-per-SIMD")
BETA = 0.5                               # gemm_tt accumulates on top of BETA * C_old
LAYOUTS = ("NN", "NT", "TT")


def expected_kind(family, M, N, K, cplx):
    """What cplxamd_gemm_plan must report for every launch of a sequence (gemm_exact_cases.KIND_NAME): 3 where the
    one-wave-per-SIMD family was asked for and takes the shape, else 1."""
    whole = M % 256 == 0 and N % (128 if cplx else 256) == 0 and K % 64 == 0 and K >= 128
    return 3 if family == "one-wave-per-SIMD" and whole else 1


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def dyadic(rs, shape, lo, hi):
    """float32 values with |v| in [2^lo, 2^hi), a random sign and a random 24-bit significand: multiplying by 2^p is exact
    while the result stays normal."""
    e = rs.randint(lo, hi, size=shape)
    m = (rs.randint(0, 1 << 23, size=shape) + (1 << 23)).astype(np.float64) * 2.0 ** -23          # [1, 2)
    sgn = rs.randint(0, 2, size=shape) * 2.0 - 1.0
    v = (sgn * m * 2.0 ** e).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), sgn * m * 2.0 ** e)
    return v


def invariance_operands(M, N, K, cplx, tag=""):
    """Base operands of section D: |a| in [2^-6, 4), |b| in [2^-9, 0.5); a bias and an old C of the result's order; planes as
    tuples.  float32."""
    rs = _rs("D", M, N, K, cplx, tag)
    P = 2 if cplx else 1
    return dict(a=tuple(dyadic(rs, (M, K), -6, 2) for _ in range(P)), b=tuple(dyadic(rs, (N, K), -9, -1) for _ in range(P)),
                bias=tuple(dyadic(rs, (N,), -3, 1) for _ in range(P)), c0=tuple(dyadic(rs, (M, N), -3, 1) for _ in range(P)))


def shifted(planes, p):
    """planes * 2^p in float32 (exact for the dyadic operands while the result is normal)."""
    with np.errstate(under="ignore"):
        return tuple(np.ldexp(v, p).astype(np.float32) for v in planes)


# ---- section E: rows of one operand scaled block by block ----------------------------------------------------------------------
ROW_SHIFTS = (0, 8, 17, 24, 30, 38, 41, 45)
E_SHAPE = (128, 64, 128)
ZERO_FROM = 41                           # 'x2': rows below 2^-41 of the operand's maximum are zeros in half


def row_range_operands(cplx, side):
    """Section E: well-scaled dyadic operands A [128, 128], B [64, 128]; `side` 'a' | 'b' names the operand whose rows are
    scaled by 2^-r in eight equal blocks, r in ROW_SHIFTS.  -> (base planes a, base planes b, r per row of that operand).
    Every block's first row holds an element of the largest binade, so that the ratio of the block maxima is 2^-r exactly."""
    M, N, K = E_SHAPE
    rs = _rs("E", cplx, side)
    P = 2 if cplx else 1
    a = [dyadic(rs, (M, K), -3, 1) for _ in range(P)]
    b = [dyadic(rs, (N, K), -3, 1) for _ in range(P)]
    rows = M if side == "a" else N
    r = np.repeat(np.array(ROW_SHIFTS), rows // len(ROW_SHIFTS))
    tgt = a if side == "a" else b
    for blk in range(len(ROW_SHIFTS)):
        tgt[0][blk * (rows // len(ROW_SHIFTS)), 0] = np.float32(1.5)        # (binade [1, 2): the largest)
    return tuple(a), tuple(b), r


def scale_rows(planes, r):
    return tuple(np.ldexp(v, -r[:, None]).astype(np.float32) for v in planes)


# ---- section F: the layers, sample by sample -------------------------------------------------------------------------------------
F_B, F_I, F_O = 128, 64, 96
F_TOL = 1e-5                             # the project's float32 parity bar, against each row's own largest reference value
F_ROW_SPAN = tuple(8 - 2 * j for j in range(8))       # sample blocks of 16 carry 2^(8 - 2 j): |x| spans 2^14, |x|^2 2^28
CLAMP = 1e-8                             # reparam.hip: sigma = sqrt(max(s2, 1e-8))
# the samples are N(0, 1) times this before the block scales: the smallest s2 (last sample block, last output units, whose
# variances carry 2^-21) is then about 64 * 32^2 * 2^-12 * 0.245 * 2^-21 = 2e-6 -- two hundred times the clamp
F_AMPLITUDE = 32.0


def layer_inputs(cplx):
    """The recipe of section F, float32: x [128, 64] (N(0, 32^2) sample rows in blocks of 16 scaled by 2^(8 - 2 j)), W [96, 64], bias,
    log_sigma2[o, :] = U(-4, 0) - 3 (o // 12) ln 2, the noise eps and an output gradient g (quarters), per plane where complex."""
    rs = _rs("F", cplx)
    P = 2 if cplx else 1
    sc = np.repeat(2.0 ** np.array(F_ROW_SPAN, dtype=np.float64), F_B // 8)[:, None]
    d = dict(x=tuple((rs.randn(F_B, F_I) * (F_AMPLITUDE * sc)).astype(np.float32) for _ in range(P)),
             w=tuple((rs.randn(F_O, F_I) * 0.1).astype(np.float32) for _ in range(P)),
             b=tuple((rs.randn(F_O) * 0.1).astype(np.float32) for _ in range(P)))
    d["ls2"] = (rs.uniform(-4, 0, (F_O, F_I)) - 3.0 * (np.arange(F_O) // 12)[:, None] * np.log(2.0)).astype(np.float32)
    nrm = np.sqrt(2.0) if cplx else 1.0
    d["eps"] = tuple((rs.randn(F_B, F_O) / nrm).astype(np.float32) for _ in range(P))
    # quarters in [-2, 2]: the bias gradient (column sums of g) is then exact in float32 whatever the order of summation,
    # so that its per-element check tests the kernel and not a cancellation
    d["g"] = tuple((rs.randint(-8, 9, (F_B, F_O)) / 4.0).astype(np.float32) for _ in range(P))
    return d


def row_check(got, ref, tol=F_TOL):
    """-> (worst ratio of a row's max |got - ref| to tol * that row's max |ref|, the rows that exceed 1)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.ndim == 1:
        got, ref = got[:, None], ref[:, None]
    err, den = np.abs(got - ref).max(axis=1), tol * np.abs(ref).max(axis=1)
    ratio = np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))     # (a zero row: exactly)
    return float(ratio.max()), np.nonzero(ratio > 1.0)[0]


# ---- section C: the scale and the split at their seams -----------------------------------------------------------------------
C_SHAPES = ((1, 8), (5, 40), (257, 64))


def scale_seam_inputs(rows, cols):
    """-> {name: (a, b, op)}: float32 planes [rows, cols] (b None where the op reads one plane) whose scale sits on a seam of
    absmax_final_kernel.  `SCALE_EXPECT[name]` is the exponent k of the scale the design promises (s = 2^k)."""
    rs = _rs("C", rows, cols)
    base = lambda: (rs.uniform(-0.9, 0.9, (rows, cols)) * 32.0).astype(np.float32)      # noqa: E731   |x| < 28.8
    mid = (rows // 2, cols // 2)
    out = {}
    a = base(); a[mid] = 32.0
    out["max_is_pow2"] = (a, None, OP_ID)                     # 32 = 0.5 2^6: k = 9, 32 s = 2^14
    a = base(); a[mid] = -np.nextafter(np.float32(32.0), np.float32(0.0))
    out["max_below_pow2"] = (a, None, OP_ID)                  # the largest value of the binade below: k = 10
    out["max_is_denormal"] = (np.ldexp(base(), -145).astype(np.float32), None, OP_ID)      # k = 15 - e > 120: clipped
    a = base(); a[mid] = np.float32(FLT_MAX)
    out["max_is_flt_max"] = (a, None, OP_ID)                  # e = 128: k = -113
    a = base(); a[-1, -1] = 100.0
    out["max_in_last_element"] = (a, None, OP_ID)             # 100 = 0.78 2^7: k = 8
    out["negative_zero_only"] = (np.full((rows, cols), -0.0, dtype=np.float32), None, OP_ID)
    out["all_zero"] = (np.zeros((rows, cols), dtype=np.float32), None, OP_ID)
    a = base(); a[mid] = np.float32(-np.inf)
    out["one_inf"] = (a, None, OP_ID)
    a = base(); a[mid] = np.float32(np.nan); a[0, 0] = 1e30
    out["nan_among_larger_values"] = (a, None, OP_ID)
    a = base(); a[mid] = np.float32(2.0 ** 70)
    out["abs2_overflows"] = (a, base(), OP_ABS2)              # (2^70)^2 = inf
    a = base(); a[0, -1] = 5.0
    out["abs2"] = (a, None, OP_ABS2)                          # max x^2 < 829.5 = 0.81 2^10: k = 5
    a = (base() / 32.0).astype(np.float32); a[mid] = 89.0
    out["exp_of_89"] = (a, None, OP_EXP)                      # expf(89) = inf
    b = base(); b[mid] = np.float32(np.nan)
    out["max2_nan_in_second_plane"] = (base(), b, OP_MAX2)
    b = base(); b[-1, 0] = -200.0
    out["max2"] = (base(), b, OP_MAX2)                        # 200 = 0.78 2^8: k = 7
    return out


SCALE_EXPECT = dict(max_is_pow2=9, max_below_pow2=10, max_is_denormal=120, max_is_flt_max=-113, max_in_last_element=8,
                    negative_zero_only=0, all_zero=0, one_inf=0, nan_among_larger_values=0, abs2_overflows=0, abs2=5,
                    exp_of_89=0, max2_nan_in_second_plane=0, max2=7)

PARTIAL_COUNTS = (0, 1, 257, 2048)


def partial_inputs(n):
    """2048 per-block maxima of which the first n count (the rest: larger values and a NaN, never to be read), the largest
    of the n in the last one.  -> (float32[2048], the maximum of the first n)."""
    rs = _rs("partials", n)
    p = np.full(2048, 3.0e38, dtype=np.float32)
    p[-1] = np.nan
    p[:n] = rs.uniform(0.0, 7.0, n).astype(np.float32)
    if n:
        p[n - 1] = 9.5
    return p, (9.5 if n else 0.0)


SPLIT_S = 3                              # the scale of split_seam_input: s = 2^3


def split_seam_input(rows, cols):
    """A float32 plane whose scale is 2^SPLIT_S and whose SCALED values cover: magnitudes 2^-45 .. 1 of the maximum (normal
    halves, subnormal halves, flush to zero), exact ties of the first piece in the normal range (odd multiples of half an
    ulp), ties in the subnormal range (2^-25 -> 0, 3 2^-25 -> 2^-23), +-0, and the largest magnitude 1.5 2^14."""
    rs = _rs("split", rows, cols)
    v = dyadic(rs, (rows, cols), -31, 15).astype(np.float64)                 # scaled units: |v| in [2^-31, 2^15)
    flat = v.reshape(-1)
    n = flat.size
    ties = [2.0 ** 10 * (1 + (2 * j + 1) * 2.0 ** -11) for j in range(3)] + [-(2.0 ** 14) * (1 + 5 * 2.0 ** -11), 2.0 ** -25,
                                                                               -3 * 2.0 ** -25, 0.0, -0.0]
    if n >= 16:
        flat[1:1 + len(ties)] = ties
    flat[0] = 1.5 * 2.0 ** 14
    x = (v * 2.0 ** -SPLIT_S).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 2.0 ** SPLIT_S, v)
    return x
