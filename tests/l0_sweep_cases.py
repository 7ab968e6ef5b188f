"""Case tables, float64 oracle and bounds of the L0 gate / LASSO mask / LRT noise sweep (tests/test_l0_sweep_host.py,
tests/test_gpu_l0_sweep.py): numpy on the CPU, fixed seeds, no GPU.

Oracle (written from the reference's formulas, ell_zero.py:132-160, lasso.py:14, relevance/real/base.py:49; not from the
kernels): with u and log_alpha the float32 values the kernel receives, widened to float64,
  train  s = sigmoid((log u - log1p(-u) - la) / 0.66)      eval  s = sigmoid(-la)
  pre = 1.2 s - 0.1,  z = clip(pre, 0, 1),  dz = -1.2 s (1 - s) (/ 0.66 in train mode) where 0 <= pre <= 1, else 0
  forward out = a z (+ bias[c]);  backward da = d z, az = a z, term = d a dz (elementwise, or summed over the rows)
  LASSO  float32(log(float64(float32(|w| + 1e-20f)))) >= threshold
  LRT    sd = sqrt(max(s2, 1e-8)), y = mu + eps sd, g_s2 = (s2 >= 1e-8) 0.5 (g_r eps_r + g_i eps_i) / sd
The uniform stream is oracle/philox.py: element e = lane e & 3 of group e >> 2, counter (group, offset), key seed.

Bounds (none is taken from a kernel's output):
  TOL_Z   1e-5 absolute on z: the float32 parity bound of the layer (test_gpu_l0._close; the header of l0.hip)
  TOL_S   TOL_Z / 1.2;  TOL_DZ = (1.2 / 0.66) TOL_S  (dz is Lipschitz in s with constant 1.2 / 0.66 |1 - 2 s| <= 1.82)
  out, da, az      |a| TOL_Z + 2^-23 |ref|  (+ 2^-8 |ref| for a bf16 output: one rounding, the package's bf16 rule)
  term             |d a| TOL_DZ + 2^-23 |ref|
  column sums      sum_r |d a| TOL_DZ + 2e-6 sum_r |term|  (the float32 column-sum allowance of test_reparam_bwd_with_bias_sums)
  Philox noise     2e-5 absolute (the atol of test_philox_stream_matches_spec)
  y                2e-5 sd + 2^-23 |ref|;   g_s2   0.5 (|g_r| + |g_i|) 2e-5 / sd + 2e-6 |ref|
  given noise      the tolerances of test_reparam_given_noise, against its float32 one-rounding-per-op chain
Clamp band: dz and the hard mask jump at pre = 0 and pre = 1; elements whose float64 pre lies within TOL_Z of either are left
out of the dz / term / HARD comparisons (z, da, az are compared everywhere).  In a column sum such an element adds
|d a| 1.2 / 0.66 / 4 (the largest |dz|) to the column's bound, in a HARD count it adds 1.  At most EXCLUDE_CAP of a case's
elements may be in the band (the host test asserts it from the oracle alone); the directed edge tables put points ON the
boundaries and are exempt.
"""
import os
import re
import zlib

import numpy as np
import torch

from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cplxmodule_amd", "csrc")
F32 = np.float32


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


GRID_CAP = _const(_src("common.h"), r"if \(g > (\d+)\) g = \1;")             # common.h stream_grid: blocks per launch
L0_THREADS = _const(_src("l0.hip"), r"constexpr int kL0Threads = (\d+);")
RP_THREADS = _const(_src("reparam.hip"), r"constexpr int kRpThreads = (\d+);")
L8 = GRID_CAP * L0_THREADS * 8            # elements past which an 8-wide grid-stride loop makes a second trip
L1 = GRID_CAP * L0_THREADS                # ... a scalar one
RP_L8 = GRID_CAP * RP_THREADS * 8
SEED, OFFSET = 2 ** 64 - 1, 2 ** 40 + 3   # every Philox case

BETA, SPAN, GAMMA = 0.66, 1.2, -0.1
TOL_Z = 1e-5
TOL_S = TOL_Z / SPAN
TOL_DZ = (SPAN / BETA) * TOL_S
DZ_MAX = SPAN / BETA / 4
E32, EBF = 2.0 ** -23, 2.0 ** -8
COLSUM = 2e-6
NOISE_ATOL = 2e-5
COVERAGE = 0.25                           # the float32 restatement stays within a quarter of TOL_Z / TOL_DZ
EXCLUDE_CAP = 1e-3
WINDOW = 4096


# ---- uniform stream ---------------------------------------------------------------------------------------------------
def uniform_window(e0, e1, seed=SEED, offset=OFFSET):
    """elements [e0, e1) of the uniform stream as the float32 values a kernel sees, without forming the stream before e0"""
    g0, g1 = e0 >> 2, (e1 + 3) >> 2
    x = philox.philox4x32(np.arange(g0, g1, dtype=np.uint64), offset, seed)
    return philox._u01(x).reshape(-1)[e0 - 4 * g0:e1 - 4 * g0].astype(F32)


def normal_window(e0, e1, cplx, seed=SEED, offset=OFFSET):
    """elements [e0, e1) of the noise stream in float64: real (4 per group), or (eps_r, eps_i) (2 per group)"""
    per = 2 if cplx else 4
    g0, g1 = e0 // per, (e1 + per - 1) // per
    x = philox.philox4x32(np.arange(g0, g1, dtype=np.uint64), offset, seed)
    u = philox._u01(x)
    scale = np.sqrt(0.5) if cplx else 1.0
    r0, r1 = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    a0, a1 = 2 * np.pi * u[:, 1], 2 * np.pi * u[:, 3]
    z = scale * np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1)
    if cplx:
        z = z.reshape(-1, 2)[e0 - 2 * g0:e1 - 2 * g0]
        return z[:, 0], z[:, 1]
    return z.reshape(-1)[e0 - 4 * g0:e1 - 4 * g0]


def windows(n, seams=(L1, L8)):
    """[e0, e1) windows of WINDOW elements: the head, around every multiple of a seam that n crosses, the tail"""
    out = {(0, min(WINDOW, n)), (max(0, n - WINDOW), n)}
    for L in seams:
        for m in range(L, n, L):
            out.add((m - WINDOW // 2, min(n, m + WINDOW // 2)))
    return sorted(w for w in out if w[1] > w[0])


# ---- the gate ---------------------------------------------------------------------------------------------------------
def gate64(la, u=None):
    """float64 (z, dz, pre); u None: the eval gate"""
    la = np.asarray(la, np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        if u is None:
            s = 1.0 / (1.0 + np.exp(la))
        else:
            u = np.asarray(u, np.float64)
            s = 1.0 / (1.0 + np.exp(-((np.log(u) - np.log1p(-u) - la) / BETA)))
    pre = SPAN * s + GAMMA
    dz = np.where((pre >= 0) & (pre <= 1), -SPAN * s * (1 - s) / (BETA if u is not None else 1.0), 0.0)
    return np.clip(pre, 0, 1), dz, pre


def gate32(la, u=None):
    """float32 numpy restatement of the gate as the header of l0.hip states it (1 / beta as a float32 factor, sigmoid as
    a reciprocal, one rounding per operation) -> float32 (z, dz, pre)"""
    la = np.asarray(la, F32)
    one = F32(1)
    with np.errstate(over="ignore", divide="ignore"):
        if u is None:
            s = one / (one + np.exp(la))
        else:
            u = np.asarray(u, F32)
            logit = np.log(u) - np.log(one - u)
            s = one / (one + np.exp(-((logit - la) * F32(1.0 / 0.66))))
    pre = F32(1.2) * s + F32(-0.1)
    ds = s * (one - s) * F32(1.2)
    dz = np.where((pre >= 0) & (pre <= 1), -ds * F32(1.0 / 0.66) if u is not None else -ds, F32(0))
    return np.clip(pre, F32(0), F32(1)), dz.astype(F32), pre


def band(pre):
    """the clamp band: float64 pre within TOL_Z of 0 or of 1"""
    return (np.abs(pre) <= TOL_Z) | (np.abs(pre - 1) <= TOL_Z)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def rounded(a, dtype):
    """the operand as the kernel is given it (bf16: rounded, then widened), float32"""
    return bf16_round(a) if dtype == torch.bfloat16 else np.asarray(a, F32)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ---- gate data --------------------------------------------------------------------------------------------------------
A_SMALL = (1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 2055)
A_VECTOR = (L8 - 8, L8, L8 + 8, 2 * L8 + 24)
A_SCALAR = (L1 - 1, L1 + 1, L1 + 9)
A_MIXED = (L8 + 8 + 5,)
A_SIZES = A_SMALL + A_SCALAR + A_VECTOR + A_MIXED
A_MAX = max(A_SIZES)
_MASTER = {}


def elem_data(n):
    """(la, a, d) of the elementwise cases: prefixes of one master draw, so one host pass covers every size"""
    if not _MASTER:
        rs = _rs("A")
        _MASTER["la"] = rs.uniform(-4, 4, A_MAX).astype(F32)
        _MASTER["a"] = rs.standard_normal(A_MAX).astype(F32)
        _MASTER["d"] = rs.standard_normal(A_MAX).astype(F32)
    return _MASTER["la"][:n], _MASTER["a"][:n], _MASTER["d"][:n]


def cols_data(rows, cols):
    """(la [cols], a, d [rows, cols], bias [cols]) of a per-column case, float32"""
    rs = _rs("cols", rows, cols)
    la = rs.uniform(-4, 4, cols).astype(F32)
    a = rs.standard_normal((rows, cols)).astype(F32)
    d = rs.standard_normal((rows, cols)).astype(F32)
    return la, a, d, rs.standard_normal(cols).astype(F32)


# B: per-column forward.  name -> (rows, cols, vector form, trips of the grid-stride loop, column step dc of the vector form)
B_CASES = {
    "dc16": (116600, 72, True, 3, 16),
    "dc304": (8400, 1000, True, 3, 304),
    "dc0": (2056, 4096, True, 3, 0),
    "scalar_wrap": (14200, 37, False, 2, None),
    "one_vector": (1, 8, True, 1, None),
    "three_vectors": (3, 8, True, 1, None),
    "one_element": (1, 1, False, 1, None),
    "small_odd": (5, 37, False, 1, None),
}


def fwd_walk(rows, cols):
    """(vector form, trips, dc) of l0_fwd_kernel in per-column mode, from the constants read from the sources (aligned
    operands): the vector form takes n % 8 == 0 and cols % 8 == 0, a thread's column advances by (8 stride) % cols a trip"""
    n = rows * cols
    vec = n % 8 == 0 and cols % 8 == 0
    work = n // 8 if vec else n
    grid = min(max((work + L0_THREADS - 1) // L0_THREADS, 1), GRID_CAP)
    stride = grid * L0_THREADS
    trips = (work + stride - 1) // stride
    return vec, trips, ((8 * stride) % cols if vec and trips > 1 else None)


# C: per-column backward plans.  name -> (rows, cols, expected plan fields)
C_CASES = {
    "one_row_v8": (1, 8, dict(V=8, TX=1, TY=256, strips=1, chunks=1)),
    "one_row_v1": (1, 1, dict(V=1, TX=1, TY=256, strips=1, chunks=1)),
    "rows_under_ty": (5, 37, dict(V=1, TX=37, TY=6, idle=34, strips=1, chunks=1)),
    "v1_idle": (3001, 37, dict(V=1, TX=37, TY=6, idle=34, strips=1)),
    "v1_dead_groups": (700, 259, dict(V=1, TX=256, TY=1, strips=2, last_strip_groups=3)),
    "v8_dead_groups": (33, 2056, dict(V=8, TX=256, TY=1, strips=2, last_strip_groups=1, chunks=2, last_chunk_rows=16,
                                      rows_per_chunk=17)),
    "v8_tx125": (3, 1000, dict(V=8, TX=125, TY=2, idle=6, strips=1, chunks=1)),
    "ty32": (4099, 64, dict(V=8, TX=8, TY=32, idle=0, chunks=8)),
    "ty256": (16400, 8, dict(V=8, TX=1, TY=256, chunks=4)),
    "ty85": (40000, 3, dict(V=1, TX=3, TY=85, idle=1)),
    "three_strips": (9, 4104, dict(V=8, TX=256, TY=1, strips=3, last_strip_groups=1, chunks=1)),
}
C_CAP = (17000, 2048)                     # rows / 16 = 1062 chunks asked for: the 1024 cap


def cols_plan(rows, cols):
    """The plan of l0_bwd_cols_kernel restated from its comment: a thread owns V columns (8 when cols % 8 == 0, else 1), TX =
    min(column groups, threads) threads span a strip, TY = threads / TX row lanes; >= 16 row steps per thread, about
    2048 workgroups, at most 1024 chunks; a chunk's rows are a multiple of TY."""
    V = 8 if cols % 8 == 0 else 1
    CG = (cols + V - 1) // V
    TX = min(CG, L0_THREADS)
    TY = L0_THREADS // TX
    strips = (CG + TX - 1) // TX
    asked = rows // (16 * TY)
    cap = min(2048 // strips, 1024)
    chunks = max(min(asked, cap), 1)
    rpc = (rows + chunks - 1) // chunks
    rpc = (rpc + TY - 1) // TY * TY
    chunks = (rows + rpc - 1) // rpc
    return dict(V=V, TX=TX, TY=TY, idle=L0_THREADS - TX * TY, strips=strips, chunks=chunks, rows_per_chunk=rpc,
                capped=asked > cap, last_strip_groups=CG - (strips - 1) * TX, last_chunk_rows=rows - (chunks - 1) * rpc)


# E: dtype routes
E_SHAPES = ((300, 72), (301, 37))
_F, _B = torch.float32, torch.bfloat16
E_FWD = ((_F, _F), (_F, _B), (_B, _B), (_B, _F))                       # a -> out
E_BWD = ((_F, _F, _F, _F), (_F, _B, _B, _B), (_B, _F, _B, _B), (_B, _B, _B, _B))    # d, a, da, az: the keys of cplxamd_l0_gate_bwd
E_BWD_REFUSED = (_F, _F, _B, _B)


# ---- products and bounds ----------------------------------------------------------------------------------------------
def fwd_ref(z, a=None, bias=None):
    out = z if a is None else a.astype(np.float64) * z
    return out if bias is None else out + bias.astype(np.float64)


def out_bound(ref, a, dtype):
    """|a| TOL_Z + 2^-23 |ref| (+ 2^-8 |ref| in bf16); a None: the gate itself, |a| = 1"""
    scale = 1.0 if a is None else np.abs(a.astype(np.float64))
    return scale * TOL_Z + (E32 + (EBF if dtype == torch.bfloat16 else 0.0)) * np.abs(ref)


def term_bound(d, a, ref):
    return np.abs(d.astype(np.float64) * a) * TOL_DZ + E32 * np.abs(ref)


def colsum_ref(d, a, dz, pre):
    """float64 column sums of term, and their bound: excluded elements stay in, at the largest |dz| each"""
    da = np.abs(d.astype(np.float64) * a)
    term = d.astype(np.float64) * a * dz
    bound = da.sum(0) * TOL_DZ + COLSUM * np.abs(term).sum(0) + (da * band(pre)).sum(0) * DZ_MAX
    return term.sum(0), bound


# ---- D: directed edge tables ------------------------------------------------------------------------------------------
LN11 = float(np.log(11.0))
EDGE_LA = (0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 200.0, -200.0)
U_MIN, U_MAX = F32(2.0 ** -25), F32(1.0)  # the ends of the stream: ((x >> 8) + 0.5) 2^-24 at x >> 8 = 0 and 2^24 - 1


def neighbours(x, k):
    """x and its k float32 neighbours on each side, ascending"""
    lo = hi = F32(x)
    out = [F32(x)]
    for _ in range(k):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out = [lo] + out + [hi]
    return np.array(out, F32)


def edge_table(train):
    """(la, u or None, runs) as [rows, 64] float32 tables; runs: index ranges of ascending-la neighbour runs (eval)"""
    la, u, runs = [], [], []
    if train:
        for x in EDGE_LA:
            for e in (U_MIN, U_MAX, F32(0.5)):
                la.append(x), u.append(e)
        # u with pre exactly 0 (s = 1/12) and exactly 1 (s = 11/12): logit(u) = la -+ 0.66 ln 11; +-8 float32 neighbours
        for x in (-3.0, -1.0, -1e-3, 0.0, 1e-3, 1.0, 3.0):
            for sign in (-1.0, 1.0):
                u0 = 1.0 / (1.0 + np.exp(-(float(F32(x)) + sign * BETA * LN11)))
                for e in neighbours(u0, 8):
                    la.append(x), u.append(e)
    else:
        la += list(EDGE_LA)
        for x in (LN11, -LN11):            # eval: pre crosses 0 at la = ln 11 and 1 at la = -ln 11
            run = neighbours(x, 64)
            runs.append((len(la), len(la) + run.size))
            la += list(run)
    pad = -len(la) % 64
    la = np.array(la + [0.0] * pad, F32).reshape(-1, 64)
    u = np.array(u + [0.5] * pad, F32).reshape(-1, 64) if train else None
    return la, u, runs


# ---- F: LASSO mask ----------------------------------------------------------------------------------------------------
F_SIZES = (1, 255, 256, 257, L1 - 1, L1 + 3)
PERIOD = 1027
F_PIVOT = 5                               # the pattern element the thresholds sit on


def l1_pattern(n):
    rs = _rs("l1")
    p = rs.standard_normal(PERIOD).astype(F32)
    p[0] = 0.7310585975646973             # n = 1 sits on the pivot's value too
    p[F_PIVOT] = p[0]
    special = [0.0, -0.0, 1e-40, -1.401298464324817e-45, 1e-20, -1e-20, np.finfo(F32).max, -np.finfo(F32).max, np.inf,
               -np.inf, np.nan, 1e-38, 1e-19, 2e-20]
    p[16:16 + len(special)] = np.array(special, F32)
    p[300:300 + len(special)] = np.array(special, F32)[::-1]
    return np.resize(p, n)


def l1_log(w):
    """float32(log(float64(float32(|w| + 1e-20f))))"""
    with np.errstate(invalid="ignore"):
        return np.log((np.abs(np.asarray(w, F32)) + F32(1e-20)).astype(np.float64)).astype(F32)


def l1_thresholds():
    t = l1_log(l1_pattern(PERIOD)[F_PIVOT:F_PIVOT + 1])[0]
    return tuple(float(x) for x in neighbours(t, 1))


def l1_ref(w, threshold):
    with np.errstate(invalid="ignore"):
        return l1_log(w) >= F32(threshold)


# ---- G: LRT noise injection -------------------------------------------------------------------------------------------
G_SIZES = (1, 7, 8, 9, 2055, RP_L8 + 8 + 3, 2 * RP_L8 + 16)
G_FORMS = ("f32", "bf16", "bf16_s2")      # float32; bf16 with a float32 variance; bf16 with a bf16 variance
G_SPECIAL = (0.0, 0.99e-8, 1e-8, 1.01e-8)
G_COLS = ((2100, 2048), (65600, 64))      # reparam_bwd(bias_sums=): both beyond the wrap of the flat kernel
G_MAX = max(G_SIZES)
_GM = {}


def reparam_data(n):
    """float32 (mu_r, mu_i, s2, eps_r, eps_i, g_r, g_i): prefixes of one master draw; the clamp's special variances at
    the head and in the last 8-wide vector"""
    if not _GM:
        rs = _rs("G")
        for k in ("mu_r", "mu_i", "eps_r", "eps_i", "g_r", "g_i"):
            _GM[k] = rs.standard_normal(G_MAX).astype(F32)
        _GM["s2"] = np.exp(rs.uniform(-25, 2, G_MAX)).astype(F32)
    d = {k: v[:n] for k, v in _GM.items()}
    s2 = d["s2"].copy()
    sp = np.array(G_SPECIAL, F32)
    s2[:min(4, n)] = sp[:min(4, n)]
    if n >= 16:
        v0 = ((n >> 3) - 1) << 3
        s2[v0:v0 + 4] = sp
    d["s2"] = s2
    return d


def reparam_dtypes(form):
    """(operand dtype, variance dtype, g_s2 dtype)"""
    return {"f32": (_F, _F, _F), "bf16": (_B, _F, _F), "bf16_s2": (_B, _B, _B)}[form]


def reparam_ref(mu_r, mu_i, s2, eps_r, eps_i, g_r, g_i):
    """float64 (y_r, y_i, g_s2, sd) on operands already rounded to the kernel's dtypes; *_i None: the real form"""
    f = lambda t: None if t is None else np.asarray(t, np.float64)  # noqa: E731
    mu_r, mu_i, s2, eps_r, eps_i, g_r, g_i = map(f, (mu_r, mu_i, s2, eps_r, eps_i, g_r, g_i))
    sd = np.sqrt(np.maximum(s2, 1e-8))
    y_r = mu_r + eps_r * sd
    y_i = None if mu_i is None else mu_i + eps_i * sd
    gs = g_r * eps_r + (0 if g_i is None else g_i * eps_i)
    keep = s2 >= np.float64(F32(1e-8))    # the kernel's constant is the float32 1e-8
    return y_r, y_i, np.where(keep, 0.5 * gs / sd, 0.0), sd


def reparam_bounds(y_ref, gs2_ref, sd, g_r, g_i, form):
    """Philox forms: (bound on y, bound on g_s2); bf16 outputs add one rounding"""
    bf_y = EBF if form != "f32" else 0.0
    bf_g = EBF if form == "bf16_s2" else 0.0
    gabs = np.abs(np.asarray(g_r, np.float64)) + (0 if g_i is None else np.abs(np.asarray(g_i, np.float64)))
    return (NOISE_ATOL * sd + (E32 + bf_y) * np.abs(y_ref),
            0.5 * gabs * NOISE_ATOL / sd + (COLSUM + bf_g) * np.abs(gs2_ref))


def given_chain32(mu, eps, sd32):
    """the float32 chain of test_reparam_given_noise: one rounding per operation"""
    return np.asarray(mu, F32) + np.asarray(eps, F32) * sd32


GIVEN_TOL = {"f32": dict(rtol=1e-6, atol=1e-7), "bf16": dict(rtol=8e-3, atol=1e-6), "bf16_s2": dict(rtol=8e-3, atol=1e-6)}
GIVEN_GS2_TOL = dict(rtol=2e-6, atol=1e-30)
