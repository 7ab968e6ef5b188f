"""Case lists and helpers of the Welch sweep (test_welch_sweep_host.py, test_gpu_welch_sweep.py): the segment chunks of the
fused kernels, the vector batches of the workspace route, the gather of the backward at every kind of step, weak bands and
layouts of csrc/spectrum.hip.

The plan is RESTATED here from the kernel's documentation, not read from the library (the host test pins the library to it):
  M        n for a power of two, else Bluestein's 2^ceil(log2(2 n - 1)).
  fused    forward: M <= 2^14 (float32 / bf16 planes) or 2^13 (float64) for a power-of-two n, M <= 2^13 for Bluestein;
           backward: M <= 2^13 always.  Everything else goes through the workspace (four-step passes).
  chunks   a fused launch splits the S segments of a row: want = ceil(2048 / rows), chunks = min(S, want),
           G = ceil(S / chunks), chunks = ceil(S / G); chunk ch holds the segments ch G .. min(ch G + G, S) - 1.
  GL       the workspace route walks the rows * S segments ("vectors") in batches of
           GL = min(256 MiB / (2 M sizeof(C2)), rows * S, 65535).
  layout   [0, 256) window scale | twiddles al(M c) | Bluestein only: chirp al(n c), B-hat al(M c) | then either the fused
           buffers at once, or two batch buffers of al(GL M c) each first; forward: partial sums al(rows chunks n c / 2)
           (one chunk through the workspace), backward: D al(rows S n c).  c = sizeof(C2) = 8 or 16, al rounds up to 256.

Reference: the reference's formula -- unfold, times window, fft, abs ** 2, mean, over scale -- in complex128 on the CPU,
from the values the kernel is given (bf16 planes: from the rounded values); gradients by CPU autograd through it.
Bounds: the project's own (test_gpu_spectrum.py), applied norm-wise PER ROW: Pxx 1e-5 (float32, bf16 planes) and 1e-11
(float64); gradients 1e-4 and 1e-10.  A bf16 gradient is rounded to bf16 when it is stored, which no norm-wise 1e-4 can hold:
it is checked per entry against 2^-8 |ref| (half a bf16 ulp, the most that one rounding costs) + 1e-4 max|ref of the row|
(the float32 bound), as fft_cases.bf16_violations does for bf16 spectra.
"""
import functools
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
IDS = {F32: "f32", F64: "f64", BF16: "bf16"}
PXX_TOL = {F32: 1e-5, BF16: 1e-5, F64: 1e-11}
GRAD_TOL = {F32: 1e-4, F64: 1e-10}
BF16_GRAD = (2.0 ** -8, 1e-4)                             # per entry: |ref| factor, max|ref of the row| factor
HEADROOM = 0.25                                           # the complex64 CPU formula stays within a quarter of a bound

TARGET_WGS = 2048
LARGE_WS = 256 << 20
GL_CAP = 65535


# ---- the plan, restated ----------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def al256(b):
    return (b + 255) & ~255


def transform_size(n):
    if n & (n - 1) == 0:
        return n
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def csize(dtype):
    """sizeof(C2<T>): bf16 planes are computed in float32"""
    return 16 if dtype == F64 else 8


def fused(n, dtype):
    """(forward fused, backward fused)"""
    lg = transform_size(n).bit_length() - 1
    pow2 = transform_size(n) == n
    return lg <= ((13 if dtype == F64 else 14) if pow2 else 13), lg <= 13


def chunking(rows, S):
    """(want, G, chunks) of a fused launch"""
    want = ceil_div(TARGET_WGS, rows)
    chunks = min(S, want)
    G = ceil_div(S, chunks)
    return want, G, ceil_div(S, G)


def batch_limit(n, dtype):
    """GL before it is capped by the number of vectors"""
    return max(1, LARGE_WS // (2 * transform_size(n) * csize(dtype)))


def expected_plan(n, rows, S, dtype):
    """(path, forward workspace bytes, backward workspace bytes)"""
    M, c = transform_size(n), csize(dtype)
    pow2 = M == n
    f_fwd, f_bwd = fused(n, dtype)
    path = ("direct" if f_fwd else "four-step") if pow2 else ("bluestein" if f_fwd else "bluestein+four-step")
    off = 256 + al256(M * c)
    if not pow2:
        off += al256(n * c) + al256(M * c)
    _, _, chunks = chunking(rows, S)
    GL = min(batch_limit(n, dtype), rows * S, GL_CAP)
    after = off + 2 * al256(GL * M * c)
    fwd = (off if f_fwd else after) + al256(rows * (chunks if f_fwd else 1) * n * (c // 2))
    bwd = (off if f_bwd else after) + al256(rows * S * n * c)
    return path, fwd, bwd


def chunk_seams(rows, S):
    """which seams of the chunk rule a fused launch of (rows, S) crosses"""
    want, G, chunks = chunking(rows, S)
    hit = set()
    if G > 1:
        hit.add("G>1")
    if S % G:
        hit.add("part-chunk")
    if chunks > 1:
        hit.add("chunks>1")
    if chunks < min(S, want):
        hit.add("fewer-chunks")
    return frozenset(hit)


def batch_seams(n, rows, S, dtype):
    """which seams of the workspace loop a call crosses"""
    GL = batch_limit(n, dtype)
    hit = set()
    if rows * S > GL:
        hit.add("batches>1")
        if GL % S:
            hit.add("batch-ends-inside-a-row")
    return frozenset(hit)


def step_seam(n, step):
    """the gather seams `step` is (for small n one step is several of them)"""
    seams = (("step=n+3", n + 3), ("step=n", n), ("step=n-1", n - 1), ("step=1", 1))
    return frozenset(name for name, s in seams if step == s)


# ---- data and the reference ------------------------------------------------------------------------------------------
def gaussian(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, dtype=F64, generator=g)


def integers(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def window_scale(window, fs, scaling):
    return fs * (window ** 2).sum() if scaling == "density" else window.sum() ** 2


def ref_pxx(x, window, step, fs=1.0, scaling="density"):
    """the reference's formula along the last dim of a [rows, T] complex tensor, differentiable"""
    n = window.shape[0]
    xw = x.unfold(-1, n, step) * window
    return (torch.fft.fft(xw, dim=-1).abs() ** 2).mean(dim=-2) / window_scale(window, fs, scaling)


def ref_pxx_blocked(x, window, step, fs=1.0, scaling="density", rows_block=64):
    """ref_pxx a block of rows at a time (rows are independent): the same values without the whole unfolded block in
    memory"""
    return torch.cat([ref_pxx(x[r:r + rows_block], window, step, fs, scaling) for r in range(0, x.shape[0], rows_block)])


def ref_grad(x, window, g, step, fs=1.0, scaling="density"):
    """autograd through ref_pxx: d sum(Pxx g) / dx as dL/dre + i dL/dim"""
    xa = x.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(ref_pxx(xa, window, step, fs, scaling), xa, grad_outputs=g.to(x.real.dtype))
    return grad


def ref_grad_blocked(x, window, g, step, fs=1.0, scaling="density", rows_block=64, seg_block=64):
    """ref_grad in blocks of rows (independent) and of segments: the mean over segments is a sum, so the gradient is
    the sum of the gradients through each block of segments -- autograd through the same formula with bounded memory"""
    n = window.shape[0]
    rows, T = x.shape
    S = (T - n) // step + 1
    out = torch.zeros_like(x)
    for r in range(0, rows, rows_block):
        for a in range(0, S, seg_block):
            b = min(a + seg_block, S)
            lo, hi = a * step, (b - 1) * step + n
            part = ref_grad(x[r:r + rows_block, lo:hi], window, g[r:r + rows_block], step, fs, scaling)
            out[r:r + rows_block, lo:hi] += part * ((b - a) / S)
    return out


def per_row(got, ref):
    """the worst norm-wise error of one row (last dim) against its own reference"""
    got = got.detach().cpu().to(ref.dtype)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = torch.linalg.norm(ref, dim=-1)
    assert bool((den > 0).all())
    return float((torch.linalg.norm(got - ref, dim=-1) / den).max())


def bf16_grad_ratio(got, ref):
    """the worst ratio of an entry's error to BF16_GRAD's bound, per plane (got: complex or planes stacked last)"""
    worst = 0.0
    got = torch.view_as_real(got.detach().cpu().to(torch.complex128))
    ref = torch.view_as_real(ref)
    for k in (0, 1):
        bound = BF16_GRAD[0] * ref[..., k].abs() + BF16_GRAD[1] * ref[..., k].abs().amax(dim=-1, keepdim=True)
        worst = max(worst, float(((got[..., k] - ref[..., k]).abs() / bound).max()))
    return worst


# ---- 2. bit-exact cases ----------------------------------------------------------------------------------------------
# (rows, S) -> the chunk seams the pair crosses
EXACT_SHAPES = {
    (1024, 5): {"G>1", "part-chunk", "chunks>1"},                       # G = 3: chunks of 3 + 2
    (700, 7): {"G>1", "part-chunk", "chunks>1"},                        # G = 3: 3 + 3 + 1
    (700, 8): {"G>1", "part-chunk", "chunks>1"},                        # G = 3: 3 + 3 + 2; S a power of two
    (512, 10): {"G>1", "part-chunk", "chunks>1"},                       # G = 3: 4 chunks, the last holds 1
    (512, 9): {"G>1", "chunks>1", "fewer-chunks"},                      # want 4, G = 3: 3 full chunks
    (3, 1001): {"G>1", "part-chunk", "chunks>1", "fewer-chunks"},       # G = 2: 501 chunks of the 683 wanted
    (2048, 6): {"G>1"},                                                 # one chunk of all 6
    (2049, 6): {"G>1"},                                                 # want = ceil(2048 / 2049) = 1
    (1, 2049): {"G>1", "part-chunk", "chunks>1", "fewer-chunks"},       # G = 2: 1025 chunks
}
EXACT_N = (1, 2, 4)
EXACT_DTYPES = (F32, BF16, F64)


def exact_steps(n):
    """1, n - 1, n and n + 3 where they are valid and distinct"""
    return tuple(sorted({s for s in (1, n - 1, n, n + 3) if s >= 1}))


def exact_cases():
    """(rows, S, n, step): every shape at every n and step"""
    return tuple((rows, S, n, step) for (rows, S) in EXACT_SHAPES for n in EXACT_N for step in exact_steps(n))


def exact_id(case):
    rows, S, n, step = case
    return f"r{rows}-S{S}-n{n}-step{step}"


def exact_scaling(case):
    """(scaling, fs): the power-of-two scales n^2 and 2 n, alternating over the cases"""
    rows, S, n, step = case
    return ("spectrum", 1.0) if (rows + S + n + step) % 2 else ("density", 2.0)


def exact_length(case):
    """T: the S segments and a tail of step - 1 samples that no segment covers (the longest that starts no segment)"""
    rows, S, n, step = case
    return (S - 1) * step + n + step - 1


def coverage(T, n, step):
    """how many segments cover each of the T samples"""
    S = (T - n) // step + 1
    cov = torch.zeros(T, dtype=torch.int64)
    for s in range(S):
        cov[s * step:s * step + n] += 1
    return cov


def is_strict(case):
    """S a power of two (the scale of a window of ones always is one here): 1 / (S scale) is exact"""
    return case[1] & (case[1] - 1) == 0


@functools.lru_cache(maxsize=None)
def exact_reference(case):
    """(x complex128 [rows, T], g [rows, n], window of ones, Pxx accumulator, gradient accumulator (complex), S scale):
    integer planes in [-4, 4], integer g in [-4, 4]; the accumulators are the integers sum_s |X_s|^2 = Pxx S scale and
    grad S scale / 2, recovered from the float64 reference by rounding.  Computed once, shared and left unchanged."""
    rows, S, n, step = case
    T = exact_length(case)
    scaling, fs = exact_scaling(case)
    seed = 1000 * rows + 10 * S + n + 100 * step
    planes = integers((rows, T, 2), seed)
    x = torch.complex(planes[..., 0], planes[..., 1])
    g = integers((rows, n), seed + 1)
    w = torch.ones(n, dtype=F64)
    k = S * float(window_scale(w, fs, scaling))
    pxx = ref_pxx(x, w, step, fs, scaling) * k
    grad = ref_grad(x, w, g, step, fs, scaling) * (k / 2)
    return x, g, w, pxx, grad, k


def integer_dft_accumulator(x, n, step):
    """sum_s |DFT_n(x_s)|_k^2 in int64 arithmetic for n in {1, 2, 4}: the rotations are +-1 and +-i"""
    assert n in (1, 2, 4)
    xr, xi = x.real.round().long().unfold(-1, n, step), x.imag.round().long().unfold(-1, n, step)
    cos = {0: 1, 1: 0, 2: -1, 3: 0}
    acc = []
    for k in range(n):
        # e^{-2 pi i j k / n} = cos - i sin with angles in quarter turns q = (j k mod n) 4 / n
        q = [(j * k % n) * 4 // n for j in range(n)]
        c = torch.tensor([cos[v] for v in q])
        s = torch.tensor([cos[(v - 1) % 4] for v in q])                 # sin(q) = cos(q - 1)
        re = (xr * c + xi * s).sum(-1)
        im = (xi * c - xr * s).sum(-1)
        acc.append((re * re + im * im).sum(-1))
    return torch.stack(acc, -1)


# ---- layouts ---------------------------------------------------------------------------------------------------------
# name -> whether the planes are copied first (the documented case: the dims other than time do not collapse into one
# row stride)
LAYOUTS = {"interleaved": False, "real-pairs": False, "planes": False, "strided-time": False, "time-in-the-middle": False,
           "transposed-batch": True, "time-in-the-middle-of-two-batch-dims": True}
LAYOUT_ROWS, LAYOUT_T = 6, 300


def layout(name, x):
    """dense complex [6, T] x -> (pr, pi, dim, unbatch): planes holding the same rows behind layout `name`, the time dim,
    and unbatch(Pxx) -> [6, n].  Works on any device."""
    R, T = x.shape
    flat = lambda y: y.reshape(R, -1)  # noqa: E731
    if name == "interleaved":
        v = torch.view_as_real(x.contiguous())
        return v[..., 0], v[..., 1], 1, flat
    if name == "real-pairs":                              # a [..., T, 2] real tensor that never was complex
        v = torch.stack([x.real, x.imag], dim=-1)
        return v[..., 0], v[..., 1], 1, flat
    if name == "planes":
        return x.real.contiguous(), x.imag.contiguous(), 1, flat
    if name == "strided-time":                            # every third element of planes three times as long
        buf = torch.zeros(2, R, 3 * T, dtype=x.real.dtype, device=x.device)
        buf[0, :, ::3], buf[1, :, ::3] = x.real, x.imag
        return buf[0, :, ::3], buf[1, :, ::3], 1, flat
    if name == "time-in-the-middle":                      # [1, T, 3, 2]: element stride 6, rows next to each other
        v = torch.view_as_real(x.t().reshape(1, T, 3, 2).contiguous())
        return v[..., 0], v[..., 1], 1, lambda y: y.reshape(R, -1)
    if name == "transposed-batch":                        # [2, 3, T] stored as [3, 2, T]
        v = torch.view_as_real(x.reshape(2, 3, T).transpose(0, 1).contiguous().transpose(0, 1))
        assert not v.is_contiguous()
        return v[..., 0], v[..., 1], 2, flat
    if name == "time-in-the-middle-of-two-batch-dims":    # [2, T, 3, 1]
        v = torch.view_as_real(x.reshape(2, 3, T).permute(0, 2, 1).reshape(2, T, 3, 1).contiguous())
        return v[..., 0], v[..., 1], 1, flat
    raise KeyError(name)


# ---- 3. toleranced seams on the real transforms ----------------------------------------------------------------------
# (name, n, rows, S, plane dtypes of the forward, of the backward); step = 1, so T = n + S - 1
FUSED_CASES = (
    ("direct-1024", 1024, 1024, 5, (F32, BF16, F64), (F32, BF16, F64)),
    ("direct-16384", 16384, 1024, 5, (F32, BF16), ()),                  # fused in the float32 forward only
    ("bluestein-500", 500, 1024, 5, (F32, BF16, F64), (F32, BF16, F64)),
    ("bluestein-4095", 4095, 1024, 5, (F32, BF16, F64), (F32, BF16, F64)),
)
WORKSPACE_CASES = (
    ("four-step-32768", 32768, 2, 300, (F32,), ()),                     # GL = 512
    ("four-step-16384-S600", 16384, 2, 600, (), (F32,)),                # GL = 1024: float32 leaves LDS only backwards
    ("four-step-16384-S300", 16384, 2, 300, (F64,), (F64,)),            # GL = 512
    ("bluestein-four-step-8193", 8193, 2, 300, (F32,), (F32,)),         # M = 32768: GL = 512
)
TOL_CASES = FUSED_CASES + WORKSPACE_CASES
TOL_FS, TOL_SCALING = 2.0, "density"


def tol_runs(which):
    """(case, dtype) of every toleranced forward (which = 4) or backward (5) run"""
    return tuple((c, d) for c in TOL_CASES for d in c[which])


def tol_id(run):
    return f"{run[0][0]}-{IDS[run[1]]}"


def value_dtype(dtype):
    """the dtype the values of a run are rounded to: float64 planes hold the float32 run's values, so the two share one
    reference"""
    return BF16 if dtype == BF16 else F32


@functools.lru_cache(maxsize=None)
def tol_input(name, narrow):
    """(x complex128 of the rounded values [rows, T], window (float32 values) float64, g [rows, n] (float32 values))"""
    case = next(c for c in TOL_CASES if c[0] == name)
    _, n, rows, S, _, _ = case
    T = n + S - 1
    vd = BF16 if narrow else F32
    planes = gaussian((2, rows, T), seed=n + S).to(vd).to(F64)
    w = torch.hamming_window(n, periodic=False, dtype=F64).to(F32).to(F64)
    g = gaussian((rows, n), seed=n + S + 1).to(F32).to(F64)
    return torch.complex(planes[0], planes[1]), w, g


@functools.lru_cache(maxsize=None)
def tol_pxx(name, narrow):
    x, w, _ = tol_input(name, narrow)
    return ref_pxx_blocked(x, w, 1, TOL_FS, TOL_SCALING)


@functools.lru_cache(maxsize=None)
def tol_grad(name, narrow):
    x, w, g = tol_input(name, narrow)
    return ref_grad_blocked(x, w, g, 1, TOL_FS, TOL_SCALING)


# ---- 4. weak bands ---------------------------------------------------------------------------------------------------
# Two rows of T samples at fs = 1000: a unit tone at +-fs / 8 = 125 (on a bin of both segment lengths, 1000 and 1024:
# the main channel holds it whole), band-limited Gaussian noise in three adjacent channels 40, 60 and 80 dB below it, and
# a white floor of -120 dB in all.  Band edges lie at x.37: never on a bin of either length, so float32 and float64
# frequencies select the same bins.
BAND_FS, BAND_T = 1000.0, 8192
BAND_NPERSEG = (1000, 1024)
BAND_LEVELS_DB = (-40.0, -60.0, -80.0)
BAND_MCB, BAND_ACB = 20.0, 20.0
BAND_ROWS = ((125.0, (165.0, 205.0, 245.0)), (-125.0, (-205.0, -165.0, -245.0)))     # (mcf, acf of -40, -60, -80 dB)
BAND_OFFSET = 0.37
BAND_DTYPES = (F32, F64)
BAND_EPS = {F32: 1e-5, F64: 1e-11}                        # the amplitude tolerances behind PXX_TOL
BAND_LEVEL_SLACK_DB = 1.5


def band_edges(row):
    """[(lo, hi)]: the main channel, then the adjacent ones, of a row"""
    mcf, acf = BAND_ROWS[row]
    return [(f - BAND_MCB / 2 + BAND_OFFSET, f + BAND_MCB / 2 + BAND_OFFSET) for f in (mcf,) + tuple(acf)]


@functools.lru_cache(maxsize=None)
def band_signal():
    """[2, T] complex128 of float32 values (so float32 and float64 planes hold the same signal)"""
    T, fs = BAND_T, BAND_FS
    t = torch.arange(T, dtype=F64)
    freq = torch.fft.fftfreq(T, 1.0 / fs).to(F64)
    rows = []
    for r, (mcf, acf) in enumerate(BAND_ROWS):
        x = torch.exp(2j * math.pi * mcf / fs * t)
        for k, (f, db) in enumerate(zip(acf, BAND_LEVELS_DB)):
            # noise on the frequencies of the length-T grid well inside the channel (3 off each edge)
            lo, hi = band_edges(r)[1 + k]
            inside = (freq > lo + 3) & (freq < hi - 3)
            z = gaussian((2, T), seed=10 * r + k)
            spec = torch.complex(z[0], z[1]) * inside
            noise = torch.fft.ifft(spec)
            # (the window widens a channel's summed spectrum by the same factor for the tone and for the noise)
            noise = noise * math.sqrt(10 ** (db / 10) / float((noise.abs() ** 2).mean()))
            x = x + noise
        z = gaussian((2, T), seed=100 + r)
        x = x + torch.complex(z[0], z[1]) * math.sqrt(0.5e-12)
        rows.append(x)
    x = torch.stack(rows)
    return torch.complex(x.real.to(F32).to(F64), x.imag.to(F32).to(F64))


def band_select(nperseg, bands, dtype=F64):
    """the reference's selection: nonzero(ff > lo & ff < hi) on fftshift(fftfreq) in `dtype` -> [index tensors]"""
    k = torch.arange(nperseg)
    ff = torch.where(k < (nperseg - 1) // 2 + 1, k, k - nperseg).to(F64) * (1.0 / (nperseg * (1.0 / BAND_FS)))
    ff = torch.roll(ff.to(dtype), nperseg // 2)
    return [torch.nonzero(ff.gt(lo) & ff.lt(hi), as_tuple=True)[0] for lo, hi in bands]


def band_powers(pxx_shifted, nperseg, dtype=F64):
    """[2, 4] linear band powers (summed in float64) of a shifted [2, nperseg] spectrum"""
    p = pxx_shifted.detach().cpu().to(F64)
    return torch.stack([torch.stack([p[r, idx].sum() for idx in band_select(nperseg, band_edges(r), dtype)])
                        for r in range(2)])


def band_ref_pxx(x, nperseg, n_overlap, scaling, cdtype=torch.complex128):
    """the reference's bandwidth_power spectrum (Hamming window, fftshift) of x in `cdtype` on the CPU"""
    w = torch.hamming_window(nperseg, periodic=False, dtype=F64 if cdtype == torch.complex128 else F32)
    p = ref_pxx(x.to(cdtype), w, nperseg - n_overlap, BAND_FS, scaling)
    return torch.roll(p, nperseg // 2, -1)


def band_bound(p_band, p_total, eps):
    """|dP_B| <= 2 eps sqrt(P_B P_tot) + eps^2 P_tot.  With d the error of the windowed spectra of all segments and
    |d| <= eps |X| norm-wise, dP_B = sum_B (2 Re X conj d + |d|^2) <= 2 |X_B| |d| + |d|^2 by Cauchy-Schwarz; the sums over
    segments and the common 1 / (S scale) turn |X_B|^2 and |X|^2 into P_B and P_tot."""
    return 2 * eps * torch.sqrt(p_band * p_total) + eps ** 2 * p_total


# (function, nperseg): bandwidth_power with its defaults (overlap n / 2, density) and acpr_calc (no overlap, spectrum)
BAND_RUNS = tuple((fn, n) for fn in ("bandwidth_power", "acpr_calc") for n in BAND_NPERSEG)


def band_run_params(fn, nperseg):
    """(n_overlap, scaling) of the Welch call behind `fn`"""
    return (nperseg // 2, "density") if fn == "bandwidth_power" else (0, "spectrum")
