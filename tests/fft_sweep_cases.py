"""Case lists and helpers of the FFT engine sweep (test_fft_sweep_host.py, test_gpu_fft_sweep.py): every transform length
csrc/fft_engine.h is compiled for, and every route that is not the packed workgroup under every layout, padding, scale,
dtype pair and batch seam.  Generators, the reference (torch.fft in complex128 on the CPU, from the values the kernel was
given) and the bounds are fft_cases.py's and rfft_cases.py's; the sweep applies the bounds PER VECTOR.

Three primitives are swept (`kind`): "c2c" (fft.transform), "r2c" and "c2r" (rfft.r2c unweighted, rfft.c2r weighted: what
rfft / ihfft and irfft / hfft run).  `positive` is the sign of the exponent.
"""
import functools

import torch

import fft_cases as fc
import rfft_cases as rc
from cplxmodule_amd import fft as hostfft
from cplxmodule_amd import rfft as hostrfft

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
WIDE = (F32, F64)
IDS = {F32: "f32", F64: "f64", BF16: "bf16"}
KINDS = ("c2c", "r2c", "c2r")


def log2(m):
    assert m & (m - 1) == 0
    return m.bit_length() - 1


# ---- 1. every compiled size ------------------------------------------------------------------------------------------
DIRECT = tuple(1 << l for l in range(0, 15))              # float64 runs 2^14 in four steps (halves 7, 7)
FOUR_STEP = tuple(1 << l for l in range(15, 23))          # halves (8,7) (8,8) (9,8) (9,9) (10,9) (10,10) (11,10) (11,11)


def bluestein_ends(m):
    """both ends of the range of n whose Bluestein transform has 2^m points: 2^(m-1) < 2n - 1 <= 2^m"""
    return tuple(sorted({(1 << (m - 2)) + 1, (1 << (m - 1)) - 1}))


BLUESTEIN = tuple(n for m in range(3, 16) for n in bluestein_ends(m))     # 3 .. 13 fused, 14 and 15 through the workspace
FFT_LENGTHS = DIRECT + FOUR_STEP + BLUESTEIN
# the half-length route: n = 2 L for every complex length L above (L = 2^22 would be n = 2^23, beyond the longest
# transform); the full-length route: the odd lengths of the Bluestein list (every one of them is odd)
RFFT_LENGTHS = tuple(2 * L for L in FFT_LENGTHS if 2 * L <= hostfft.MAX_N) + BLUESTEIN


def vectors(n):
    return 1 if n >= 1 << 20 else 3


def expected_fft_plan(n, dtype):
    """(path, vectors per workgroup) as csrc/fft.hip documents them, NOT read from the library: LDS holds 2^14 float32 or
    2^13 float64 points, a fused Bluestein pair 2^13 of either, the packed workgroup 2^10"""
    m = fc.transform_size(n)
    blue = m != n
    lds = log2(m) <= (13 if blue or dtype == F64 else 14)
    path = ("bluestein" if lds else "bluestein+four-step") if blue else ("direct" if lds else "four-step")
    return path, fc.vectors_per_workgroup(n)


def expected_rfft_plan(n, dtype):
    """(path, complex length, points run, vectors per workgroup)"""
    cn = rc.complex_length(n)
    path, vpw = expected_fft_plan(cn, dtype)
    return path, cn, fc.transform_size(cn), vpw


def halves(points, dtype):
    """the (logN1, logN2) of fft_vectors' two passes for a transform of `points` through the workspace; None in LDS"""
    lg = log2(points)
    return ((lg + 1) // 2, lg // 2) if lg > (13 if dtype == F64 else 14) else None


def per_vector(got, ref):
    """the worst norm-wise error of ONE vector (along the last dim) against its own reference.  got: planes (re, im), a
    Cplx, or a real tensor; ref: complex128 / float64 on the CPU"""
    if hasattr(got, "real") and not torch.is_tensor(got):
        got = (got.real, got.imag)
    if isinstance(got, tuple):
        got = fc.c128(*got) if len(got) == 2 else got[0]
    got = got.detach().cpu().to(ref.dtype)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = torch.linalg.norm(ref, dim=-1)
    assert bool((den > 0).all())
    return float((torch.linalg.norm(got - ref, dim=-1) / den).max())


# ---- 2. every route that is not the packed workgroup -----------------------------------------------------------------
# (route, n, dtype): the smallest length that reaches the route
C2C_ROUTES = (
    ("one-vector", 2048, F32), ("one-vector", 2048, F64), ("one-vector-32-per-lane", 16384, F32),
    ("one-vector-16-per-lane", 8192, F64),
    ("fused-bluestein-4096", 1025, F32), ("fused-bluestein-4096", 1025, F64),
    ("fused-bluestein-8192", 2049, F32), ("fused-bluestein-8192", 2049, F64),
    ("workspace-four-step", 32768, F32), ("workspace-four-step", 16384, F64),
    ("workspace-bluestein", 4097, F32), ("workspace-bluestein", 4097, F64),
)
REAL_ROUTES = (
    ("one-vector", 4096, F32), ("one-vector", 4096, F64), ("one-vector-32-per-lane", 32768, F32),
    ("fused-bluestein-4096", 2050, F32), ("fused-bluestein-4096", 2050, F64),
    ("fused-bluestein-8192", 4098, F32), ("fused-bluestein-8192", 4098, F64),
    ("fused-bluestein-8192-odd", 2049, F32), ("fused-bluestein-8192-odd", 2049, F64),
    ("workspace-four-step", 65536, F32), ("workspace-four-step", 32768, F64),
    ("workspace-bluestein", 8194, F32), ("workspace-bluestein", 8194, F64),
    ("workspace-bluestein-odd", 4097, F32), ("workspace-bluestein-odd", 4097, F64),
)
# route -> (path, points run by the complex transform)
ROUTE_PLAN = {
    "one-vector": ("direct", 2048), "one-vector-32-per-lane": ("direct", 16384), "one-vector-16-per-lane": ("direct", 8192),
    "fused-bluestein-4096": ("bluestein", 4096), "fused-bluestein-8192": ("bluestein", 8192),
    "fused-bluestein-8192-odd": ("bluestein", 8192), "workspace-four-step": ("four-step", None),
    "workspace-bluestein": ("bluestein+four-step", 16384), "workspace-bluestein-odd": ("bluestein+four-step", 16384),
}
ROUTES = tuple(("c2c",) + r for r in C2C_ROUTES) + tuple((k,) + r for k in ("r2c", "c2r") for r in REAL_ROUTES)


def route_id(case):
    kind, route, n, dtype = case
    return f"{kind}-{route}-{n}-{IDS[dtype]}"


B = 6                                                     # vectors of a baseline run: 2 x 3


def in_len(kind, n):
    return n // 2 + 1 if kind == "c2r" else n


def out_len(kind, n):
    return n // 2 + 1 if kind == "r2c" else n


def planes(kind, shape, dtype, seed):
    """input planes on the CPU: (re, im), or (x,) for r2c; half spectra keep non-zero DC and Nyquist imaginary parts"""
    if kind == "r2c":
        return (rc.real_gaussian(shape, dtype, seed),)
    return rc.half_spectrum(shape, dtype, seed) if kind == "c2r" else fc.gaussian(shape, dtype, seed)


def default_sign(kind):
    return kind == "c2r"                                  # fft, rfft: e^-; irfft: e^+


def run(kind, xs, n, dim=-1, positive=None, scale=1.0, out_dtype=None):
    """the primitive along `dim` of planes on the device -> tuple of output planes"""
    positive = default_sign(kind) if positive is None else positive
    out_dtype = xs[0].dtype if out_dtype is None else out_dtype
    dim %= xs[0].dim()
    if kind == "c2c":
        return tuple(hostfft.transform(xs[0], xs[1], n, dim, positive, scale, out_dtype))
    if kind == "r2c":
        return tuple(hostrfft.r2c(xs[0], n, dim, positive, False, scale, out_dtype))
    return (hostrfft.c2r(xs[0], xs[1], n, dim, positive, True, scale, out_dtype),)


def reference(kind, xs, n, positive=None, scale=1.0):
    """the same in complex128 / float64 on the CPU, along the last dim, from the planes' values"""
    positive = default_sign(kind) if positive is None else positive
    if kind == "c2c":
        z = fc.c128(*xs)
        ref = torch.fft.ifft(z, n=n, norm="forward") if positive else torch.fft.fft(z, n=n)
    elif kind == "r2c":
        ref = torch.fft.rfft(xs[0].detach().double().cpu(), n=n)
        ref = ref.conj().resolve_conj() if positive else ref
    else:
        z = fc.c128(*xs)
        ref = torch.fft.irfft(z, n=n, norm="forward") if positive else torch.fft.hfft(z, n=n)
    return ref * scale


@functools.lru_cache(maxsize=None)
def baseline_input(kind, n, dtype):
    """the B Gaussian vectors of a route's baseline, on the CPU: computed once, shared and left unchanged"""
    return planes(kind, (B, in_len(kind, n)), dtype, seed=7 * n + KINDS.index(kind))


def _dense_out_strides(kind, view, n, dim):
    return hostfft._dense_like(view, dim, out_len(kind, n))[1]


def runs_of(kind, view, n, dim):
    """the batch runs fft.py / rfft.py give a launch on `view` along `dim`"""
    dim %= view.dim()
    return hostfft._runs(view.shape, view.stride(), _dense_out_strides(kind, view, n, dim), dim)


def takes_no_copy(kind, views, n, dim):
    """the condition of the no-copy branch of fft.transform / rfft.r2c / rfft.c2r: one layout, at most three runs"""
    return all(v.stride() == views[0].stride() for v in views) and len(runs_of(kind, views[0], n, dim)) <= 3


# name -> (batch runs of the launch, copies of the B vectors in the result)
LAYOUTS = {"dim0": (1, 1), "middle": (2, 1), "step2": (1, 1), "channels-last": (2, 1), "transposed": (1, 1),
           "runs-2": (2, 1), "runs-3": (3, 2), "expanded": (2, 4)}


def layout(name, x):
    """dense [B, L] plane x -> (view holding the same vectors behind layout `name`, dim to transform, unbatch), where
    unbatch(y) is the result as [copies, B, n_out].  Works on any device."""
    L = x.shape[1]
    z = lambda *shape: torch.zeros(*shape, dtype=x.dtype, device=x.device)  # noqa: E731
    if name == "dim0":                                    # element stride B, vectors next to each other
        return x.t().contiguous(), 0, lambda y: y.t().unsqueeze(0)
    if name == "middle":                                  # [2, L, 3]: element stride 3, runs of stride 3 L and 1
        return x.reshape(2, 3, L).permute(0, 2, 1).contiguous(), 1, lambda y: y.permute(0, 2, 1).reshape(1, B, -1)
    if name == "step2":                                   # every second element of a buffer twice as long
        buf = z(B, 2 * L)
        buf[:, ::2] = x
        return buf[:, ::2], 1, lambda y: y.unsqueeze(0)
    if name == "channels-last":                           # [1, 2, 3, L]: element stride 2
        v = x.reshape(1, 2, 3, L).contiguous(memory_format=torch.channels_last)
        assert v.stride(3) == 2 and v.stride(1) == 1
        return v, 3, lambda y: y.reshape(1, B, -1)
    if name == "transposed":                              # [1, 2, 3, L] stored as [1, L, 3, 2]: element stride B
        v = x.reshape(1, 2, 3, L).transpose(1, 3).contiguous().transpose(1, 3)
        assert v.stride(3) == B
        return v, 3, lambda y: y.reshape(1, B, -1)
    if name == "runs-2":                                  # three of four rows: the batch dims do not fuse
        buf = z(2, 4, L)
        buf[:, :3] = x.reshape(2, 3, L)
        return buf[:, :3], 2, lambda y: y.reshape(1, B, -1)
    if name == "runs-3":
        buf = z(2, 3, 4, L)
        buf[:, :2, :3] = x.reshape(1, 2, 3, L)
        return buf[:, :2, :3], 3, lambda y: y.reshape(2, B, -1)
    if name == "expanded":                                # input stride 0 along the leading dim
        return x.reshape(1, B, L).expand(4, B, L), 2, lambda y: y.reshape(4, B, -1)
    raise KeyError(name)


# ---- the batch seam of the workspace loop ----------------------------------------------------------------------------
# GL = min(256 MiB / (2 M sizeof(C2<T>)), vectors, 65535) vectors go through the workspace at a time.  The cap at 65535
# cannot bind: M >= 2^14 on this route, so the first term is at most 1024.
# (kind, n, dtype, GL)
SEAMS = (
    ("c2c", 32768, F32, 512), ("c2c", 16384, F64, 512), ("c2c", 4097, F32, 1024),
    ("r2c", 65536, F32, 512), ("r2c", 32768, F64, 512), ("r2c", 8194, F32, 1024), ("r2c", 4097, F32, 1024),
    ("c2r", 65536, F32, 512), ("c2r", 32768, F64, 512), ("c2r", 8194, F32, 1024), ("c2r", 4097, F32, 1024),
)
# batch -> distinct vectors d: the batch is d vectors expanded over a leading dim of batch / d, so d divides the batch;
# d does not divide GL (a power of two), so a dropped v0 lands on a different vector
CYCLE = {513: 9, 1027: 13, 1025: 5, 2051: 7}


def seam_batches(GL):
    return (GL + 1, 2 * GL + 3)


def seam_id(case):
    kind, n, dtype, GL = case
    return f"{kind}-{n}-{IDS[dtype]}-GL{GL}"


def workspace_bytes(kind, n, batch, dtype):
    return hostfft.plan(n, batch, dtype)[2] if kind == "c2c" else hostrfft.plan(n, batch, dtype, kind == "c2r")[4]


# the grid of the one-vector-per-workgroup kernel is one-dimensional: 65537 workgroups (a prime: one vector, expanded)
# and 9363 x 7 = 65541 (seven vectors, expanded)
GRID_BATCHES = ((1, 1), (2, 2), (65537, 1), (65541, 7))   # (vectors, distinct vectors)
GRID_CASES = (("c2c", 2048, F32), ("r2c", 4096, F32), ("c2r", 4096, F32))
