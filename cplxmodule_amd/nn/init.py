"""Parameter initialisers: the eight names of cplxmodule/nn/init.py, and `cplx_polar_factor`.

Restates the observable behaviour of cplxmodule/nn/init.py:12-130, including the reference's fan quirk: for 2-d weights
`get_fans` reports fan_in = shape[0] (the OUTPUT size), which is what the bias bound of CplxLinear ends up using.

`cplx_trabelsi_independent_` (the orthogonal initialiser of Deep Complex Networks, Trabelsi et al. 2018) differs from the
reference on purpose.  The reference draws Z with numpy, takes a HOST numpy.linalg.svd(full_matrices=True) of it -- single
threaded, O(n^3), minutes for a 4096 x 4096 layer -- and keeps U_k V[:k, :].  Here the semi-unitary factor is the unitary
polar factor U V^H of Z, computed WITHOUT an SVD by the Newton-Schulz recurrence X <- X (1.5 I - 0.5 X^H X), which needs
two complex GEMMs per step and nothing else.

Two routes run the same recurrence with the same stopping rule:
  * device tensors: the library's complex GEMMs (exact float32: ops.cgemm; float64: cplxamd_gemm_f64) and the three
    finishing kernels of csrc/init.hip, on the current stream, one scalar read back per step;
  * host tensors: plain torch ops on complex tensors.  This is the HOST TWIN of the device route -- parameters are normally
    initialised before `.to(device)`, as with every other initialiser here -- and NOT a fallback: a device tensor never
    takes it, and a missing kernel is an error.
"""
import math

import torch

from .. import _lib, ops
from .._lib import CplxAmdError, call, ptr, stream_ptr
from ..cplx import Cplx

__all__ = ["get_fans", "cplx_kaiming_normal_", "cplx_xavier_normal_", "cplx_kaiming_uniform_", "cplx_xavier_uniform_",
           "cplx_trabelsi_standard_", "cplx_trabelsi_independent_", "cplx_uniform_independent_", "cplx_polar_factor"]


def get_fans(cplxtensor):
    shape = tuple(cplxtensor.shape)
    if len(shape) < 2:
        raise ValueError("Fan in and fan out can not be computed for tensor with "
                         "fewer than 2 dimensions.")
    if len(shape) == 2:
        return shape[0], shape[1]
    field = 1
    for s in shape[2:]:
        field *= s
    return shape[1] * field, shape[0] * field


def cplx_kaiming_normal_(tensor, a=0.0, mode="fan_in", nonlinearity="leaky_relu"):
    """Independent Kaiming-normal planes with the slope widened to sqrt(1 + 2 a^2), i.e. each plane carries half of the
    complex variance."""
    assert isinstance(tensor, Cplx)
    get_fans(tensor)
    slope = math.sqrt(1 + 2 * a * a)
    for plane in (tensor.real, tensor.imag):
        torch.nn.init.kaiming_normal_(plane, a=slope, mode=mode, nonlinearity=nonlinearity)
    return tensor


def cplx_xavier_normal_(tensor, gain=1.0):
    """Independent Xavier-normal planes, each with gain / sqrt 2."""
    assert isinstance(tensor, Cplx)
    get_fans(tensor)
    for plane in (tensor.real, tensor.imag):
        torch.nn.init.xavier_normal_(plane, gain=gain / math.sqrt(2))
    return tensor


def cplx_kaiming_uniform_(tensor, a=0.0, mode="fan_in", nonlinearity="leaky_relu"):
    """Independent Kaiming-uniform planes with the slope widened to sqrt(1 + 2 a^2), i.e. each
    plane carries half of the complex variance."""
    assert isinstance(tensor, Cplx)
    slope = math.sqrt(1 + 2 * a * a)
    for plane in (tensor.real, tensor.imag):
        torch.nn.init.kaiming_uniform_(plane, a=slope, mode=mode, nonlinearity=nonlinearity)
    return tensor


def cplx_xavier_uniform_(tensor, gain=1.0):
    """Independent Xavier-uniform planes, each with gain / sqrt 2."""
    assert isinstance(tensor, Cplx)
    get_fans(tensor)
    for plane in (tensor.real, tensor.imag):
        torch.nn.init.xavier_uniform_(plane, gain=gain / math.sqrt(2))
    return tensor


def cplx_uniform_independent_(tensor, a=0.0, b=1.0):
    for plane in (tensor.real, tensor.imag):
        torch.nn.init.uniform_(plane, a, b)
    return tensor


def _trabelsi_scale(cplx, kind):
    """1 / sqrt(fan_in + fan_out) (glorot / xavier) or 1 / sqrt(fan_in) (kaiming / he), nn/init.py:69-76, 111-115."""
    kind = kind.lower()
    assert kind in ("glorot", "xavier", "kaiming", "he")
    fan_in, fan_out = get_fans(cplx)
    return 1 / math.sqrt(fan_in + fan_out) if kind in ("glorot", "xavier") else 1 / math.sqrt(fan_in)


def cplx_trabelsi_standard_(cplx, kind="glorot"):
    """Standard complex initialization proposed in Trabelsi et al. (2018).

    The reference draws rho ~ Rayleigh(scale) and theta ~ U(-pi, pi) and writes rho cos theta, rho sin theta
    (nn/init.py:78-85).  That is exactly the Box-Muller construction of two independent normal variates: with
    rho = scale sqrt(-2 log u), (rho cos theta, rho sin theta) are i.i.d. N(0, scale^2).  So the two planes are filled with
    `normal_(0, scale)` from the generator of the tensor's own device (torch.manual_seed reproduces it; the reference
    used numpy's global generator, whose stream cannot be matched)."""
    scale = _trabelsi_scale(cplx, kind)
    with torch.no_grad():
        cplx.real.normal_(0.0, scale)
        cplx.imag.normal_(0.0, scale)
    return cplx


# ------------------------------------------------------------------------------------------ #
#  the unitary polar factor by Newton-Schulz                                                 #
# ------------------------------------------------------------------------------------------ #
_MAX_STEPS = 100
_MAX_DRAWS = 16              # draws of Z in cplx_trabelsi_independent_: 0.09^16 even at 16384 x 16384 in float32
_THRESHOLD = 1e-3            # ||X^H X - I||_F at which the iteration is in its quadratic regime
_EXTRA = {torch.float32: 2, torch.float64: 3}      # further steps once below the threshold: 0.75 r^2 per step
_ROUNDOFF = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def _step_cap(dtype):
    """Steps within which the residual must reach the threshold.  A singular value s of X_0 = X / ||X||_F grows by 1.5 per
    step while it is small, so it needs log_1.5(1 / s) steps to come near 1.  s below the unit roundoff u means that X is
    within its own rounding error of a rank-deficient matrix -- and for an exactly rank-deficient one the null direction
    is fed by rounding noise of that size, which the recurrence would amplify into an arbitrary 'factor' after a few steps
    more.  So the cap is log_1.5(1 / u) steps (42 in float32, 91 in float64), and never more than 100."""
    return min(_MAX_STEPS, math.ceil(math.log(1 / _ROUNDOFF[dtype]) / math.log(1.5)))


class _NotConverged(CplxAmdError):
    """The step cap was reached: the one failure a fresh random draw cures (`cplx_trabelsi_independent_`)."""


def _check_start(m2, status=0.0):
    if not math.isfinite(m2):
        raise CplxAmdError("cplx_polar_factor: the input contains a non-finite value (or its squares overflow)")
    if m2 <= 0.0 or status != 0.0:
        raise CplxAmdError("cplx_polar_factor: the input is all zero, it has no polar factor")


def _check_residual(r2, step, cap):
    """True once below the threshold; raises on a non-finite residual or past the cap."""
    if not math.isfinite(r2):
        raise CplxAmdError(f"cplx_polar_factor: non-finite residual at step {step}")
    if math.sqrt(r2) <= _THRESHOLD:
        return True
    if step >= cap:
        raise _NotConverged(f"cplx_polar_factor: not converged after {step} steps (||X^H X - I||_F = {math.sqrt(r2):.3g}): "
                           "the input is rank-deficient to working precision")
    return False


def _polar_host(zr, zi):
    """Host twin of `_polar_device`: the same recurrence in torch ops on a complex tensor.  Returns (X, wide, steps) with X
    [n, k], n >= k; the factor is X, or X^H when `wide`."""
    z = torch.complex(zr, zi)
    wide = z.shape[0] < z.shape[1]
    x = z.mH.contiguous() if wide else z
    m2 = float((x.real * x.real + x.imag * x.imag).sum(dtype=torch.float64))
    _check_start(m2)
    x = x * (1.0 / math.sqrt(m2))
    eye = torch.eye(x.shape[1], dtype=x.dtype)
    cap, left, step = _step_cap(zr.dtype), None, 0
    while left is None or left > 0:
        step += 1
        g = x.mH @ x
        d = g - eye
        if left is None:
            if _check_residual(float((d.real * d.real + d.imag * d.imag).sum(dtype=torch.float64)), step, cap):
                left = _EXTRA[zr.dtype] + 1
        x = x @ (eye - 0.5 * d)                      # 1.5 I - 0.5 G
        left = None if left is None else left - 1
    return x, wide, step


def _plane_code(t):
    return _lib.F32 if t.dtype == torch.float32 else _lib.F64


def _cgemm_into(ar, ai, a_strides, br, bi, b_strides, M, N, K, conj_b, cr, ci):
    """C[m, n] = sum_k A[m, k] op(B[n, k]) into the given dense planes: exact float32 or float64.  The float64 branch is
    `f64._gemm`'s call of cplxamd_gemm_f64 (one 2-d product, no batch, no bias) without its allocation of C per call:
    the loop's temporaries are allocated once."""
    if ar.dtype == torch.float32:
        ops.cgemm(ar, ai, a_strides, br, bi, b_strides, M, N, K, conj_b=conj_b, out=(cr, ci))
    else:
        call("cplxamd_gemm_f64", ptr(ar), ptr(ai), a_strides[0], a_strides[1], 0, ptr(br), ptr(bi), b_strides[0], b_strides[1],
             0, None, None, ptr(cr), ptr(ci), N, M * N, 1, M, N, K, int(conj_b), stream_ptr())


def _polar_device(zr, zi):
    """The recurrence on dense float32 / float64 device planes [rows, cols].  Returns (xr, xi, wide, steps, stat, ws): X
    [n, k] with n >= k, the factor being X (or X^H when `wide`); `stat` / `ws` are the float64 scalars and the reduction
    workspace, handed on to the caller's finishing kernels."""
    rows, cols = zr.shape
    wide = rows < cols
    n, k = max(rows, cols), min(rows, cols)
    dev, dt, code = zr.device, zr.dtype, _plane_code(zr)
    ws = torch.empty(int(_lib.load().cplxamd_init_ws_bytes()), dtype=torch.uint8, device=dev)
    stat = torch.zeros(8, dtype=torch.float64, device=dev)        # [0:3] moments, [3] residual^2, [4] status
    mom, res, status = stat[0:3], stat[3:4], stat[4:5]
    # every temporary of the loop: two X-sized pairs, G and P.  X_0 starts as zeros: for an input without a factor
    # (all zero, non-finite) the store below writes nothing, and the step queued ahead of the first read works on zeros
    xr, xi = (torch.zeros(n, k, dtype=dt, device=dev) for _ in range(2))
    yr, yi = (torch.empty(n, k, dtype=dt, device=dev) for _ in range(2))
    gr, gi, pr, pi = (torch.empty(k, k, dtype=dt, device=dev) for _ in range(4))
    call("cplxamd_init_moments", ptr(zr), ptr(zi), rows * cols, code, ptr(mom), ptr(ws), stream_ptr())
    # X_0 = Z / ||Z||_F, or its hermitian transpose: every singular value is at most 1
    call("cplxamd_init_scale_store", ptr(zr), ptr(zi), ptr(xr), ptr(xi), rows, cols, int(wide), _lib.INIT_SCALE_NORM, 1.0,
         ptr(mom), ptr(status), code, code, stream_ptr())
    cap, left, step = _step_cap(dt), None, 0
    while left is None or left > 0:
        step += 1
        # A[i, m] = B[i, m] = X[m, i] with conj(B): sum_m X[m, i] conj(X[m, j]) = conj(G)[i, j] = G^T
        _cgemm_into(xr, xi, (1, k), xr, xi, (1, k), k, k, n, True, gr, gi)
        # P^T = 1.5 I - 0.5 G^T (the coefficients are real) and ||G - I||_F, which a transpose does not change
        call("cplxamd_init_ns_poly", ptr(gr), ptr(gi), ptr(pr), ptr(pi), k, 1.5, -0.5, code, ptr(res), ptr(ws), stream_ptr())
        # X P: sum_i X[m, i] P[i, j] with B[j, i] = P^T[j, i], no conjugation.  Queued before the read-back, so the device
        # does not idle while the host looks at the residual.
        _cgemm_into(xr, xi, (k, 1), pr, pi, (k, 1), n, k, k, False, yr, yi)
        if left is None:
            s = stat.tolist()                    # the one device -> host read of this step (current stream)
            if step == 1:
                _check_start(s[2], s[4])
            if _check_residual(s[3], step, cap):
                left = _EXTRA[dt] + 1
        xr, xi, yr, yi = yr, yi, xr, xi
        left = None if left is None else left - 1
    return xr, xi, wide, step, stat, ws


def _compute_dtype(dtype):
    if dtype in (torch.float32, torch.bfloat16):
        return torch.float32
    if dtype == torch.float64:
        return torch.float64
    raise CplxAmdError(f"unsupported dtype {dtype}: float32, bfloat16 and float64 tensors are initialised")


def _std_complex(m):
    """numpy's std of a complex array: sqrt(mean |m - mean m|^2) (nn/init.py:117)."""
    c = m - m.mean()
    return math.sqrt(float((c.real * c.real + c.imag * c.imag).mean(dtype=torch.float64)))


def _semi_unitary(zr, zi, out_dtype, target=None):
    """Polar factor of the dense compute-dtype planes (zr, zi) as dense [rows, cols] planes of `out_dtype`; with `target`
    rescaled so that its complex standard deviation is `target`."""
    rows, cols = zr.shape
    if zr.is_cuda:
        xr, xi, wide, _, stat, ws = _polar_device(zr, zi)
        if target is None and not wide and out_dtype == zr.dtype:
            return xr, xi
        code = _plane_code(zr)
        out_code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float64: _lib.F64}[out_dtype]
        o_r, o_i = (torch.empty(rows, cols, dtype=out_dtype, device=zr.device) for _ in range(2))
        mode, f = (_lib.INIT_SCALE_CONST, 1.0) if target is None else (_lib.INIT_SCALE_STD, float(target))
        if target is not None:
            call("cplxamd_init_moments", ptr(xr), ptr(xi), rows * cols, code, ptr(stat[0:3]), ptr(ws), stream_ptr())
        call("cplxamd_init_scale_store", ptr(xr), ptr(xi), ptr(o_r), ptr(o_i), xr.shape[0], xr.shape[1], int(wide), mode, f,
             ptr(stat[0:3]), ptr(stat[4:5]), code, out_code, stream_ptr())
        if target is not None and stat[4].item() != 0.0:
            raise CplxAmdError("cplx_trabelsi_independent_: the factor has no spread to rescale (a constant matrix)")
        return o_r, o_i
    x, wide, _ = _polar_host(zr, zi)
    m = (x.mH if wide else x).resolve_conj()
    if target is not None:
        std = _std_complex(m)
        if not (math.isfinite(std) and std > 0.0):
            raise CplxAmdError("cplx_trabelsi_independent_: the factor has no spread to rescale (a constant matrix)")
        m = m * (target / std)
    return m.real.to(out_dtype).contiguous(), m.imag.to(out_dtype).contiguous()


def cplx_polar_factor(z):
    """The unitary polar factor U V^H of a 2-d Cplx z = U S V^H, as a new Cplx of the same shape and dtype: orthonormal
    columns when rows >= columns, orthonormal rows otherwise.  No SVD: Newton-Schulz on X_0 = X / ||X||_F (X = z, or z^H for
    a wide z), X <- X (1.5 I - 0.5 X^H X), until ||X^H X - I||_F <= 1e-3 and then 2 (float32) or 3 (float64) steps more.
    bfloat16 is computed in float32 and rounded once.  Raises CplxAmdError for a non-finite or all-zero input and for one
    that has not converged within the step cap (a rank-deficient input; see `_step_cap`) -- it never returns NaN."""
    if not isinstance(z, Cplx):
        raise CplxAmdError("cplx_polar_factor: not a Cplx")
    get_fans(z)                     # (fewer than 2 dimensions: its ValueError)
    if z.dim() != 2:
        raise ValueError(f"cplx_polar_factor takes a 2-d tensor, got {z.dim()} dimensions")
    if z.shape[0] == 0 or z.shape[1] == 0:
        raise CplxAmdError("cplx_polar_factor: empty input")
    ct = _compute_dtype(z.dtype)
    with torch.no_grad():
        zr, zi = z.real.detach().to(ct).contiguous(), z.imag.detach().to(ct).contiguous()
        o_r, o_i = _semi_unitary(zr, zi, z.dtype)
    return Cplx(o_r, o_i)


def cplx_trabelsi_independent_(cplx, kind="glorot"):
    """Orthogonal complex initialization proposed in Trabelsi et al. (2018): a semi-unitary matrix of the shape
    (prod(shape[:2]), prod(shape[2:])) (the weight itself when 2-d), rescaled to the standard deviation
    1 / sqrt(fan_in + fan_out) (glorot / xavier) or 1 / sqrt(fan_in) (kaiming / he), written in place.

    Two deliberate differences from the reference (nn/init.py:90-123):
      * Z has i.i.d. standard normal real and imaginary parts and M is its unitary POLAR factor (`cplx_polar_factor`),
        which makes M Haar-distributed over the semi-unitary matrices.  The reference draws uniform [0, 1) entries and
        keeps U_k V[:k, :] of a full SVD.
      * Z is drawn with torch.randn on the tensor's device (float64 for float64 tensors, float32 otherwise), so
        torch.manual_seed reproduces the result; the reference draws from numpy's global generator.  The random stream
        therefore cannot match the reference's.

    A draw whose smallest singular value is below the unit roundoff relative to ||Z||_F does not reach the residual
    threshold within `_step_cap` steps (for a square float32 Z about 1.5 draws in 1000 at 4096 x 4096, 1 in 100 at 8192,
    9 in 100 at 16384).  Such a draw is discarded and Z is drawn again, up to `_MAX_DRAWS` times in all.  For a Gaussian Z
    the factors U, V are independent of the singular values, so rejecting on the singular values leaves M Haar-
    distributed; the result is still a function of the seed alone.  Only a generator that keeps producing
    rank-deficient matrices can make this raise."""
    scale = _trabelsi_scale(cplx, kind)
    shape = tuple(cplx.shape)
    rows, cols = (shape if len(shape) == 2 else (shape[0] * shape[1], math.prod(shape[2:])))
    ct = _compute_dtype(cplx.dtype)
    with torch.no_grad():
        for draw in range(1, _MAX_DRAWS + 1):
            z = torch.randn(2, rows, cols, dtype=ct, device=cplx.device)
            try:
                m_r, m_i = _semi_unitary(z[0], z[1], cplx.dtype, target=scale)
                break
            except _NotConverged:
                if draw == _MAX_DRAWS:
                    raise
        cplx.real.copy_(m_r.reshape(shape))
        cplx.imag.copy_(m_i.reshape(shape))
    return cplx
