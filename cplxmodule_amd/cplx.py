"""Planar complex tensors and the functional complex algebra of the hot path.

`Cplx` keeps the reference's contract (cplxmodule/cplx.py:10-376): a light container over two
real tensors of identical shape which are never copied on construction.  The GEMM-shaped
functions (`linear`, `conv2d`, `@`) and `abs` run on the HIP kernels of libcplxamd.so; cheap
pointwise arithmetic and views stay as torch plumbing on the two planes.
"""
import math
import os
from copy import deepcopy

import torch

from . import ops
from ._lib import CplxAmdError, ntuple


class Cplx:
    """Complex tensor in split (real, imag) layout."""

    __slots__ = ("_re", "_im")

    def __new__(cls, real, imag=None):
        if isinstance(real, cls):
            return real
        if isinstance(real, complex):
            real, imag = torch.tensor(real.real), torch.tensor(real.imag)
        elif isinstance(real, float):
            if imag is None:
                imag = 0.0
            elif not isinstance(imag, float):
                raise TypeError("Imaginary part must be float.")
            real, imag = torch.tensor(real), torch.tensor(imag)
        elif not isinstance(real, torch.Tensor):
            raise TypeError("Real part must be torch.Tensor.")
        if imag is None:
            imag = torch.zeros_like(real)
        elif not isinstance(imag, torch.Tensor):
            raise TypeError("Imaginary part must be torch.Tensor.")
        if real.shape != imag.shape:
            raise ValueError("Real and imaginary parts have mistmatching shape.")
        obj = super().__new__(cls)
        obj._re, obj._im = real, imag
        return obj

    # -- parts and basic protocol ---------------------------------------------------------
    real = property(lambda self: self._re)
    imag = property(lambda self: self._im)
    shape = property(lambda self: self._re.shape)
    dtype = property(lambda self: self._re.dtype)
    device = property(lambda self: self._re.device)

    def _map(self, fn, *a, **k):
        return type(self)(fn(self._re, *a, **k), fn(self._im, *a, **k))

    def apply(self, f, *a, **k):
        """Apply `f` to the real and the imaginary planes independently."""
        return self._map(f, *a, **k)

    def __copy__(self):
        return type(self)(self._re, self._im)

    def __deepcopy__(self, memo):
        return type(self)(deepcopy(self._re, memo), deepcopy(self._im, memo))

    def __getitem__(self, key):
        return type(self)(self._re[key], self._im[key])

    def __setitem__(self, key, value):
        if isinstance(value, (Cplx, complex)):
            self._re[key], self._im[key] = value.real, value.imag
        else:
            self._re[key], self._im[key] = value, value

    def __iter__(self):
        return map(type(self), self._re, self._im)

    def __reversed__(self):
        return type(self)(reversed(self._re), reversed(self._im))

    def __len__(self):
        return self.shape[0]

    def __repr__(self):
        return f"{type(self).__name__}(\n  real={self._re},\n  imag={self._im}\n)"

    def clone(self):
        return self._map(torch.clone)

    def detach(self):
        return self._map(torch.Tensor.detach)

    def requires_grad_(self, requires_grad=True):
        return type(self)(self._re.requires_grad_(requires_grad),
                          self._im.requires_grad_(requires_grad))

    @property
    def grad(self):
        re, im = self._re.grad, self._im.grad
        return None if re is None or im is None else type(self)(re, im)

    def is_complex(self):
        return True

    def dim(self):
        return self._re.dim()

    def size(self, *dim):
        return self._re.size(*dim)

    def item(self):
        return float(self._re) + 1j * float(self._im)

    # -- placement ------------------------------------------------------------------------
    def to(self, *a, **k):
        return self._map(torch.Tensor.to, *a, **k)

    def cuda(self, device=None, non_blocking=False):
        return self._map(torch.Tensor.cuda, device=device, non_blocking=non_blocking)

    def cpu(self):
        return self._map(torch.Tensor.cpu)

    @classmethod
    def from_numpy(cls, array):
        return cls(torch.from_numpy(array.real.copy()), torch.from_numpy(array.imag.copy()))

    def numpy(self):
        return self._re.numpy() + 1j * self._im.numpy()

    # -- constructors ---------------------------------------------------------------------
    @classmethod
    def _filled(cls, maker, sizes, dtype, device, requires_grad, imag_maker=None):
        re = maker(*sizes, dtype=dtype, device=device, requires_grad=requires_grad)
        im = (imag_maker or maker)(*sizes, dtype=dtype, device=device, requires_grad=requires_grad)
        return cls(re, im)

    @classmethod
    def empty(cls, *sizes, dtype=None, device=None, requires_grad=False):
        return cls._filled(torch.empty, sizes, dtype, device, requires_grad)

    @classmethod
    def zeros(cls, *sizes, dtype=None, device=None, requires_grad=False):
        return cls._filled(torch.zeros, sizes, dtype, device, requires_grad)

    @classmethod
    def ones(cls, *sizes, dtype=None, device=None, requires_grad=False):
        return cls._filled(torch.ones, sizes, dtype, device, requires_grad, torch.zeros)

    # -- shape manipulation ---------------------------------------------------------------
    def t(self):
        return self._map(torch.Tensor.t)

    def h(self):
        return self.conj.t()

    def flatten(self, start_dim=0, end_dim=-1):
        return self._map(torch.flatten, start_dim, end_dim)

    def view(self, *shape):
        shape = shape[0] if shape and isinstance(shape[0], tuple) else shape
        return self._map(torch.Tensor.view, *shape)

    def view_as(self, other):
        return self.view(*other.shape)

    def reshape(self, *shape):
        shape = shape[0] if shape and isinstance(shape[0], tuple) else shape
        return self._map(torch.Tensor.reshape, *shape)

    def squeeze(self, dim=None):
        return self._map(torch.squeeze) if dim is None else self._map(torch.squeeze, dim)

    def unsqueeze(self, dim):
        return self._map(torch.unsqueeze, dim)

    def permute(self, *dims):
        return self._map(torch.Tensor.permute, *dims)

    def transpose(self, dim0, dim1):
        return self._map(torch.transpose, dim0, dim1)

    # -- arithmetic -----------------------------------------------------------------------
    @property
    def conj(self):
        return type(self)(self._re, -self._im)

    def conjugate(self):
        return self.conj

    def __pos__(self):
        return self

    def __neg__(self):
        return type(self)(-self._re, -self._im)

    def __add__(self, other):
        if isinstance(other, (Cplx, complex)):
            return type(self)(self._re + other.real, self._im + other.imag)
        return type(self)(self._re + other, self._im)

    __radd__ = __iadd__ = __add__

    def __sub__(self, other):
        if isinstance(other, (Cplx, complex)):
            return type(self)(self._re - other.real, self._im - other.imag)
        return type(self)(self._re - other, self._im)

    __isub__ = __sub__

    def __rsub__(self, other):
        return -self + other

    def __mul__(self, other):
        if isinstance(other, Cplx) and ops.cplx_mul_ok(self._re, self._im, other._re, other._im):
            return type(self)(*ops.cplx_mul(self._re, self._im, other._re, other._im))      # one launch (float32: same bits as the reference's 6 kernels; bf16: float32 intermediates)
        if isinstance(other, (Cplx, complex)):
            return type(self)(self._re * other.real - self._im * other.imag,
                              self._im * other.real + self._re * other.imag)
        return type(self)(self._re * other, self._im * other)

    __rmul__ = __imul__ = __mul__

    def __truediv__(self, other):
        if isinstance(other, Cplx) and ops.cplx_mul_ok(self._re, self._im, other._re, other._im):
            return type(self)(*ops.cplx_mul(self._re, self._im, other._re, other._im, div=True))
        if isinstance(other, (Cplx, complex)):
            other = Cplx(other) if isinstance(other, complex) else other
            den = other.real * other.real + other.imag * other.imag
            return self * (other.conj / den)
        return type(self)(self._re / other, self._im / other)

    __itruediv__ = __truediv__

    def __rtruediv__(self, other):
        den = self._re * self._re + self._im * self._im
        return (self.conj / den) * other

    def __matmul__(self, other):
        """Complex matrix product on the complex GEMM kernel (reference: 4 torch.matmul,
        cplxmodule/cplx.py:167-174)."""
        if not isinstance(other, Cplx):
            other = Cplx(other)
        return matmul(self, other)

    __imatmul__ = __matmul__

    def __rmatmul__(self, other):
        return matmul(Cplx(other), self)

    def __abs__(self):
        """Modulus via one fused kernel (reference: stack + norm, cplxmodule/cplx.py:183-192)."""
        if self._re.dtype in (torch.float32, torch.bfloat16) and self._im.dtype == self._re.dtype:
            return ops.AbsFn.apply(self._re, self._im)
        # other dtypes (float64 host-side utilities): the reference's own formulation
        return torch.norm(torch.stack([self._re, self._im], dim=0), p=2, dim=0)

    @property
    def angle(self):
        return torch.atan2(self._im, self._re)


# ------------------------------------------------------------------------------------------ #
#  functional API                                                                            #
# ------------------------------------------------------------------------------------------ #
def randn(*size, dtype=None, device=None, requires_grad=False):
    """Standard complex Gaussian noise: ONE normal draw of shape [2, *size] / sqrt(2), plane 0 ->
    real, plane 1 -> imag (same layout as cplxmodule/cplx.py:544-550, so that a recorded noise
    tape can be shared with the reference)."""
    z = torch.randn(2, *size, dtype=dtype, device=device) / math.sqrt(2)
    out = Cplx(z[0], z[1])
    return out.requires_grad_(True) if requires_grad else out


def randn_like(input, dtype=None, device=None, requires_grad=False):
    return randn(*input.size(), dtype=input.dtype if dtype is None else dtype,
                 device=input.device if device is None else device, requires_grad=requires_grad)


def phaseshift(input, phi=0.0):
    """z exp(i phi), phi in radians (cplxmodule/cplx.py:619-631)."""
    phi = torch.as_tensor(phi, dtype=input.real.dtype, device=input.real.device)
    return input * Cplx(torch.cos(phi), torch.sin(phi))


def linear(input, weight, bias=None):
    """y = x W^T + b on the complex GEMM kernel (replaces linear_naive, cplxmodule/cplx.py:634-648)."""
    br, bi = (None, None) if bias is None else (bias.real, bias.imag)
    yr, yi = ops.CplxLinearFn.apply(input.real, input.imag, weight.real, weight.imag, br, bi)
    return Cplx(yr, yi)


# CPLXAMD_TRUE_3M=1: `linear_3m` really runs Gauss's three products (A/B, accuracy studies); default 0 -- see linear_3m
_TRUE_3M = os.environ.get("CPLXAMD_TRUE_3M", "0") == "1"


def linear_3m(input, weight, bias=None, true_3m=None):
    """Gauss's three-product form (cplxmodule/cplx.py:669-694).  On the reference's CPU path it is the FAST spelling of
    `linear` (0.64x the time); here it must not be a pessimisation: for bf16 activations the one-loop 4M MFMA kernel is
    both faster (2.32 vs 2.60 ms fwd+bwd at configs[1]: the K loop is issue / LDS bound, not MFMA bound, so dropping a
    quarter of the MFMAs buys nothing -- profiles/r04_gemm_w4_ab.txt section 8) and more accurate (no bf16-rounded operand
    sums), so by default `linear_3m` IS `linear`.  `true_3m=True` (or env CPLXAMD_TRUE_3M=1) runs the three real MFMA
    GEMMs + fused combine (operand sums rounded to bf16; float32 activations always take the exact 4M kernel)."""
    if not (_TRUE_3M if true_3m is None else true_3m):
        return linear(input, weight, bias)
    br, bi = (None, None) if bias is None else (bias.real, bias.imag)
    yr, yi = ops.CplxLinearFn.apply(input.real, input.imag, weight.real, weight.imag, br, bi, 1)
    return Cplx(yr, yi)


# the remaining algorithm names of the reference (cplx.py:634-698) share the 4M kernel
linear_naive = linear_cat = linear


def bilinear(input1, input2, weight, bias=None, conjugate=True):
    """y = x1^H W x2 + b (conjugate=True) or x1^T W x2 + b (cplxmodule/cplx.py:1062-1087):
    one complex GEMM over the second input with the [O, I1, I2] weight read as [(O I1), I2],
    then the bilinear reduction kernel over the first input."""
    br, bi = (None, None) if bias is None else (bias.real, bias.imag)
    yr, yi = ops.CplxBilinearFn.apply(input1.real, input1.imag, input2.real, input2.imag, weight.real,
                                      weight.imag, br, bi, bool(conjugate), None, None, None, 0, 0)
    return Cplx(yr, yi)


bilinear_naive = bilinear_cat = bilinear


def einsum(equation, *tensors):
    """Einstein summation of one or two complex tensors, no conjugation (cplxmodule/cplx.py:1032-1059).

    One operand: `torch.einsum` on each plane (a permutation / diagonal / sum is plumbing; any device).  Two operands:
    everything `torch.einsum` accepts for two operands, as ONE launch of the strided contraction kernel (csrc/einsum.hip;
    plain `[M, K] x [N, K]` products go to `linear`'s GEMM family: cplxmodule_amd/einsum.py), float32 on the exact
    float32 matrix instruction whatever `fp32_mode` says, bfloat16 with float32 accumulation, float64 on the checking
    route of `@`.  Differentiable to any order.  There is no host path: two CPU operands raise."""
    if not tensors:
        raise RuntimeError("`einsum()` requires at least one tensor.")
    if len(tensors) > 2:
        raise RuntimeError(f"`Cplx.einsum` does not support more than 2 tensors. Got {len(tensors)}.")
    if len(tensors) == 1:
        z = tensors[0]
        return Cplx(torch.einsum(equation, z.real), torch.einsum(equation, z.imag))
    from . import einsum as _einsum
    a, b = tensors
    for pos, t in enumerate((a, b)):
        if not isinstance(t, Cplx):
            raise CplxAmdError(f"einsum: operand {pos} is a {type(t).__name__}, not a Cplx (real x complex products are "
                               "not offered: wrap the tensor in Cplx)")
    planes = (a.real, a.imag, b.real, b.imag)
    if any(t.dtype != a.dtype for t in planes):
        raise CplxAmdError(f"einsum: mixed dtypes {a.real.dtype}/{a.imag.dtype} and {b.real.dtype}/{b.imag.dtype}: "
                           "both operands must share one dtype")
    if a.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise CplxAmdError(f"einsum: unsupported dtype {a.dtype}: the contraction kernel takes float32 and bfloat16 "
                           "(float64 runs the checking route)")
    if any(not t.is_cuda for t in planes):
        raise CplxAmdError("einsum: two-operand products run on MI355X only (there is no CPU path): got a tensor on "
                           f"'{next(t.device for t in planes if not t.is_cuda)}'")
    if any(t.device != a.device for t in planes):
        raise CplxAmdError(f"einsum: operands on different devices: {a.device} vs {b.device}")
    return Cplx(*_einsum.einsum2(equation, *planes))


def matmul(u, v):
    """u[..., M, K] @ v[..., K, N]; batch dims of `v` (if any) must equal those of `u`."""
    ur, ui, vr, vi = u.real, u.imag, v.real, v.imag
    if vr.dim() == 2:
        lead, K = ur.shape[:-1], ur.shape[-1]
        # (x W^T) with W = v^T: feed v through the strided B operand, no copy
        a_r, a_i = ur.reshape(-1, K).contiguous(), ui.reshape(-1, K).contiguous()
        N = vr.shape[1]
        yr, yi = _MatmulFn.apply(a_r, a_i, vr.contiguous(), vi.contiguous())
        return Cplx(yr.view(*lead, N), yi.view(*lead, N))
    if ur.shape[:-2] != vr.shape[:-2]:
        raise CplxAmdError("batched complex matmul needs identical batch dimensions")
    batch = ur.shape[:-2]
    M, K, N = ur.shape[-2], ur.shape[-1], vr.shape[-1]
    flat = [t.reshape(-1, *t.shape[-2:]).contiguous() for t in (ur, ui, vr, vi)]
    nb = flat[0].shape[0]
    if nb > 65535:                                     # grid.z limit of the batched launch
        parts = [_BatchedMatmulFn.apply(*(t[lo:lo + 65535] for t in flat)) for lo in range(0, nb, 65535)]
        yr, yi = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    else:
        yr, yi = _BatchedMatmulFn.apply(*flat)
    return Cplx(yr.view(*batch, M, N), yi.view(*batch, M, N))


class _BatchedMatmulFn(torch.autograd.Function):
    """[Z, M, K] @ [Z, K, N] in one batched launch of the generic complex GEMM (blockIdx.z = entry)."""

    @staticmethod
    def forward(ctx, ar, ai, vr, vi):
        Z, M, K = ar.shape
        N = vr.shape[2]
        if ar.dtype != vr.dtype:
            raise CplxAmdError("matmul operands must share a dtype")
        ctx.save_for_backward(ar, ai, vr, vi)
        return ops.cgemm_batched(ar, ai, (K, 1, M * K), vr, vi, (1, N, K * N), Z, M, N, K)

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, vr, vi = ctx.saved_tensors
        Z, M, K = ar.shape
        N = vr.shape[2]
        if torch.is_grad_enabled():       # create_graph=True: dA = G V^H, dV = A^H G through this Function itself
            T = lambda t: t.transpose(1, 2).contiguous()  # noqa: E731
            gr, gi = gr.contiguous(), gi.contiguous()
            dar, dai = _BatchedMatmulFn.apply(gr, gi, T(vr), -T(vi))
            dvr, dvi = _BatchedMatmulFn.apply(T(ar), -T(ai), gr, gi)
            return dar, dai, dvr, dvi
        gr, gi = gr.contiguous(), gi.contiguous()
        # dA[m,k] = sum_n G[m,n] conj(V[k,n]);  dV[k,n] = conj(sum_m A[m,k] conj(G[m,n]))
        dar, dai = ops.cgemm_batched(gr, gi, (N, 1, M * N), vr, vi, (N, 1, K * N), Z, M, K, N, conj_b=True)
        tr, ti = ops.cgemm_batched(ar, ai, (1, K, M * K), gr, gi, (1, N, M * N), Z, K, N, M, conj_b=True)
        return dar, dai, tr, -ti


class _MatmulFn(torch.autograd.Function):
    """[M,K] @ [K,N] (no conjugation) on the generic complex GEMM."""

    @staticmethod
    def forward(ctx, ar, ai, vr, vi):
        M, K = ar.shape
        N = vr.shape[1]
        ctx.save_for_backward(ar, ai, vr, vi)
        if ar.dtype != vr.dtype:
            raise CplxAmdError("matmul operands must share a dtype")
        return ops.cgemm(ar, ai, (K, 1), vr, vi, (1, N), M, N, K, out_dtype=ar.dtype)

    @staticmethod
    def backward(ctx, gr, gi):
        ar, ai, vr, vi = ctx.saved_tensors
        M, K = ar.shape
        N = vr.shape[1]
        if torch.is_grad_enabled():       # create_graph=True: dA = G V^H, dV = A^H G through this Function itself
            T = lambda t: t.t().contiguous()  # noqa: E731
            gr, gi = gr.contiguous(), gi.contiguous()
            dar, dai = _MatmulFn.apply(gr, gi, T(vr), -T(vi))
            dvr, dvi = _MatmulFn.apply(T(ar), -T(ai), gr, gi)
            return dar, dai, dvr, dvi
        gr, gi = gr.contiguous(), gi.contiguous()
        # dA = G conj(V)^T : dA[m,k] = sum_n G[m,n] conj(V[k,n])
        dar, dai = ops.cgemm(gr, gi, (N, 1), vr, vi, (N, 1), M, K, N, conj_b=True, out_dtype=ar.dtype)
        # dV = conj(A)^T G : dV[k,n] = sum_m conj(A[m,k]) G[m,n]; computed as conj(sum A conj(G))
        tr, ti = ops.cgemm(ar, ai, (1, K), gr, gi, (1, N), K, N, M, conj_b=True, out_dtype=ar.dtype)
        return dar, dai, tr, -ti


def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
           padding_mode="zeros"):
    """Complex 2-d cross-correlation y = x * W + b (no conjugation), cplxmodule/cplx.py:770-838."""
    from . import conv  # late import: conv pulls in its own kernels
    return conv.cplx_conv2d(input, weight, bias, stride, padding, dilation, groups, padding_mode)


def conv1d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, padding_mode="zeros"):
    """Complex 1-d cross-correlation on [B, C, L] (cplxmodule/cplx.py:803-819): the 2-d kernels on a
    height-1 image."""
    from . import conv
    return conv.cplx_conv1d(input, weight, bias, stride, padding, dilation, groups, padding_mode)


def conv3d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, padding_mode="zeros"):
    """Complex 3-d cross-correlation on [B, C, D, H, W] (cplxmodule/cplx.py:841-857): the sum over
    the depth taps of 2-d correlations on the conv2d kernels (conv3d.py)."""
    from .conv3d import cplx_conv3d
    return cplx_conv3d(input, weight, bias, stride, padding, dilation, groups, padding_mode)


def symmetric_circular_padding(input, padding):
    """cplxmodule/cplx.py:701-714: circular padding ((p + 1) // 2, p // 2) per spatial dimension of a [B, C, L_1 .. L_n]
    complex tensor (`padding`: int or one entry per spatial dimension, fed to F.pad in the reference's order)."""
    import torch.nn.functional as F
    assert input.dim() > 2
    if isinstance(padding, int):
        padding = (input.dim() - 2) * [padding]
    assert isinstance(padding, (tuple, list)) and len(padding) + 2 == input.dim()
    expanded = []
    for pad in padding:
        expanded.extend(((pad + 1) // 2, pad // 2))
    return Cplx(F.pad(input.real, tuple(expanded), mode="circular"), F.pad(input.imag, tuple(expanded), mode="circular"))


def convnd(conv, input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, padding_mode="zeros"):
    """The reference's module-level operator (cplxmodule/cplx.py:770-800).  `conv` -- there the real torch functional that
    does the work (F.conv1d / 2d / 3d) -- only names the dimensionality here: the kernels behind conv1d / conv2d / conv3d
    run whichever is handed in (None: decided by input.dim())."""
    nd = input.dim() - 2
    name = getattr(conv, "__name__", "") if conv is not None else ""
    if name in ("conv1d", "conv2d", "conv3d") and int(name[4]) != nd:
        raise ValueError(f"{name} on a {input.dim()}-d input")
    fn = {1: conv1d, 2: conv2d, 3: conv3d}.get(nd)
    if fn is None:
        raise ValueError(f"convnd: {nd} spatial dimensions are not supported (1, 2 or 3)")
    return fn(input, weight, bias, stride, padding, dilation, groups, padding_mode)


def convnd_naive(conv, input, weight, stride=1, padding=0, dilation=1, groups=1):
    """cplxmodule/cplx.py:717-726 (four real convolutions; the grouped form): the same complex kernels."""
    return convnd(conv, input, weight, None, stride, padding, dilation, groups)


def convnd_quick(conv, input, weight, stride=1, padding=0, dilation=1):
    """cplxmodule/cplx.py:729-742 (two real convolutions with stacked filters, groups = 1): the same complex kernels."""
    return convnd(conv, input, weight, None, stride, padding, dilation, 1)


def convnd_3m(conv, input, weight, stride=1, padding=0, dilation=1, groups=1):
    """cplxmodule/cplx.py:745-767 (Gauss's three real convolutions; not wired into the reference's layers): routed to the
    four-product kernels, like linear_3m -- one fused K loop beats three launches plus operand sums on this chip."""
    return convnd(conv, input, weight, None, stride, padding, dilation, groups)


def conv_transpose2d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1,
                     dilation=1, padding_mode="zeros"):
    """Complex 2-d transposed convolution, weight [in, out / groups, kh, kw], no conjugation
    (cplxmodule/cplx.py:860-1001; the reference's functional default `groups=0` is not kept).  Runs
    the data-gradient kernels of conv2d as the forward pass."""
    from . import conv
    return conv.cplx_conv_transpose2d(input, weight, bias, stride, padding, output_padding, groups,
                                      dilation, padding_mode)


def conv_transpose1d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1,
                     dilation=1, padding_mode="zeros"):
    from . import conv
    return conv.cplx_conv_transpose1d(input, weight, bias, stride, padding, output_padding, groups,
                                      dilation, padding_mode)


def conv_transpose3d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1,
                     dilation=1, padding_mode="zeros"):
    """Complex 3-d transposed convolution on [B, C, D, H, W], weight [in, out / groups, kd, kh, kw], no conjugation
    (cplxmodule/cplx.py:1004-1029; the reference's functional default `groups=0` is not kept).  Runs the data-gradient
    kernel of the native 3-d convolution (csrc/conv3d.hip) as the forward pass; float32 and bfloat16 only, no second
    derivative."""
    from .conv3d import cplx_conv_transpose3d
    return cplx_conv_transpose3d(input, weight, bias, stride, padding, output_padding, groups, dilation, padding_mode)


def conv_transposend(conv, input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1,
                     padding_mode="zeros"):
    """The reference's module-level transposed operator (cplxmodule/cplx.py:916-945).  As in `convnd`, `conv` -- there
    the real torch functional that does the work (F.conv_transpose1d / 2d / 3d) -- only names the dimensionality here
    (None: decided by input.dim()); the kernels behind conv_transpose1d / 2d / 3d run."""
    nd = input.dim() - 2
    name = getattr(conv, "__name__", "") if conv is not None else ""
    if name in ("conv_transpose1d", "conv_transpose2d", "conv_transpose3d") and int(name[14]) != nd:
        raise ValueError(f"{name} on a {input.dim()}-d input")
    fn = {1: conv_transpose1d, 2: conv_transpose2d, 3: conv_transpose3d}.get(nd)
    if fn is None:
        raise ValueError(f"conv_transposend: {nd} spatial dimensions are not supported (1, 2 or 3)")
    return fn(input, weight, bias, stride, padding, output_padding, groups, dilation, padding_mode)


def conv_transposend_naive(conv_t, input, weight, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
    """cplxmodule/cplx.py:860-873 (four real transposed convolutions): the same complex kernels."""
    return conv_transposend(conv_t, input, weight, None, stride, padding, output_padding, groups, dilation)


def conv_transposend_3m(conv_t, input, weight, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
    """cplxmodule/cplx.py:876-913 (Gauss's three real transposed convolutions): routed to the four-product kernels, like
    convnd_3m."""
    return conv_transposend(conv_t, input, weight, None, stride, padding, output_padding, groups, dilation)


def from_interleaved_real(input, copy=True, dim=-1):
    """[..., 2D] interleaved (re, im) -> Cplx [..., D]  (cplxmodule/cplx.py:451-455).  copy=True along
    the last dim on the GPU is one de-interleaving kernel pass (csrc/layout.hip) instead of two
    strided copies; copy=False returns strided views like the reference."""
    dim = dim % input.dim()
    if copy and dim == input.dim() - 1 and input.is_cuda and input.dtype in (torch.float32, torch.bfloat16):
        return Cplx(*ops.DeinterleaveFn.apply(input))
    shape = list(input.shape)
    shape[dim:dim + 1] = [shape[dim] // 2, 2]
    pair = input.reshape(shape)
    re, im = pair.select(dim + 1, 0), pair.select(dim + 1, 1)
    return Cplx(re.clone(), im.clone()) if copy else Cplx(re, im)


from_real = from_interleaved_real


def to_interleaved_real(input, flatten=True, dim=-1):
    """Cplx [..., D] -> real [..., 2D] interleaved (cplxmodule/cplx.py:466-470); last dim on the GPU:
    one interleaving kernel pass."""
    d = dim % input.dim()
    re, im = input.real, input.imag
    if d == input.dim() - 1 and re.is_cuda and re.dtype in (torch.float32, torch.bfloat16):
        out = ops.InterleaveFn.apply(re, im)
        return out if flatten else out.view(*re.shape, 2)
    out = torch.stack([re, im], dim=d + 1)
    return out.flatten(d, d + 1) if flatten else out


to_real = to_interleaved_real


def from_concatenated_real(input, copy=True, dim=-1):
    re, im = torch.chunk(input, 2, dim=dim)
    return Cplx(re.clone(), im.clone()) if copy else Cplx(re, im)


def to_concatenated_real(input, flatten=None, dim=-1):
    return torch.cat([input.real, input.imag], dim=dim)


# ---- joining / splitting (cplxmodule/cplx.py:379-448): plane-wise torch plumbing, any device --------------------------
def cat(tensors, dim):
    tensors = [*map(Cplx, tensors)]
    return Cplx(torch.cat([z.real for z in tensors], dim=dim), torch.cat([z.imag for z in tensors], dim=dim))


def split(input, split_size_or_sections, dim=0):
    """see documentation for `torch.split`"""
    return tuple(Cplx(re, im) for re, im in zip(torch.split(input.real, split_size_or_sections, dim),
                                                torch.split(input.imag, split_size_or_sections, dim)))


def chunk(input, chunks, dim=0):
    """see documentation for `torch.chunk`"""
    return tuple(Cplx(re, im) for re, im in zip(torch.chunk(input.real, chunks, dim), torch.chunk(input.imag, chunks, dim)))


def stack(tensors, dim):
    tensors = [*map(Cplx, tensors)]
    return Cplx(torch.stack([z.real for z in tensors], dim=dim), torch.stack([z.imag for z in tensors], dim=dim))


def unbind(input, dim=0):
    """see documentation for `torch.unbind`"""
    return tuple(Cplx(re, im) for re, im in zip(torch.unbind(input.real, dim), torch.unbind(input.imag, dim)))


def take(input, index):
    """see documentation for `torch.take`"""
    return Cplx(torch.take(input.real, index), torch.take(input.imag, index))


def narrow(input, dim, start, length):
    """see documentation for `torch.narrow`"""
    return Cplx(torch.narrow(input.real, dim, start, length), torch.narrow(input.imag, dim, start, length))


def squeeze(input, dim=None):
    """see documentation for `torch.squeeze`"""
    return input.squeeze(dim)


def unsqueeze(input, dim):
    """see documentation for `torch.unsqueeze`"""
    return Cplx(torch.unsqueeze(input.real, dim), torch.unsqueeze(input.imag, dim))


# ---- elementary functions (cplxmodule/cplx.py:482-541): one fused kernel each way (csrc/cplxfn.hip) ----------------------
def _elementary(input, fn):
    return Cplx(*ops.CplxFnFn.apply(input.real, input.imag, fn))


def exp(input):
    r"""e^z = e^x (cos y + i sin y)."""
    return _elementary(input, "exp")


def log(input):
    r"""Principal logarithm (log|z|, atan2(y, x)); |z| is formed with scaling, so it never overflows or underflows."""
    return _elementary(input, "log")


def sin(input):
    r"""sin z = sin x cosh y + i cos x sinh y."""
    return _elementary(input, "sin")


def cos(input):
    r"""cos z = cos x cosh y - i sin x sinh y."""
    return _elementary(input, "cos")


def tan(input):
    r"""tan z = -i tanh(iz).  Finite wherever the true value is: the reference's sin(z) / cos(z) gives NaN once cosh(y)
    overflows (tan(x + 100j) there is nan, here ~1j)."""
    return _elementary(input, "tan")


def sinh(input):
    r"""sinh z = sinh x cos y + i cosh x sin y."""
    return _elementary(input, "sinh")


def cosh(input):
    r"""cosh z = cosh x cos y + i sinh x sin y."""
    return _elementary(input, "cosh")


def tanh(input):
    r"""tanh z in Kahan's form, saturated to (sign x, 4 sin y cos y e^{-2|x|}) for |x| > 11.  Finite wherever the true
    value is: the reference's sinh(z) / cosh(z) gives NaN once cosh(x) overflows (tanh(100 + 1j) there is nan, here ~1)."""
    return _elementary(input, "tanh")


# ---- Fourier transforms (not in the reference; signatures, shapes, n / s and norm as torch.fft): one launch of the
# package's own FFT kernels per transformed dim (cplxmodule_amd/fft.py, csrc/fft.hip) --------------------------------------
def _fourier(input, s, dim, norm, inverse, name):
    from . import fft as _fft
    return Cplx(*_fft.fftn(input, s, dim, norm, inverse, name))


def fft(input, n=None, dim=-1, norm=None):
    r"""Discrete Fourier transform X_k = sum_j x_j e^{-2 pi i jk/n} along `dim` of a `Cplx`, as `torch.fft.fft`: `n` pads
    with zeros or truncates, `norm` is None / "backward" (no scaling), "ortho" (1 / sqrt n) or "forward" (1 / n).  Planes
    of float32, bfloat16 (float32 arithmetic, one rounding) or float64 on the device; the result has the input's dtype
    and memory order.  Any length up to 2^22; differentiable to any order."""
    return _fourier(input, None if n is None else [n], [dim], norm, False, "fft")


def ifft(input, n=None, dim=-1, norm=None):
    r"""Inverse transform x_j = 1/n sum_k X_k e^{+2 pi i jk/n} along `dim`, as `torch.fft.ifft` (`norm` names the
    direction that carries the 1 / n, as there)."""
    return _fourier(input, None if n is None else [n], [dim], norm, True, "ifft")


def fft2(input, s=None, dim=(-2, -1), norm=None):
    """Two-dimensional transform, as `torch.fft.fft2`: one launch per dim, the last listed dim first; bf16 planes keep
    a float32 intermediate and round once."""
    return _fourier(input, s, dim, norm, False, "fft2")


def ifft2(input, s=None, dim=(-2, -1), norm=None):
    """Inverse of `fft2`, as `torch.fft.ifft2`."""
    return _fourier(input, s, dim, norm, True, "ifft2")


def fftn(input, s=None, dim=None, norm=None):
    """N-dimensional transform, as `torch.fft.fftn`: over all dims, the last len(s), or those in `dim`."""
    return _fourier(input, s, dim, norm, False, "fftn")


def ifftn(input, s=None, dim=None, norm=None):
    """Inverse of `fftn`, as `torch.fft.ifftn`."""
    return _fourier(input, s, dim, norm, True, "ifftn")


# ---- real-input / real-output transforms (as torch.fft's): an even length runs ONE complex transform of half the
# length plus an untangling pass, on the same engine (cplxmodule_amd/rfft.py, csrc/rfft.hip) ------------------------------
def _one(n):
    return None if n is None else [n]


def rfft(input, n=None, dim=-1, norm=None):
    r"""X_k = sum_j x_j e^{-2 pi i jk/n}, k = 0 .. n // 2, of a REAL tensor along `dim`, as `torch.fft.rfft` -> `Cplx` whose
    planes have the input's dtype (float32, bfloat16 or float64) and memory order.  No zero plane is built and only the
    half spectrum is computed and written.  Differentiable to any order (the gradient is not `irfft`: see rfft.py)."""
    from . import rfft as _rfft
    return Cplx(*_rfft.rfftn(input, _one(n), [dim], norm, False, "rfft"))


def irfft(input, n=None, dim=-1, norm=None):
    r"""Inverse of `rfft`, as `torch.fft.irfft`: a `Cplx` half spectrum -> a real tensor of length `n` (default 2 (m - 1))
    along `dim`; the first n // 2 + 1 entries are used (zero-padded if fewer), the imaginary parts of the DC and, for
    even n, the Nyquist entry are ignored."""
    from . import rfft as _rfft
    return _rfft.irfftn(input, _one(n), [dim], norm, True, "irfft")


def rfft2(input, s=None, dim=(-2, -1), norm=None):
    """`torch.fft.rfft2`: the real transform along the last listed dim, then the complex one along the other."""
    from . import rfft as _rfft
    return Cplx(*_rfft.rfftn(input, s, dim, norm, False, "rfft2"))


def irfft2(input, s=None, dim=(-2, -1), norm=None):
    """`torch.fft.irfft2`: the complex inverse along the first listed dim, then the real-output one along the last."""
    from . import rfft as _rfft
    return _rfft.irfftn(input, s, dim, norm, True, "irfft2")


def rfftn(input, s=None, dim=None, norm=None):
    """`torch.fft.rfftn`: over all dims, the last len(s), or those in `dim`; the half spectrum lies along the last one."""
    from . import rfft as _rfft
    return Cplx(*_rfft.rfftn(input, s, dim, norm, False, "rfftn"))


def irfftn(input, s=None, dim=None, norm=None):
    """`torch.fft.irfftn`: the inverse of `rfftn`; the last entry of `s` is the real output's length (default 2 (m - 1))."""
    from . import rfft as _rfft
    return _rfft.irfftn(input, s, dim, norm, True, "irfftn")


def hfft(input, n=None, dim=-1, norm=None):
    r"""`torch.fft.hfft`: the transform of a Hermitian signal given by its half (`Cplx`) -> its real spectrum of length
    `n` (default 2 (m - 1)): `irfft`'s kernel with the opposite sign and the forward transform's scaling."""
    from . import rfft as _rfft
    return _rfft.irfftn(input, _one(n), [dim], norm, False, "hfft")


def ihfft(input, n=None, dim=-1, norm=None):
    r"""`torch.fft.ihfft`: a real tensor -> the half (`Cplx`) of its Hermitian inverse transform: `rfft`'s kernel with the
    opposite sign and the inverse transform's scaling."""
    from . import rfft as _rfft
    return Cplx(*_rfft.rfftn(input, _one(n), [dim], norm, True, "ihfft"))


def stft(input, n_fft, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", normalized=False,
         onesided=None):
    r"""Short-time Fourier transform with `torch.stft`'s arguments and shape rules -> `Cplx` [..., N, frames] in torch's
    memory order, always (there is no `return_complex`).  Framing, reflect / constant padding and the window happen in the
    kernel's loader: no frame and no padded copy is made.  Any number of leading dims; `window=None` is rectangular.
    Deterministic, capturable, differentiable to any order (cplxmodule_amd/stft.py)."""
    from . import stft as _stft
    return _stft.stft(input, n_fft, hop_length, win_length, window, center, pad_mode, normalized, onesided)


def istft(input, n_fft, hop_length=None, win_length=None, window=None, center=True, normalized=False, onesided=None,
          length=None, return_complex=False, *, check_nola=True):
    r"""Inverse of `stft` with `torch.istft`'s arguments: a `Cplx` spectrogram [..., N, frames] -> a real tensor [..., T]
    (`onesided=False, return_complex=True`: a `Cplx`).  The overlap-add is one gather pass in a fixed order (no atomics).  `check_nola=True` reads the minimum of the window
    envelope on the host and raises RuntimeError below 1e-11, as torch does; pass False inside a stream capture."""
    from . import stft as _stft
    return _stft.istft(input, n_fft, hop_length, win_length, window, center, normalized, onesided, length, return_complex,
                       check_nola=check_nola)


def fftconvolve(input, other, mode="full"):
    r"""Linear convolution along the last dim, full[n] = sum_m input[n - m] other[m] (a plain complex product, nothing
    is conjugated), with the modes of `scipy.signal.fftconvolve` / `torchaudio.functional.fftconvolve`: "full" returns
    all N + M - 1 entries, "same" full[(M - 1) // 2 : (M - 1) // 2 + N] (the length of `input`, whichever operand is
    longer), "valid" full[min(N, M) - 1 : max(N, M)].  Each operand is a `Cplx` or a real tensor (a null imaginary
    plane: no zero plane is built); two real operands give a real tensor, else a `Cplx`, dense, in the operands' dtype
    (float32, bfloat16 -- float32 arithmetic, rounded once -- or float64, on the device).  Leading dims broadcast by
    torch's rules and are read in place (step slices, `expand`, transposed leading dims: no copy).  The shorter operand
    is the filter: up to 4096 taps one fused overlap-save kernel reads the long operand once and writes the result once
    (csrc/fftconv.hip); longer filters are composed from cplx.fft launches.  Deterministic, capturable in a hipGraph,
    differentiable to any order (cplxmodule_amd/fftconv.py)."""
    from . import fftconv as _fftconv
    return _fftconv.fftconvolve(input, other, mode)


# ---- chirp-z transforms (arguments and results as scipy.signal's): m bins on any arc or spiral of the z-plane from n
# samples, on one fused kernel (cplxmodule_amd/czt.py, csrc/czt.hip) ---------------------------------------------------------
def czt(x, m=None, w=None, a=1 + 0j):
    r"""Chirp-z transform y_k = sum_j x_j a^{-j} w^{jk}, k = 0 .. m - 1, along the last dim, as `scipy.signal.czt`: the
    z-transform of every vector at the points a w^{-k}.  `m` defaults to the number of samples n, `w` to e^{-2 pi i / m};
    `w` and `a` are Python numbers (no tensors, no gradient).  `x` is a `Cplx` or a real tensor (a null imaginary plane:
    no zero plane is built) of float32, bfloat16 (float32 arithmetic, one rounding) or float64 on the device; leading dims
    are batch and are read in place.  The result is a `Cplx` [..., m] in the input's dtype and memory order.  Up to
    n + m - 1 <= 8192 one launch reads n and writes m entries per vector; up to 2^22 the transform goes through a
    workspace.  `czt(x)` of a `Cplx` with the default `w`, a == 1 and a power of two m >= n is a zero-padded FFT and calls
    `cplx.fft`'s kernel (any other m is no shorter a convolution there than here).  Deterministic, capturable in a hipGraph, differentiable to any order in `x`.

    Off the unit circle the algorithm's tables span a factor e^D, D = |ln|w|| max(n, m)^2 / 2 + |ln|a|| n, and the error
    follows eps e^D (scipy's does too, silently); a contour with D > ln 2^24 (float32, bfloat16) or ln 2^53 (float64)
    leaves no correct digit and raises CplxAmdError."""
    from . import czt as _czt
    return _czt.czt(x, m, w, a)


def zoom_fft(x, fn, m=None, fs=2, endpoint=False):
    r"""The DFT of the last dim on `m` (default n) equally spaced frequencies of the band `fn` = (f1, f2) (a scalar: (0,
    fn)) at sampling rate `fs`, as `scipy.signal.zoom_fft`: `czt` with w = e^{-2 pi i scale / m}, a = e^{2 pi i f1 / fs},
    scale = (f2 - f1) / fs (with `endpoint`: times m / (m - 1), so that f2 is the last bin).  The kernel receives the
    fractions -scale / m and f1 / fs themselves, not a complex number to take the argument of."""
    from . import czt as _czt
    return _czt.zoom_fft(x, fn, m, fs, endpoint)


def czt_points(m, w=None, a=1 + 0j):
    r"""The points a w^{-k}, k = 0 .. m - 1, at which `czt` evaluates the z-transform, as `scipy.signal.czt_points`: a
    complex128 tensor on the host."""
    from . import czt as _czt
    return _czt.czt_points(m, w, a)


def upfirdn(h, x, up=1, down=1):
    r"""Upsample by `up`, FIR filter, downsample by `down` along the last dim, with the argument order and the result of
    `scipy.signal.upfirdn` (`mode="constant"`): y[n] = sum_k h[k] xu[n down - k] where xu[i up] = x[i] and zero
    elsewhere, for n < ceil(((N - 1) up + K) / down).  `h` and `x` are each a `Cplx` or a real tensor (a null imaginary
    plane: no zero plane is built); two real operands give a real tensor, else a `Cplx`, dense, in the operands' dtype
    (float32, bfloat16 -- float32 arithmetic, rounded once -- or float64, on the device).  Leading dims of `x` and `h`
    broadcast by torch's rules (a filter per channel, or one for all) and are read in place (step slices, `expand`,
    transposed leading dims: no copy).  Up to 4096 taps one direct-form polyphase kernel (csrc/upfirdn.hip) reads the
    signal once and writes the result once: xu is never built and each output costs ceil(K / up) multiply-adds.  Longer
    filters are composed from torch zero-stuffing, cplx.fftconvolve and a strided slice, which is not the hot path.
    Deterministic, capturable in a hipGraph, differentiable to any order in both operands (cplxmodule_amd/upfirdn.py).
    There is no `axis`: move the dim."""
    from . import upfirdn as _upfirdn
    return _upfirdn.upfirdn(h, x, up, down)


def resample_poly(x, up, down, window=("kaiser", 5.0)):
    r"""Resample along the last dim by the rational factor up / down with a polyphase low-pass, as
    `scipy.signal.resample_poly` does with `padtype="constant"`: ceil(N up / down) entries.  `up` and `down` are reduced
    by their gcd; equal rates return a copy of the input.  `window` is `("kaiser", beta)`: a Kaiser-windowed sinc of
    20 max(up, down) + 1 taps with its cut-off at 1 / max(up, down) of Nyquist and gain `up`, designed in float64 on the
    host with torch and cached (a constant: it has no gradient); or a 1-d real tensor of taps, which is the filter (times
    `up`, as scipy scales the array it is given) and receives a gradient if it requires one.  The whole resampling is one
    launch of cplx.upfirdn's kernel with the filter's delay folded into its offset: nothing is padded, nothing is sliced.
    `x` is a `Cplx` or a real tensor; dtypes, broadcasting, layouts and derivatives as `upfirdn`."""
    from . import upfirdn as _upfirdn
    return _upfirdn.resample_poly(x, up, down, window)


def lfilter(b, a, x, zi=None):
    r"""Filter along the last dim with the rational transfer function b / a, with the argument order and the result of
    `scipy.signal.lfilter` (direct form II transposed): a[0] y[n] = sum_k b[k] x[n - k] - sum_{k >= 1} a[k] y[n - k].
    `b` [..., nb], `a` [..., na], `x` [..., N] and `zi` are each a `Cplx` or a real tensor (a null imaginary plane: no
    zero plane is built); all-real operands give a real tensor, else a `Cplx`, dense, in the operands' dtype (float32,
    bfloat16 -- float32 arithmetic and state, rounded once -- or float64, on the device).  Leading dims broadcast by
    torch's rules (a filter per channel, or one for all) and are read in place (step slices, `expand`, transposed leading
    dims: no copy).  `a[..., 0]` normalises both `b` and `a` by a differentiable division.  Returns `y`; with `zi`
    [..., D], D = max(na, nb) - 1, returns `(y, zf)`, the state that continues the filter on the next block.  D = 0 is a
    scale.  Up to order 8 one chunk-parallel kernel (csrc/iir.hip) reads the signal once and writes the result once; the
    recurrence is parallel in time inside a tile, and long rows with few rows are cut into segments.  nb - 1 > 8 is
    composed from one cplx.upfirdn launch and the all-pole kernel; na - 1 > 8 raises `CplxAmdError`: use `sosfilt`.
    Deterministic, capturable in a hipGraph, differentiable to any order in b, a, x and zi (cplxmodule_amd/iir.py).
    Unlike scipy: `a[..., 0] == 0` is not checked (that would read the device; it gives inf / nan), and there is no
    `axis`: move the dim."""
    from . import iir as _iir
    return _iir.lfilter(b, a, x, zi)


def sosfilt(sos, x, zi=None):
    r"""Filter along the last dim with a cascade of second-order sections, as `scipy.signal.sosfilt`: `sos`
    [..., n_sections, 6] holds b0 b1 b2 a0 a1 a2 per section, a `Cplx` or a real tensor; `x`, dtypes, broadcasting,
    layouts and the result as `lfilter`.  Returns `y`, or `(y, zf)` when `zi` [..., n_sections, 2] is given.  The whole
    cascade runs inside one launch of `lfilter`'s kernel, a section reading the one before it from on-chip memory (up to
    16 sections per launch, longer cascades are chained); its gradient with respect to `x` is one launch too, reversed in
    time, conjugated, sections in reverse order.  When `sos` or `zi` requires a gradient (or `x` does and `zi` is given)
    the cascade is composed from one differentiable `lfilter` section per biquad, which is not the hot path.
    Unlike scipy: every section is normalised by its own a0, and `sos[..., 3] != 1` or `== 0` is not checked (a zero gives
    inf / nan); `zi` keeps n_sections next to the state dim, [..., n_sections, 2], so that leading dims broadcast (scipy
    puts n_sections first); there is no `axis`."""
    from . import iir as _iir
    return _iir.sosfilt(sos, x, zi)


def lfilter_zi(b, a):
    r"""The initial state of `lfilter` that is the steady state of the unit step, as `scipy.signal.lfilter_zi`: `b`
    [..., nb], `a` [..., na] (each a `Cplx` or a real tensor, leading dims broadcast) -> [..., D], D = max(na, nb) - 1, a
    real tensor when both are real, else a `Cplx`.  `lfilter(b, a, x, zi=lfilter_zi(b, a) * x[..., :1])` starts without
    a transient.  Coefficient-sized torch arithmetic in closed form (no linear solve), on any device, differentiable:
    after normalising by `a[..., 0]`, zi[0] = sum_{k >= 1} (b_k - a_k b_0) / sum_k a_k and
    zi[k] = (1 + a_1 + .. + a_k) zi[0] - sum_{j = 1 .. k} (b_j - a_j b_0).
    Unlike scipy: a filter with a pole at 1 (sum_k a_k == 0) is not checked (that would read the device) and gives inf /
    nan where scipy raises."""
    from . import filtfilt as _ff
    return _ff.lfilter_zi(b, a)


def sosfilt_zi(sos):
    r"""The initial state of `sosfilt` that is the steady state of the unit step, as `scipy.signal.sosfilt_zi`: `sos`
    [..., n_sections, 6] (a `Cplx` or a real tensor) -> [..., n_sections, 2], the layout `sosfilt` takes for `zi`.  Section
    s holds `lfilter_zi` of its biquad times the DC gains sum b / sum a of the sections before it.  Torch arithmetic on
    any device, differentiable; the remarks of `lfilter_zi` apply."""
    from . import filtfilt as _ff
    return _ff.sosfilt_zi(sos)


def filtfilt(b, a, x, padtype="odd", padlen=None):
    r"""Zero-phase filtering along the last dim: the filter b / a forward, then backward, as `scipy.signal.filtfilt` with
    `method="pad"`.  `x` [..., N] is extended by `padlen` samples on each side (default 3 max(na, nb)): `padtype` "odd"
    (2 x[0] - x[e - m] on the left), "even" (x[e - m]), "constant" (x[0]) or None (no extension); the right side mirrors
    the left.  The forward pass runs over the extension from the state `lfilter_zi(b, a) * ext[0]`, the backward pass
    over the reversed result from `lfilter_zi(b, a) *` (its first sample); the result is reversed and the extension
    dropped.  Nothing is conjugated.  Operands, dtypes (float32; bfloat16 with float32 arithmetic and a float32
    intermediate, rounded once; float64), broadcasting of leading dims, in-place reading of sliced / `expand`ed /
    transposed operands, real or `Cplx` results and the error types are `lfilter`'s.  For 1 <= D <= 8 and no operand
    requiring grad the call is two launches of `lfilter`'s kernel (csrc/filtfilt.hip): the first forms the extension from
    `x` where it lies and writes one compute-type workspace of N + 2 padlen samples, the second reads it in reverse and
    writes the N interior samples; both scale the steady state inside the kernel.  No padded copy, no flip, no slice;
    deterministic, capturable in a hipGraph.  When an operand requires grad, or D = 0, or nb - 1 > 8, the result is
    composed from a torch extension, two `lfilter` calls with `zi` and flips (differentiable to any order in b, a and x;
    not the hot path).  na - 1 > 8 raises `CplxAmdError`: use `sosfiltfilt`.  `ValueError` for an unknown `padtype`, a
    negative `padlen` and N <= padlen (scipy's wording), raised before the device is looked at.
    Unlike scipy: there is no `axis` (move the dim), no `method="gust"` and no `irlen`; an empty signal gives an empty
    result; `a[..., 0] == 0` and sum_k a_k == 0 are not checked (inf / nan)."""
    from . import filtfilt as _ff
    return _ff.filtfilt(b, a, x, padtype, padlen)


def sosfiltfilt(sos, x, padtype="odd", padlen=None):
    r"""Zero-phase filtering along the last dim with a cascade of second-order sections, as `scipy.signal.sosfiltfilt`:
    `filtfilt` with `sosfilt_zi(sos)` for the entering states; `sos`, `x`, dtypes, broadcasting and layouts as `sosfilt`,
    `padtype` / `padlen` and the errors as `filtfilt`.  Up to 16 sections and no operand requiring grad: two launches,
    the cascade running inside each.  More sections, or an operand that requires grad: composed from a torch extension, two
    `sosfilt` calls with `zi` and flips (not the hot path).
    Unlike scipy: `padlen` defaults to 3 (2 n_sections + 1); scipy subtracts min(#(b2 == 0), #(a2 == 0)) from the bracket,
    which would read the device here -- pass `padlen` for scipy's number.  No `axis`; the remarks of `sosfilt` apply."""
    from . import filtfilt as _ff
    return _ff.sosfiltfilt(sos, x, padtype, padlen)


def fftshift(input, dim=None):
    """`torch.fft.fftshift` on each plane (plumbing: any device)."""
    return Cplx(torch.fft.fftshift(input.real, dim=dim), torch.fft.fftshift(input.imag, dim=dim))


def ifftshift(input, dim=None):
    """`torch.fft.ifftshift` on each plane (plumbing: any device)."""
    return Cplx(torch.fft.ifftshift(input.real, dim=dim), torch.fft.ifftshift(input.imag, dim=dim))


def modrelu(input, threshold=0.5):
    """Soft-threshold of the modulus, phase kept: z * relu(1 - threshold / max(|z|, 1e-5))
    (cplxmodule/cplx.py:565-616; note the reference's flipped sign convention).  `threshold` is a
    float or a (learnable) tensor broadcastable to the input."""
    return Cplx(*ops.ModReluFn.apply(input.real, input.imag, threshold))


def dropout(input, p=0.5, training=True):
    """Complex dropout: real and imaginary parts of an element are dropped together
    (cplxmodule/nn/modules/extra.py:7-25); the Bernoulli stream is the package's Philox stream."""
    if not training or p == 0.0:
        return input
    from .nn.relevance.noise import noise
    seed, offset = noise.next(input.real.device)
    return Cplx(*ops.CplxDropoutFn.apply(input.real, input.imag, p, seed, offset))


def max_pool2d(input, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False):
    """Complex max pooling on [B, C, H, W]: the element of largest modulus in each window keeps
    both its parts (cplxmodule/cplx.py:1114-1175, 1183-1190)."""
    k = ntuple(kernel_size, 2)
    s = k if stride is None else ntuple(stride, 2)
    return Cplx(*ops.CplxMaxPool2dFn.apply(input.real, input.imag, k, s, ntuple(padding, 2),
                                           ntuple(dilation, 2), bool(ceil_mode)))


def max_pool1d(input, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False):
    """[B, C, L] (cplxmodule/cplx.py:1178-1181): the 2-d kernel on a height-1 image."""
    first = lambda v: v if isinstance(v, int) else v[0]  # noqa: E731
    k = first(kernel_size)
    s = k if stride is None else first(stride)
    z = Cplx(input.real.unsqueeze(2), input.imag.unsqueeze(2))
    out = max_pool2d(z, (1, k), (1, s), (0, first(padding)), (1, first(dilation)), ceil_mode)
    return Cplx(out.real.squeeze(2), out.imag.squeeze(2))


def max_pool3d(input, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False):
    """[B, C, D, H, W] (cplxmodule/cplx.py:1193-1200): separable, 2-d pool then 1-d pool over depth."""
    from .conv3d import cplx_max_pool3d
    return cplx_max_pool3d(input, kernel_size, stride, padding, dilation, ceil_mode)


# float64: a parity mode on its own kernels (f64.py)
_BatchedMatmulFn = ops.Route(_BatchedMatmulFn, "matmul_batched")
_MatmulFn = ops.Route(_MatmulFn, "matmul2d")
