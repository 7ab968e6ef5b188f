"""3-d convolution and abs-max pooling composed from the 2-d kernels.

Reference: cplx.conv3d (cplxmodule/cplx.py:841-857), CplxConv3d (nn/modules/conv.py:199-247),
the 3-d VD / ARD / masked layers, cplx.max_pool3d (cplx.py:1193-1200).  Not on the hot path
(SURVEY 8 names conv2d), so there is no dedicated 3-d kernel: a [kd, kh, kw] correlation is the
sum over the kd depth taps of 2-d correlations of depth-strided slices, each of which runs the
conv2d kernels (forward, dgrad, wgrad through their autograd Functions) on a [B * D', C, H, W]
batch; abs-max pooling is separable (max modulus over (h, w), then over d) and runs the 2-d and
1-d pooling kernels.  The variance path of the VD layers is the same composition on
(|x|^2, exp(log_sigma2)) followed by the fused noise-injection kernel.

The TRANSPOSED 3-d convolution (cplx.conv_transpose3d, cplxmodule/cplx.py:860-1029; nn.CplxConvTranspose3d) does run
on a native 3-d kernel, csrc/conv3d.hip: its forward pass is a strided data gradient, which at stride 2 in
three dimensions multiplies seven structural zeros of eight unless the kernel splits the voxels into stride phases, and
a composition from 2-d launches would add a scatter over depth on top.  CplxConvTranspose3dFn mirrors
conv.CplxConvTranspose2dFn: forward = cplxamd_conv3d_dgrad with V = conj(W) and the bias inside the epilogue (one
rounding), backward = cplxamd_conv3d_fwd / cplxamd_conv3d_wgrad / cplxamd_chansum2.  Deviations from the reference:
`groups=1` by default (not 0), no float64 form, no second derivative.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib, ops
from ._lib import CplxAmdError, call, try_call, dtype_code, ntuple, ptr, require_device, stream_ptr  # noqa: F401
from .cplx import Cplx
from .conv import CplxConv2dFn, RealConv2dFn, _scratch


def _depth_out(D, k, s, p, d):
    return (D + 2 * p - d * (k - 1) - 1) // s + 1


def _tap(x, a, dd, sd, Dout):
    """depth tap `a` of a [B, C, Dp, H, W] tensor as a 2-d batch [B * Dout, C, H, W]"""
    xs = x[:, :, a * dd: a * dd + sd * (Dout - 1) + 1: sd]
    B, C, _, H, W = xs.shape
    return xs.permute(0, 2, 1, 3, 4).reshape(B * Dout, C, H, W)


def _fold(y, B, Dout):
    """[B * Dout, O, H', W'] -> [B, O, Dout, H', W']"""
    return y.view(B, Dout, *y.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()


def _prepare(planes, kd, stride, padding, dilation, padding_mode):
    """pads what the 2-d kernels cannot (depth; everything for circular mode) -> planes, 2-d padding"""
    (sd, sh, sw), (pd, ph, pw), (dd, dh, dw) = stride, padding, dilation
    if padding_mode == "circular":
        pads = []
        # symmetric_circular_padding (cplxmodule/cplx.py:699-712) hands `padding` to F.pad in its own
        # order and F.pad starts at the LAST dim: padding[0] wraps W, padding[2] wraps D
        for p in (pd, ph, pw):
            pads.extend(((p + 1) // 2, p // 2))
        planes = [F.pad(t, tuple(pads), mode="circular") for t in planes]
        pd = ph = pw = 0
    elif padding_mode != "zeros":
        raise ValueError("padding_mode must be 'zeros' or 'circular'.")
    elif pd:
        planes = [F.pad(t, (0, 0, 0, 0, pd, pd)) for t in planes]
    Dout = _depth_out(planes[0].shape[2], kd, sd, 0, dd)
    return planes, (ph, pw), Dout


def cplx_conv3d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                padding_mode="zeros"):
    stride, padding, dilation = ntuple(stride, 3), ntuple(padding, 3), ntuple(dilation, 3)
    kd = weight.shape[2]
    (xr, xi), pad2, Dout = _prepare([input.real, input.imag], kd, stride, padding, dilation, padding_mode)
    B = xr.shape[0]
    br, bi = (None, None) if bias is None else (bias.real, bias.imag)
    yr = yi = None
    for a in range(kd):
        tr, ti = CplxConv2dFn.apply(_tap(xr, a, dilation[0], stride[0], Dout),
                                    _tap(xi, a, dilation[0], stride[0], Dout),
                                    weight.real[:, :, a], weight.imag[:, :, a],
                                    br if a == 0 else None, bi if a == 0 else None,
                                    stride[1:], pad2, dilation[1:], groups, False)
        yr, yi = (tr, ti) if yr is None else (yr + tr, yi + ti)
    return Cplx(_fold(yr, B, Dout), _fold(yi, B, Dout))


def real_conv3d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    stride, padding, dilation = ntuple(stride, 3), ntuple(padding, 3), ntuple(dilation, 3)
    kd = w.shape[2]
    (x,), pad2, Dout = _prepare([x], kd, stride, padding, dilation, "zeros")
    B = x.shape[0]
    y = None
    for a in range(kd):
        t = RealConv2dFn.apply(_tap(x, a, dilation[0], stride[0], Dout), w[:, :, a],
                               b if a == 0 else None, stride[1:], pad2, dilation[1:], groups)
        y = t if y is None else y + t
    return _fold(y, B, Dout)


def _conv_args(layer):
    return layer.stride, layer.padding, layer.dilation, layer.groups


def cplx_conv3d_lrt(layer, input, eps=None):
    """Training-mode forward of CplxConv3dVD / ARD (complex/base.py:120-135 with F.conv3d)."""
    mu = cplx_conv3d(input, layer.weight, layer.bias, *_conv_args(layer))
    a = ops.Abs2Fn.apply(input.real, input.imag)
    S = ops.ExpFn.apply(layer.log_sigma2).to(a.dtype)
    s2 = real_conv3d(a, S, None, *_conv_args(layer)).float()
    if eps is not None:
        er, ei, seed, offset = eps.real.contiguous(), eps.imag.contiguous(), 0, 0
    else:
        er, ei, seed, offset = layer._draw_noise(mu.shape, input)
    return Cplx(*ops.ReparamFn.apply(mu.real, mu.imag, s2, er, ei, seed, offset))


def real_conv3d_layer(layer, input, eps=None):
    """Forward of Conv3dVD / ARD (real/base.py:116-163): eval -> mean only."""
    mu = real_conv3d(input, layer.weight, layer.bias, *_conv_args(layer))
    if not layer.training:
        return mu
    a = ops.Abs2Fn.apply(input, None)
    S = ops.ExpFn.apply(layer.log_sigma2).to(a.dtype)
    s2 = real_conv3d(a, S, None, *_conv_args(layer)).float()
    seed = offset = 0
    if eps is None:
        eps, seed, offset = layer._draw_noise(mu.shape, input)
    return ops.ReparamFn.apply(mu, None, s2, eps, None, seed, offset)[0]


# ------------------------------------------------------------------------------------------ #
#  transposed 3-d convolution on the native 3-d kernel (csrc/conv3d.hip)                      #
# ------------------------------------------------------------------------------------------ #
_PLAIN_DGRAD = False      # private: True runs the data gradient without stride phases (scripts/bench_conv_transpose3d.py only)


def _geom3(x_shape, w_shape, stride, padding, dilation, groups):
    """int[19] geometry of the forward correlation x [B, Ci, D, H, W] (*) w [Co, Ci / groups, KD, KH, KW] and its
    output shape (asked of the library: one formula)."""
    B, Ci, D, H, W = x_shape
    Co, _, KD, KH, KW = w_shape
    arr = (ctypes.c_int * 19)(B, Ci, Co, D, H, W, KD, KH, KW, *ntuple(stride, 3), *ntuple(padding, 3), *ntuple(dilation, 3),
                              groups)
    out = (ctypes.c_int * 3)()
    if not try_call("cplxamd_conv3d_out_shape", arr, ctypes.byref(out, 0), ctypes.byref(out, 4), ctypes.byref(out, 8)):
        raise ValueError(f"unsupported 3-d convolution geometry: input {tuple(x_shape)}, weight {tuple(w_shape)}, stride "
                         f"{stride}, padding {padding}, dilation {dilation}, groups {groups} (empty output, channels not "
                         "divisible by groups, or more than 2^31 voxels)")
    return arr, (B, Co, out[0], out[1], out[2])


def _transpose_out_shape3(x_shape, w_shape, stride, padding, output_padding, dilation, groups):
    B, _, D, H, W = x_shape
    _, Cog, KD, KH, KW = w_shape
    s, p, o, d = (ntuple(v, 3) for v in (stride, padding, output_padding, dilation))
    ext = [(L - 1) * s[n] - 2 * p[n] + d[n] * (k - 1) + o[n] + 1 for n, (L, k) in enumerate(((D, KD), (H, KH), (W, KW)))]
    return (B, Cog * groups, *ext)


def _chansum2(gr, gi):
    """The complex bias gradient (conv.chansum2, reached through this module's `call`): float32 ([C], [C])."""
    B, C = gr.shape[0], gr.shape[1]
    if gr.numel() == 0:
        return (torch.zeros(C, dtype=torch.float32, device=gr.device),) * 2
    out = torch.empty(2, C, dtype=torch.float32, device=gr.device)
    ws = _scratch(gr.device, 2 * 64 * C * 8)
    call("cplxamd_chansum2", ptr(gr), ptr(gi), ptr(out[0]), ptr(out[1]), B, C, gr.numel() // (B * C), dtype_code(gr),
         ptr(ws), stream_ptr())
    return out[0], out[1]


class CplxConvTranspose3dFn(torch.autograd.Function):
    """y = x (*)^T W + b without conjugation (cplx.conv_transposend_naive, cplxmodule/cplx.py:860-873) on planar
    [B, C, D, H, W] operands.  The transposed correlation is the adjoint of `Conv_V`, which the dgrad kernel computes as
    g -> g (*)^T conj(V); with V = conj(W) that is the forward pass here, bias in the epilogue.  Backward, by the same
    adjointness:  dx = Conv_V(gy) (the forward kernel),  dV = wgrad(g_out = x, input = gy),  dW = conj(dV),  db = sum gy."""

    @staticmethod
    def forward(ctx, xr, xi, wr, wi, br, bi, stride, padding, output_padding, dilation, groups, circular):
        require_device(xr, xi, wr, wi, br, bi)
        code = dtype_code(xr)
        if xi.dtype != xr.dtype:
            raise CplxAmdError(f"real and imaginary planes differ in dtype: {xr.dtype} vs {xi.dtype}")
        ctx.circular, ctx.xshape = circular, tuple(xr.shape)
        if circular:                       # (pads in F.pad order; padded HERE so that the backward folds dx before it rounds)
            xr, xi = F.pad(xr, circular, mode="circular"), F.pad(xi, circular, mode="circular")
        xr, xi = xr.contiguous(), xi.contiguous()
        if wr.shape[0] != xr.shape[1]:
            raise ValueError(f"expected {wr.shape[0]} input channels, got {xr.shape[1]}")
        yshape = _transpose_out_shape3(xr.shape, wr.shape, stride, padding, output_padding, dilation, groups)
        if min(yshape[2:]) <= 0:
            raise ValueError("transposed convolution output would be empty")
        geom, oshape = _geom3(yshape, wr.shape, stride, padding, dilation, groups)
        if tuple(oshape) != tuple(xr.shape):
            raise ValueError("output_padding must be smaller than either stride or dilation")
        vr, vi = ops.cast(wr.contiguous(), xr.dtype), ops.cast((-wi).contiguous(), xr.dtype)
        if br is not None:
            br, bi = br.float().contiguous(), bi.float().contiguous()
        yr, yi = torch.empty(yshape, dtype=xr.dtype, device=xr.device), torch.empty(yshape, dtype=xr.dtype, device=xr.device)
        call("cplxamd_conv3d_dgrad", ptr(xr), ptr(xi), ptr(vr), ptr(vi), ptr(br), ptr(bi), ptr(yr), ptr(yi), geom, code,
             1 if _PLAIN_DGRAD else 0, stream_ptr())
        ctx.save_for_backward(xr, xi, vr, vi)
        ctx.geom, ctx.has_bias, ctx.wshape = geom, br is not None, tuple(wr.shape)
        return yr, yi

    @staticmethod
    @ops.once_differentiable
    def backward(ctx, gr, gi):
        xr, xi, vr, vi = ctx.saved_tensors
        gr, gi = gr.contiguous(), gi.contiguous()
        code = dtype_code(gr)
        need = ctx.needs_input_grad
        dxr = dxi = dwr = dwi = dbr = dbi = None
        if need[0] or need[1]:
            if ctx.circular and xr.dtype != torch.float32:
                # the wrapped margins are ADDED into dx: float32 sums from the (exactly) widened operands, folded in
                # float32, rounded once -- folding bf16 results would round twice
                dxr, dxi = torch.empty_like(xr, dtype=torch.float32), torch.empty_like(xi, dtype=torch.float32)
                wide = [t.float() for t in (gr, gi, vr, vi)]          # (named: they must outlive the launch's pointers)
                call("cplxamd_conv3d_fwd", *(ptr(t) for t in wide), ptr(dxr), ptr(dxi), ctx.geom, _lib.F32, stream_ptr())
            else:
                dxr, dxi = torch.empty_like(xr), torch.empty_like(xi)
                call("cplxamd_conv3d_fwd", ptr(gr), ptr(gi), ptr(vr), ptr(vi), ptr(dxr), ptr(dxi), ctx.geom, code, stream_ptr())
            if ctx.circular:
                dxr, dxi = (_circular_fold(t, ctx.circular, ctx.xshape).to(xr.dtype) for t in (dxr, dxi))
        if need[2] or need[3]:
            dw = torch.empty((2,) + ctx.wshape, dtype=torch.float32, device=xr.device)
            nbytes = int(_lib_ws_bytes(ctx.geom))
            ws = _scratch(xr.device, nbytes)
            # (the roles swap: the layer's input x is the correlation's output gradient, gy its input)
            call("cplxamd_conv3d_wgrad", ptr(xr), ptr(xi), ptr(gr), ptr(gi), ptr(dw[0]), ptr(dw[1]), ctx.geom, code,
                 ptr(ws), ws.numel(), stream_ptr())
            dwr, dwi = dw[0], -dw[1]
        if ctx.has_bias and (need[4] or need[5]):
            dbr, dbi = _chansum2(gr, gi)
        return (dxr, dxi, dwr, dwi, dbr, dbi) + (None,) * 6


def _circular_pads(padding):
    """cplx.symmetric_circular_padding's F.pad argument: ((p + 1) // 2, p // 2) per entry of `padding`, and F.pad starts
    at the LAST dim -- padding[0] wraps W, padding[2] wraps D (cplxmodule/cplx.py:701-714)."""
    pads = []
    for p in ntuple(padding, 3):
        pads.extend(((p + 1) // 2, p // 2))
    return tuple(pads)


def _circular_fold(g, pads, shape):
    """Adjoint of F.pad(x, pads, mode='circular') for x of `shape`: the margins are added back onto the voxels they wrap."""
    for n in range(len(pads) // 2):
        dim, (lo, hi), L = g.dim() - 1 - n, pads[2 * n: 2 * n + 2], shape[-1 - n]
        core = g.narrow(dim, lo, L).clone()
        if lo:
            core.narrow(dim, L - lo, lo).add_(g.narrow(dim, 0, lo))
        if hi:
            core.narrow(dim, 0, hi).add_(g.narrow(dim, lo + L, hi))
        g = core
    return g


def _lib_ws_bytes(geom):
    n = _lib.load().cplxamd_conv3d_wgrad_ws_bytes(geom)
    if n < 0:
        raise CplxAmdError("cplxamd_conv3d_wgrad_ws_bytes failed: unsupported shape")
    return n


def cplx_conv_transpose3d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1,
                          padding_mode="zeros"):
    if input.dim() != 5 or weight.dim() != 5:
        raise ValueError(f"conv_transpose3d takes a [B, C, D, H, W] input and a [in, out / groups, kd, kh, kw] weight, got "
                         f"{tuple(input.shape)} and {tuple(weight.shape)}")
    stride, output_padding, dilation = ntuple(stride, 3), ntuple(output_padding, 3), ntuple(dilation, 3)
    circular = None
    if any(o < 0 or (o >= s and o >= d) for o, s, d in zip(output_padding, stride, dilation)):
        raise ValueError("output_padding must be smaller than either stride or dilation")
    if padding_mode == "circular":     # the reference pads the INPUT circularly, then runs padding 0
        circular, padding = _circular_pads(padding), 0
        if any(p > L for p, L in zip(circular, (input.shape[4],) * 2 + (input.shape[3],) * 2 + (input.shape[2],) * 2)):
            raise ValueError("circular padding must not exceed the input's extent")
    elif padding_mode != "zeros":
        raise ValueError("padding_mode must be 'zeros' or 'circular'.")
    br, bi = (None, None) if bias is None else (bias.real, bias.imag)
    yr, yi = CplxConvTranspose3dFn.apply(input.real, input.imag, weight.real, weight.imag, br, bi, stride,
                                         ntuple(padding, 3), output_padding, dilation, groups, circular)
    return Cplx(yr, yi)


def cplx_max_pool3d(input, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False):
    """[B, C, D, H, W]: largest modulus over (h, w) per depth slice, then over the depth window --
    the same element (first maximum in (d, h, w) order) a direct 3-d scan selects."""
    from . import cplx
    k = ntuple(kernel_size, 3)
    s = k if stride is None else ntuple(stride, 3)
    p, d = ntuple(padding, 3), ntuple(dilation, 3)
    B, C, D, H, W = input.shape
    flat = Cplx(input.real.reshape(B, C * D, H, W), input.imag.reshape(B, C * D, H, W))
    y = cplx.max_pool2d(flat, k[1:], s[1:], p[1:], d[1:], ceil_mode)
    Ho, Wo = y.shape[-2:]

    def depth_last(t):
        return t.view(B, C, D, Ho, Wo).permute(0, 1, 3, 4, 2).reshape(B, C * Ho * Wo, D)

    z = cplx.max_pool1d(Cplx(depth_last(y.real), depth_last(y.imag)), k[0], s[0], p[0], d[0], ceil_mode)
    Do = z.shape[-1]

    def depth_back(t):
        return t.view(B, C, Ho, Wo, Do).permute(0, 1, 4, 2, 3).contiguous()

    return Cplx(depth_back(z.real), depth_back(z.imag))
