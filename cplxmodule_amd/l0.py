"""LinearL0's hard-concrete gate around the real GEMM, and the L0 / LASSO penalties and masks (csrc/l0.hip, the
`real_l0` / `real_l1` kinds of csrc/kl.hip).

Reference: cplxmodule/nn/relevance/extensions/real/ell_zero.py:90-170 and lasso.py:7-19.  The gate multiplies one GEMM
operand (group None: the weight; "input": the input) or the GEMM result ("output") and is regenerated in the backward
from the uniform stream position (DESIGN.md "uniform stream"); only a supplied tape (noise modes "torch" / "tape") is
kept between the passes.  The gated operand is materialised once per step (W (.) z, x (.) z): fusing the gate into the
GEMM's operand loads is not done here.
"""
import torch

from . import _lib, x3
from ._lib import CplxAmdError, call, dtype_code, ptr, require_device, scratch, stream_ptr
from ._lib import al16 as _al16
from .ops import (_Pieces, _announce, _c, _f32, _noise_args, _real_linear_dw, _real_linear_dx, _real_linear_fwd, _ws,
                  colsum, grad_buffer, once_differentiable)

COLS, TRAIN, HARD = 1, 2, 4          # include/cplxamd.h CPLXAMD_L0_*


def _operand(t):
    """float32 or bf16 activations; anything else (float64 included) is the package's unsupported-dtype error."""
    dtype_code(t)
    return _al16(t.contiguous())


def philox_uniform(n, seed, offset, device):
    """The uniform stream of the gate, materialised (tests)."""
    u = torch.empty(n, dtype=torch.float32, device=device)
    require_device(u)
    call("cplxamd_philox_uniform", ptr(u), seed, offset, n, stream_ptr())
    return u


def _check_sizes(rows, cols, mode, la, *full):
    """Every [rows, cols] operand holds rows * cols elements; log_alpha one per column (COLS) or per element."""
    n = rows * cols
    if la.numel() != (cols if mode & COLS else n) or any(t is not None and t.numel() != n for t in full):
        raise CplxAmdError(f"L0 gate: operand sizes do not match [{rows}, {cols}] (mode {mode})")


def _noise(u, seed, offset):
    sd, of, st = _noise_args(seed, offset)
    return ptr(u), sd, of, st


def gate_fwd(a, la, rows, cols, mode, u=None, seed=0, offset=0, bias=None, out_dtype=None, total=False):
    """out = a (.) z (+ bias per column) as [rows, cols] in `out_dtype`; a None: z itself (the relevance mask).
    -> out, or (out, float64 sum of out) with total=True."""
    require_device(a, la, u, bias)
    la = _al16(_f32(la.contiguous()))
    a = None if a is None else _operand(a)
    u = None if u is None else _al16(_f32(u.contiguous()))
    bias = None if bias is None else _al16(_f32(bias.contiguous()))
    _check_sizes(rows, cols, mode, la, a, u if mode & TRAIN else None)
    if bias is not None and (not mode & COLS or bias.numel() != cols):
        raise CplxAmdError("L0 gate: the bias is one value per column of a per-column gate")
    out = torch.empty(rows, cols, dtype=out_dtype or (a.dtype if a is not None else torch.float32), device=la.device)
    tot = torch.empty((), dtype=torch.float64, device=la.device) if total else None
    pu, sd, of, st = _noise(u, seed, offset)
    call("cplxamd_l0_gate_fwd", ptr(a), ptr(la), pu, sd, of, st, ptr(bias), ptr(out), rows, cols, mode,
         dtype_code(a) if a is not None else _lib.F32, dtype_code(out), ptr(tot), ptr(_ws(la.device)) if total else None,
         stream_ptr())
    return (out, tot) if total else out


def gate_bwd(d, a, la, rows, cols, mode, u=None, seed=0, offset=0, da_dtype=None, az_dtype=None, da=None,
             dla=None):
    """(D (.) z [in `da` or a new da_dtype tensor; da_dtype False: not formed], A (.) z [az_dtype None: not formed],
    d log_alpha [elementwise, or summed over the rows per column with COLS -- deterministic])."""
    require_device(d, a, la, u)
    d, a = _operand(d), _operand(a)
    la = _al16(_f32(la.contiguous()))
    u = None if u is None else _al16(_f32(u.contiguous()))
    _check_sizes(rows, cols, mode, la, d, a, da, u if mode & TRAIN else None)
    if dla is not None and dla.numel() != la.numel():
        raise CplxAmdError("L0 gate: d log_alpha must have log_alpha's size")
    if da is None and da_dtype is not False:
        da = torch.empty(rows, cols, dtype=da_dtype or d.dtype, device=d.device)
    az = None if az_dtype is None else torch.empty(rows, cols, dtype=az_dtype, device=d.device)
    if dla is None:
        dla = torch.empty(la.shape, dtype=torch.float32, device=d.device)
    ws, nb = None, 0
    if mode & COLS:
        ws = scratch("l0_bwd", d.device, int(_lib.load().cplxamd_l0_gate_bwd_ws_bytes(rows, cols)), 1 << 16)
        nb = ws.numel()
    pu, sd, of, st = _noise(u, seed, offset)
    call("cplxamd_l0_gate_bwd", ptr(d), ptr(a), ptr(la), pu, sd, of, st, ptr(da), ptr(az), ptr(dla), rows, cols, mode,
         dtype_code(d), dtype_code(a), dtype_code(da) if da is not None else _lib.F32,
         dtype_code(az) if az is not None else _lib.F32, ptr(ws), nb, stream_ptr())
    return da, az, dla


def l1_mask(w, threshold, count=False):
    """LASSO relevance log(|w| + 1e-20) >= threshold as a bool tensor of w's shape (+ the float64 count of ones)."""
    require_device(w)
    w = _f32(w.contiguous())
    mask = torch.empty(w.shape, dtype=torch.bool, device=w.device)
    cnt = torch.empty((), dtype=torch.float64, device=w.device) if count else None
    call("cplxamd_l1_mask", ptr(w), float(threshold), ptr(mask), ptr(cnt), ptr(_ws(w.device)) if count else None,
         w.numel(), stream_ptr())
    return (mask, cnt) if count else mask


# ------------------------------------------------------------------------------------------ #
#  the three forms of LinearL0.forward (ell_zero.py:121-132), bias added after the gate        #
# ------------------------------------------------------------------------------------------ #
def _stash(ctx, u, seed):
    """Tensors of the noise position the backward regenerates the gate from: a supplied tape, or the device state."""
    return (u, seed if isinstance(seed, torch.Tensor) else None)


def _unstash(ctx, u, st):
    return u, (st if st is not None else ctx.seed), ctx.offset


class L0LinearFn(torch.autograd.Function):
    """group None: y = x (W (.) z)^T + b, z = gate(log_alpha [O, I])."""

    @staticmethod
    def forward(ctx, x, w, b, la, u, seed, offset, train):
        require_device(x, w, b, la, u)
        O, I = w.shape
        x2 = _operand(x.reshape(-1, I))
        mode = TRAIN if train else 0
        wz = gate_fwd(w, la, O, I, mode, u, seed, offset, out_dtype=x2.dtype)
        ctx.mode = x3.get_fp32_mode()
        y, ctx.wz = _real_linear_fwd(x2, wz, _c(b), mode=ctx.mode, xs=_Pieces(x2))
        ctx.save_for_backward(x2, w, la, *_stash(ctx, u, seed))
        ctx.gmode, ctx.seed, ctx.offset = mode, seed, offset
        ctx.has_bias, ctx.lead = b is not None, x.shape[:-1]
        return y.view(*ctx.lead, O)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, w, la, u, st = ctx.saved_tensors
        u, seed, offset = _unstash(ctx, u, st)
        O, I = w.shape
        need = ctx.needs_input_grad
        g2 = _operand(g.reshape(-1, O))
        gs = _Pieces(g2)
        dx = dw = db = dla = None
        if need[1] or need[3]:
            D = _real_linear_dw(g2, x2, mode=ctx.mode, gs=gs)                 # G^T x = d(W (.) z), float32
            dw = grad_buffer(w) if need[1] else None
            dla = grad_buffer(la) if need[3] else None
            dw, _, dla = gate_bwd(D, w, la, O, I, ctx.gmode, u, seed, offset, da_dtype=torch.float32 if need[1] else False,
                                  da=dw, dla=dla)
            _announce(w if need[1] else None, la if need[3] else None)
            dw = dw if need[1] else None
            dla = dla if need[3] else None
        if ctx.has_bias and need[2]:
            db = colsum(g2)
        if need[0]:
            dx = _real_linear_dx(g2, ctx.wz, x2.dtype, mode=ctx.mode, gs=gs).view(*ctx.lead, I)
        return dx, dw, db, dla, None, None, None, None


class L0InputLinearFn(torch.autograd.Function):
    """group "input": y = (x (.) z) W^T + b, z = gate(log_alpha [1, I]) drawn per sample ([*lead, 1, I] uniforms)."""

    @staticmethod
    def forward(ctx, x, w, b, la, u, seed, offset, train):
        require_device(x, w, b, la, u)
        O, I = w.shape
        x2 = _operand(x.reshape(-1, I))
        B = x2.shape[0]
        mode = COLS | (TRAIN if train else 0)
        xz = gate_fwd(x2, la, B, I, mode, u, seed, offset)
        ctx.mode = x3.get_fp32_mode()
        y, ctx.wm = _real_linear_fwd(xz, _c(w), _c(b), mode=ctx.mode, xs=_Pieces(xz))
        ctx.save_for_backward(x2, w, la, *_stash(ctx, u, seed))          # (x (.) z is formed again in the backward)
        ctx.gmode, ctx.seed, ctx.offset = mode, seed, offset
        ctx.has_bias, ctx.lead = b is not None, x.shape[:-1]
        return y.view(*ctx.lead, O)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, w, la, u, st = ctx.saved_tensors
        u, seed, offset = _unstash(ctx, u, st)
        O, I = w.shape
        B = x2.shape[0]
        need = ctx.needs_input_grad
        g2 = _operand(g.reshape(-1, O))
        gs = _Pieces(g2)
        dx = dw = db = dla = None
        # d(x (.) z) = G W in float32, then ONE pass: dx = that (.) z, d log_alpha (column sums), x (.) z for dW
        dxz = _real_linear_dx(g2, ctx.wm, torch.float32, mode=ctx.mode, gs=gs)
        dla = grad_buffer(la) if need[3] else None
        dx, xz, dla = gate_bwd(dxz, x2, la, B, I, ctx.gmode, u, seed, offset,
                               da_dtype=x2.dtype if need[0] else False,
                               az_dtype=x2.dtype if need[1] else None, dla=dla)
        if need[1]:
            dw = grad_buffer(w)
            _real_linear_dw(g2, xz, out=dw, mode=ctx.mode, gs=gs)
        _announce(w if need[1] else None, la if need[3] else None)
        if ctx.has_bias and need[2]:
            db = colsum(g2)
        dx = dx.view(*ctx.lead, I) if need[0] else None
        return dx, dw, db, (dla if need[3] else None), None, None, None, None


class L0OutputLinearFn(torch.autograd.Function):
    """group "output": y = (x W^T) (.) z + b, z = gate(log_alpha [O, 1]) drawn per sample ([*lead, O, 1] uniforms)."""

    @staticmethod
    def forward(ctx, x, w, b, la, u, seed, offset, train):
        require_device(x, w, b, la, u)
        O, I = w.shape
        x2 = _operand(x.reshape(-1, I))
        B = x2.shape[0]
        mode = COLS | (TRAIN if train else 0)
        ctx.mode = x3.get_fp32_mode()
        pre, ctx.wm = _real_linear_fwd(x2, _c(w), None, out_dtype=torch.float32, mode=ctx.mode, xs=_Pieces(x2))
        y = gate_fwd(pre, la, B, O, mode, u, seed, offset, bias=b, out_dtype=x2.dtype)
        ctx.save_for_backward(x2, w, la, pre, *_stash(ctx, u, seed))
        ctx.gmode, ctx.seed, ctx.offset = mode, seed, offset
        ctx.has_bias, ctx.lead = b is not None, x.shape[:-1]
        return y.view(*ctx.lead, O)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, w, la, pre, u, st = ctx.saved_tensors
        u, seed, offset = _unstash(ctx, u, st)
        O, I = w.shape
        B = x2.shape[0]
        need = ctx.needs_input_grad
        g2 = _operand(g.reshape(-1, O))
        dx = dw = db = dla = None
        dla = grad_buffer(la) if need[3] else None
        dpre, _, dla = gate_bwd(g2, pre, la, B, O, ctx.gmode, u, seed, offset, dla=dla)      # G (.) z, d log_alpha
        gs = _Pieces(dpre)
        if need[1]:
            dw = grad_buffer(w)
            _real_linear_dw(dpre, x2, out=dw, mode=ctx.mode, gs=gs)
        _announce(w if need[1] else None, la if need[3] else None)
        if ctx.has_bias and need[2]:
            db = colsum(g2)
        if need[0]:
            dx = _real_linear_dx(dpre, ctx.wm, x2.dtype, mode=ctx.mode, gs=gs).view(*ctx.lead, I)
        return dx, dw, db, (dla if need[3] else None), None, None, None, None


# ------------------------------------------------------------------------------------------ #
#  penalties of one parameter (kl.hip kinds real_l0 / real_l1)                                #
# ------------------------------------------------------------------------------------------ #
def _grads(kind, p, g_elem=None, g_scalar=None):
    require_device(p, g_elem, g_scalar)
    p = _f32(p.contiguous())
    g = torch.empty_like(p)
    l0 = kind == "real_l0"
    if g_scalar is not None:
        g_scalar = _f32(g_scalar.reshape(()).contiguous())
    call("cplxamd_vd_kl_bwd", ptr(p), None, ptr(p), _lib.KL_KINDS[kind], ptr(None if g_elem is None else
         _f32(g_elem.contiguous())), ptr(g_scalar), ptr(g if l0 else None), ptr(None if l0 else g), None, p.numel(),
         stream_ptr())
    return g


class OneParamPenaltyFn(torch.autograd.Function):
    """The elementwise penalty tensor: sigmoid(shift - log_alpha) (kind real_l0) or |w| (real_l1)."""

    @staticmethod
    def forward(ctx, kind, p):
        require_device(p)
        pc = _f32(p.contiguous())
        elem = torch.empty_like(pc)
        call("cplxamd_vd_kl_fwd", ptr(pc), None, ptr(pc), _lib.KL_KINDS[kind], ptr(elem), None, None, pc.numel(),
             stream_ptr())
        ctx.kind = kind
        ctx.save_for_backward(pc)
        return elem.view_as(p)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return None, _grads(ctx.kind, p, g_elem=g).view_as(g)


class OneParamPenaltySumFn(torch.autograd.Function):
    """sum of the penalty in one fused pass; the backward scales by the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, kind, p):
        require_device(p)
        pc = _f32(p.contiguous())
        tot = torch.empty((), dtype=torch.float32, device=p.device)
        call("cplxamd_vd_kl_fwd", ptr(pc), None, ptr(pc), _lib.KL_KINDS[kind], None, ptr(tot), ptr(_ws(p.device)),
             pc.numel(), stream_ptr())
        ctx.kind = kind
        ctx.save_for_backward(pc)
        return tot

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return None, _grads(ctx.kind, p, g_scalar=g).view(ctx.saved_tensors[0].shape)


def check_param(t):
    if t.dtype != torch.float32:
        raise CplxAmdError(f"unsupported dtype {t.dtype}: LinearL0 / LinearLASSO take float32 parameters (bf16 or "
                           "float32 activations); there is no float64 route for these layers")
    return t
