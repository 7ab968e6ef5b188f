"""The masked layers' route on compacted operands (cplxmodule_amd/compact.py, csrc/compact.hip): the live-index kernel,
the gather / expand / compact-weight passes bit for bit against torch on the CPU, and the four layers with the route on
and off against one float64 reference.

Tolerances (README "Tolerances"): float32 rtol 1e-5 + atol 1e-5 max|ref|; bf16 as the dense bf16 tests hold the same
layers (tests/test_gpu_linear.py test_bf16_layer_vs_oracle: outputs 1e-2, gradients 3e-2; tests/test_gpu_conv_cl.py:
outputs 1e-2, gradients 2e-2, all norm-wise); index lists, copies and the zeros of masked entries are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 1030)
PATTERNS = ("live", "dead", "first", "last", "alternating", "random10", "soft")


def _pattern(name, O, C, T, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(O, C, T)
    if name == "live":
        m += 1
    elif name == "first":
        m[0, 0] = 1
    elif name == "last":
        m[-1, -1, -1] = 1
    elif name == "alternating":
        m[::2, ::2] = 1
    elif name == "random10":
        m = (torch.rand(O, C, T, generator=g) < 0.1).float()
        m[torch.rand(O, generator=g) < 0.5] = 0                   # whole rows and columns dead
        m[:, torch.rand(C, generator=g) < 0.5] = 0
    elif name == "soft":
        m = (torch.rand(O, C, T, generator=g) < 0.05).float() * 0.5
        m[:, ::3] = 0
    return m


def _check_live_index(m, granule=1):
    from cplxmodule_amd import compact
    O, C, T = m.shape
    md = m.to(DEV)
    a = [t.cpu() for t in compact.live_index(md, granule)]
    b = [t.cpu() for t in compact.live_index(md, granule)]
    live_r = torch.nonzero(m.ne(0).any(2).any(1)).flatten().tolist()
    live_c = torch.nonzero(m.ne(0).any(2).any(0)).flatten().tolist()
    want_r, want_c = compact.pad_live(live_r, O, granule), compact.pad_live(live_c, C, granule)
    rows, cols, inv_rows, inv_cols, counts = a
    assert counts.tolist() == [len(live_r), len(want_r), len(live_c), len(want_c)]
    assert rows[:len(want_r)].tolist() == want_r and cols[:len(want_c)].tolist() == want_c
    for inv, lst, n in ((inv_rows, want_r, O), (inv_cols, want_c, C)):
        ref = torch.full((n,), -1, dtype=torch.int32)
        ref[torch.tensor(lst, dtype=torch.long)] = torch.arange(len(lst), dtype=torch.int32)
        assert torch.equal(inv, ref)
    # two runs: identical bits (the defined prefix of the lists, everything else in full)
    assert torch.equal(a[0][:len(want_r)], b[0][:len(want_r)]) and torch.equal(a[1][:len(want_c)], b[1][:len(want_c)])
    assert all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))


@pytest.mark.parametrize("T", (1, 9))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_live_index_matches_torch(pattern, T):
    for k, (O, C) in enumerate((o, c) for o in SIZES for c in SIZES):
        _check_live_index(_pattern(pattern, O, C, T, 100 * k + T))


def test_live_index_long_axis_and_granule():
    m = _pattern("random10", 3, 70000, 1, 5)            # more than one pass of the scan block (4096 indices per pass)
    assert 0 < int(m.ne(0).any(0).sum()) < 70000
    _check_live_index(m)
    _check_live_index(m.reshape(70000, 3, 1).contiguous())
    for pattern in ("random10", "first", "last", "dead", "live", "alternating"):       # the padded lists of the plan
        _check_live_index(_pattern(pattern, 257, 130, 9, 9), granule=64)
        _check_live_index(_pattern(pattern, 65, 1030, 1, 10), granule=64)


def _offset(t, off):
    """The same values behind a pointer `off` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


AXES, INNERS = (1, 63, 64, 65, 130), (1, 3, 8, 9, 81)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_gather_and_expand_bit_exact(dtype):
    from cplxmodule_amd import compact
    g = torch.Generator().manual_seed(1)
    for outer in (1, 5):
        for A in AXES:
            for inner in INNERS:
                for off in (0, 1):
                    n = int(torch.randint(0, A + 1, (1,), generator=g))
                    idx = torch.sort(torch.randperm(A, generator=g)[:n]).values
                    inv = torch.full((A,), -1, dtype=torch.int32)
                    inv[idx] = torch.arange(n, dtype=torch.int32)
                    sr, si = (torch.randn(outer, A, inner, generator=g).to(dtype) for _ in range(2))
                    dr, di = (_offset(t.to(DEV), off) for t in (sr, si))
                    idx_d, inv_d = idx.to(DEV, torch.int32), inv.to(DEV)
                    what = (outer, A, inner, off, n)
                    # gather: two planes, and one plane alone
                    gr, gi = compact.gather(dr, di, idx_d, 1)
                    assert torch.equal(gr.cpu(), sr.index_select(1, idx)) and torch.equal(gi.cpu(), si.index_select(1, idx)), what
                    g1, none = compact.gather(di, None, idx_d, 1)
                    assert none is None and torch.equal(g1.cpu(), si.index_select(1, idx)), what
                    # expand: into a filled tensor, and into zeros
                    cr, ci = (torch.randn(outer, n, inner, generator=g).to(dtype) for _ in range(2))
                    fr, fi = torch.randn(A, generator=g), torch.randn(A, generator=g)
                    er, ei = compact.expand(_offset(cr.to(DEV), off), _offset(ci.to(DEV), off), inv_d, 1, (fr.to(DEV), fi.to(DEV)))
                    for got, src, fill in ((er, cr, fr), (ei, ci, fi)):
                        ref = fill.to(dtype)[None, :, None].expand(outer, A, inner).clone().index_copy_(1, idx, src)
                        assert torch.equal(got.cpu(), ref), what
                    e0, none = compact.expand(_offset(cr.to(DEV), off), None, inv_d, 1)
                    assert none is None
                    assert torch.equal(e0.cpu(), torch.zeros(outer, A, inner, dtype=dtype).index_copy_(1, idx, cr)), what


def test_gather_expand_layouts():
    """The views the layers use: the last dimension of [.., I], the channels of NCHW and of channels-last tensors
    (which stay channels-last), a bias."""
    from cplxmodule_amd import compact
    x = torch.randn(3, 5, 70)
    idx = torch.tensor([0, 3, 4, 69])
    got, _ = compact.gather(x.to(DEV), None, idx.to(DEV, torch.int32), -1)
    assert torch.equal(got.cpu(), x[..., idx])
    img = torch.randn(2, 12, 5, 7)
    ch = torch.tensor([1, 2, 8, 11])
    inv = torch.full((12,), -1, dtype=torch.int32)
    inv[ch] = torch.arange(4, dtype=torch.int32)
    for fmt in (torch.contiguous_format, torch.channels_last):
        d = img.to(DEV).contiguous(memory_format=fmt)
        got, _ = compact.gather(d, None, ch.to(DEV, torch.int32), 1)
        assert got.is_contiguous(memory_format=fmt) and torch.equal(got.cpu(), img[:, ch])
        back, _ = compact.expand(got, None, inv.to(DEV), 1)
        assert back.is_contiguous(memory_format=fmt)
        assert torch.equal(back.cpu(), torch.zeros_like(img).index_copy_(1, ch, img[:, ch]))
    b = torch.randn(12)
    got, _ = compact.gather(b.to(DEV), None, ch.to(DEV, torch.int32), 0)
    assert torch.equal(got.cpu(), b[ch])


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("in_dtype", (torch.float32, torch.bfloat16))
def test_compact_and_expand_weight_bit_exact(in_dtype, out_dtype):
    from cplxmodule_amd import compact
    g = torch.Generator().manual_seed(2)
    for O, C, T in ((1, 1, 1), (63, 65, 1), (64, 130, 1), (65, 64, 9), (130, 63, 3), (5, 8, 81)):
        for off in (0, 1):
            mask = (torch.rand(O, C, T, generator=g) < 0.6).float() * torch.where(torch.rand(O, C, T, generator=g) < 0.5, 1.0, 0.5)
            rows = torch.sort(torch.randperm(O, generator=g)[:max(1, O // 2)]).values
            cols = torch.sort(torch.randperm(C, generator=g)[:max(1, (2 * C) // 3)]).values
            wr, wi = (torch.randn(O, C, T, generator=g).to(in_dtype) for _ in range(2))
            args = (mask.to(DEV), rows.to(DEV, torch.int32), cols.to(DEV, torch.int32))
            cr, ci = compact.compact_weight(_offset(wr.to(DEV), off), _offset(wi.to(DEV), off), *args, out_dtype)
            for got, w in ((cr, wr), (ci, wi)):
                assert got.dtype == out_dtype
                assert torch.equal(got.cpu(), (w.float() * mask)[rows][:, cols].to(out_dtype)), (O, C, T, off)
            c1, none = compact.compact_weight(wr.to(DEV), None, *args, out_dtype)
            assert none is None and torch.equal(c1, cr)
            # the adjoint: scatter back with the mask, exact zeros elsewhere
            inv_r, inv_c = torch.full((O,), -1, dtype=torch.int32), torch.full((C,), -1, dtype=torch.int32)
            inv_r[rows] = torch.arange(len(rows), dtype=torch.int32)
            inv_c[cols] = torch.arange(len(cols), dtype=torch.int32)
            sr, si = (torch.randn(len(rows), len(cols), T, generator=g).to(in_dtype) for _ in range(2))
            er, ei = compact.expand_weight(_offset(sr.to(DEV), off), _offset(si.to(DEV), off), mask.to(DEV), inv_r.to(DEV),
                                           inv_c.to(DEV), out_dtype)
            for got, s in ((er, sr), (ei, si)):
                full = torch.zeros(O, C, T)
                full[rows[:, None], cols[None, :]] = s.float()
                assert torch.equal(got.cpu(), (full * mask).to(out_dtype)), (O, C, T, off)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_c_abi_unaligned_outputs_take_the_element_path(dtype):
    """The host wrappers always allocate aligned outputs; the C entry points also accept outputs that are not 16-byte
    aligned (shapes that would otherwise take the 16-byte stores) and then store element by element."""
    from cplxmodule_amd import _lib
    from cplxmodule_amd._lib import call, dtype_code, ptr, stream_ptr
    g = torch.Generator().manual_seed(4)
    outer, A, J, inner = 3, 16, 8, 8
    idx = torch.sort(torch.randperm(A, generator=g)[:J]).values
    inv = torch.full((A,), -1, dtype=torch.int32)
    inv[idx] = torch.arange(J, dtype=torch.int32)
    idx_d, inv_d = idx.to(DEV, torch.int32), inv.to(DEV)
    src = [torch.randn(outer, A, inner, generator=g).to(dtype) for _ in range(2)]
    sd = [t.to(DEV) for t in src]
    out = [_offset(torch.zeros(outer, J, inner, dtype=dtype, device=DEV), 1) for _ in range(2)]
    assert all(t.data_ptr() % 16 != 0 for t in out)
    call("cplxamd_gather_axis", ptr(sd[0]), ptr(sd[1]), ptr(idx_d), ptr(out[0]), ptr(out[1]), outer, A, J, inner,
         dtype_code(sd[0]), stream_ptr())
    assert all(torch.equal(o.cpu(), t.index_select(1, idx)) for o, t in zip(out, src))
    small = [t.index_select(1, idx) for t in src]
    fill = [torch.randn(A, generator=g) for _ in range(2)]
    full = [_offset(torch.zeros(outer, A, inner, dtype=dtype, device=DEV), 1) for _ in range(2)]
    small_d, fill_d = [t.to(DEV) for t in small], [t.to(DEV) for t in fill]      # (held: ptr() keeps no reference)
    call("cplxamd_expand_axis", ptr(small_d[0]), ptr(small_d[1]), ptr(inv_d), ptr(fill_d[0]), ptr(fill_d[1]), ptr(full[0]),
         ptr(full[1]), outer, J, A, inner, dtype_code(full[0]), stream_ptr())
    for o, t, f in zip(full, small, fill):
        assert torch.equal(o.cpu(), f.to(dtype)[None, :, None].expand(outer, A, inner).clone().index_copy_(1, idx, t))
    # the weight pair: [O, C, T] = [16, 16, 4] float32 in, `dtype` out
    O = C = 16
    T = 4
    mask = (torch.rand(O, C, T, generator=g) < 0.6).float() * 0.5
    w = [torch.randn(O, C, T, generator=g) for _ in range(2)]
    cw = [_offset(torch.zeros(J, J, T, dtype=dtype, device=DEV), 1) for _ in range(2)]
    w_d, mask_d = [t.to(DEV) for t in w], mask.to(DEV)
    call("cplxamd_compact_weight", ptr(w_d[0]), ptr(w_d[1]), ptr(mask_d), ptr(idx_d), ptr(idx_d), ptr(cw[0]),
         ptr(cw[1]), O, C, T, J, J, _lib.F32, dtype_code(cw[0]), stream_ptr())
    for o, t in zip(cw, w):
        assert torch.equal(o.cpu(), (t * mask)[idx][:, idx].to(dtype))
    s = [torch.randn(J, J, T, generator=g) for _ in range(2)]
    ew = [_offset(torch.zeros(O, C, T, dtype=dtype, device=DEV), 1) for _ in range(2)]
    s_d = [t.to(DEV) for t in s]
    call("cplxamd_expand_weight", ptr(s_d[0]), ptr(s_d[1]), ptr(mask_d), ptr(inv_d), ptr(inv_d), ptr(ew[0]),
         ptr(ew[1]), O, C, T, J, J, _lib.F32, dtype_code(ew[0]), stream_ptr())
    for o, t in zip(ew, s):
        ref = torch.zeros(O, C, T)
        ref[idx[:, None], idx[None, :]] = t
        assert torch.equal(o.cpu(), (ref * mask).to(dtype))


# ---- the layers ----------------------------------------------------------------------------------------------------------
def _structured_mask(shape, live_rows, live_cols, seed, soft=False):
    """Dead rows and columns plus scattered zeros inside the live part (every live row / column keeps an entry)."""
    g = torch.Generator().manual_seed(seed)
    O, C = shape[:2]
    rows = torch.sort(torch.randperm(O, generator=g)[:live_rows]).values
    cols = torch.sort(torch.randperm(C, generator=g)[:live_cols]).values
    inner = (torch.rand(live_rows, live_cols, *shape[2:], generator=g) < 0.7).float()
    inner[torch.arange(live_rows), torch.arange(live_rows) % live_cols] = 1
    inner[torch.arange(live_cols) % live_rows, torch.arange(live_cols)] = 1
    if soft:
        inner = inner * 0.5
    m = torch.zeros(shape)
    m[rows[:, None], cols[None, :]] = inner
    return m


def _bf16_exact_(layer):
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(p.bfloat16().float())


CASES = {
    # name: (kind, cplx, dtype, x shape, layer args, layer kwargs, live rows, live cols, channels-last, (y tol, grad tol))
    "cplx_linear_f32": ("linear", True, torch.float32, (48, 130), (130, 70), {}, 20, 50, False, (1e-5, 1e-5)),
    "real_linear_f32": ("linear", False, torch.float32, (48, 130), (130, 70), {}, 20, 50, False, (1e-5, 1e-5)),
    "cplx_linear_bf16": ("linear", True, torch.bfloat16, (64, 256), (256, 192), {}, 100, 60, False, (1e-2, 3e-2)),
    "real_linear_bf16": ("linear", False, torch.bfloat16, (64, 256), (256, 192), {}, 100, 60, False, (1e-2, 3e-2)),
    # (6 -> 10 channels: the granule pads both lists to the full size, so this case runs dense with the flag on)
    "cplx_conv_nchw_f32": ("conv", True, torch.float32, (2, 6, 9, 9), (6, 10, 3), dict(padding=1), 4, 3, False, (1e-5, 1e-5)),
    "real_conv_nchw_f32": ("conv", False, torch.float32, (2, 6, 9, 9), (6, 10, 3), dict(padding=1), 4, 3, False, (1e-5, 1e-5)),
    # (the smallest NCHW float32 shape at which the route IS taken: more than 64 channels on both sides)
    "cplx_conv_nchw_f32_wide": ("conv", True, torch.float32, (2, 70, 9, 9), (70, 72, 3), dict(padding=1), 20, 30, False,
                                (1e-5, 1e-5)),
    "real_conv_nchw_f32_wide": ("conv", False, torch.float32, (2, 70, 9, 9), (70, 72, 3), dict(padding=1), 20, 30, False,
                                (1e-5, 1e-5)),
    "cplx_conv_cl_bf16": ("conv", True, torch.bfloat16, (2, 128, 16, 16), (128, 128, 3), dict(padding=1), 64, 64, True,
                          (1e-2, 2e-2)),
    "real_conv_cl_bf16": ("conv", False, torch.bfloat16, (2, 128, 16, 16), (128, 128, 3), dict(padding=1), 64, 64, True,
                          (1e-2, 2e-2)),
}


def _make(case, seed=0, soft=False):
    from cplxmodule_amd.nn import masked
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, tol = CASES[case]
    torch.manual_seed(seed)
    cls = {("linear", True): masked.CplxLinearMasked, ("linear", False): masked.LinearMasked,
           ("conv", True): masked.CplxConv2dMasked, ("conv", False): masked.Conv2dMasked}[kind, cplx]
    layer = cls(*args, **kwargs)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 1:
                p.normal_()                       # a bias that is visible at the dead features
    if dtype == torch.bfloat16:
        _bf16_exact_(layer)
    layer = layer.to(DEV)
    wshape = (layer.weight.real if cplx else layer.weight).shape
    layer.mask = _structured_mask(tuple(wshape), lr, lc, seed + 1, soft)
    planes = 2 if cplx else 1
    xs = [torch.randn(xshape).to(dtype) for _ in range(planes)]
    return layer, xs, cl


def _forward(layer, xs, cl, cplx):
    from cplxmodule_amd import Cplx
    leaves = [t.to(DEV).clone() for t in xs]
    if cl:
        leaves = [t.contiguous(memory_format=torch.channels_last) for t in leaves]
    leaves = [t.requires_grad_(True) for t in leaves]
    y = layer(Cplx(*leaves) if cplx else leaves[0])
    return leaves, ((y.real, y.imag) if cplx else (y,))


def _params(layer, cplx):
    if cplx:
        return [layer.weight.real, layer.weight.imag], [layer.bias.real, layer.bias.imag]
    return [layer.weight], [layer.bias]


def _reference(case, layer, xs, gs):
    """float64 torch on the CPU: linear / conv2d(x, w * mask, b) and its gradients."""
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, tol = CASES[case]
    ws, bs = _params(layer, cplx)
    mask = layer.mask.detach().double().cpu()
    x = [t.double().requires_grad_(True) for t in xs]
    w = [t.detach().double().cpu().requires_grad_(True) for t in ws]
    b = [t.detach().double().cpu().requires_grad_(True) for t in bs]
    op = (lambda a, k, bias=None: F.linear(a, k * mask, bias)) if kind == "linear" else \
        (lambda a, k, bias=None: F.conv2d(a, k * mask, bias, padding=kwargs.get("padding", 0)))
    if cplx:
        y = [op(x[0], w[0], b[0]) - op(x[1], w[1]), op(x[0], w[1], b[1]) + op(x[1], w[0])]
    else:
        y = [op(x[0], w[0], b[0])]
    sum((a * g.double()).sum() for a, g in zip(y, gs)).backward()
    n = lambda ts: [t.detach().numpy() for t in ts]  # noqa: E731
    return dict(y=n(y), dx=n([t.grad for t in x]), dw=n([t.grad for t in w]), db=n([t.grad for t in b]))


@pytest.mark.parametrize("case", sorted(CASES))
def test_layer_parity_route_on_and_off(case):
    from cplxmodule_amd.nn import masked
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, (ytol, gtol) = CASES[case]
    layer, xs, cl = _make(case)
    gs = [torch.randn(*((xshape[0], args[1]) if kind == "linear" else (xshape[0], args[1]) + tuple(xshape[2:]))).to(dtype)
          for _ in xs]
    ref = _reference(case, layer, xs, gs)
    mask = layer.mask.cpu()
    dead_out = ~mask.flatten(1).ne(0).any(1)
    dead_in = ~mask.transpose(0, 1).flatten(1).ne(0).any(1)
    assert dead_out.any() and dead_in.any()
    ws, bs = _params(layer, cplx)
    wide = max(args[0], args[1]) > 64
    for on in (True, False):
        masked.compact_(layer, enabled=on, max_live=1.0)
        assert masked.compaction(layer)[""]["active"] is (on and wide)
        layer.zero_grad(set_to_none=True)
        leaves, y = _forward(layer, xs, cl, cplx)
        sum((a * g.to(DEV)).sum() for a, g in zip(y, gs)).backward()
        got = dict(y=y, dx=[t.grad for t in leaves], dw=[t.grad for t in ws], db=[t.grad for t in bs])
        for name, tol in (("y", ytol), ("dx", gtol), ("dw", gtol), ("db", gtol)):
            for k, (a, b) in enumerate(zip(got[name], ref[name])):
                a = a.detach().float().cpu().numpy()
                print(f"{case} route={'on' if on else 'off'} {name}[{k}] max err / max ref = "
                      f"{np.abs(a - b).max() / np.abs(b).max():.3e} (asked {tol:g})")
                np.testing.assert_allclose(a, b, rtol=tol, atol=tol * float(np.abs(b).max()), err_msg=f"{name}[{k}] on={on}")
        if on:
            for k, yk in enumerate(y):        # dead output features: the bias in the output dtype, bit for bit
                bias = bs[k].detach().to(yk.dtype)
                want = bias[dead_out.to(DEV)]
                sel = yk.detach()[:, dead_out.to(DEV)]
                assert torch.equal(sel, want.view(1, -1, *([1] * (sel.dim() - 2))).expand_as(sel))
            for t in leaves:                   # dead input features: exact zeros
                d = t.grad[..., dead_in.to(DEV)] if kind == "linear" else t.grad[:, dead_in.to(DEV)]
                assert d.numel() > 0 and (d == 0).all()
            for t in ws:                       # masked weights: exact zeros
                assert (t.grad[mask.to(DEV) == 0] == 0).all()


@pytest.mark.parametrize("case", ("cplx_linear_f32", "real_linear_bf16", "cplx_conv_nchw_f32_wide", "real_conv_cl_bf16"))
def test_soft_mask_stays_soft(case):
    """A mask of 0.5 entries: the compacted weight is weight * mask, not a binarised one."""
    from cplxmodule_amd.nn import masked
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, (ytol, gtol) = CASES[case]
    layer, xs, cl = _make(case, seed=3, soft=True)
    outs = []
    for on in (True, False):
        masked.compact_(layer, enabled=on, max_live=1.0)
        outs.append(_forward(layer, xs, cl, cplx)[1])
    for a, b in zip(*outs):
        a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
        tol = 2 * ytol                                            # (two results, each held to ytol, against each other)
        np.testing.assert_allclose(a, b, rtol=tol, atol=tol * float(np.abs(b).max()))


@pytest.mark.parametrize("case", ("cplx_linear_f32", "real_linear_f32", "cplx_conv_nchw_f32", "real_conv_nchw_f32",
                                  "cplx_conv_cl_bf16", "real_linear_bf16"))
def test_degenerate_masks(case):
    from cplxmodule_amd.nn import masked
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, tol = CASES[case]
    layer, xs, cl = _make(case)
    ws, bs = _params(layer, cplx)
    # all zero: the broadcast bias, zero gradients except the bias gradient, no error
    layer.mask = torch.zeros_like(layer.mask)
    masked.compact_(layer, max_live=1.0)
    rep = masked.compaction(layer)[""]
    assert rep["rows"][:2] == (0, 0) and rep["cols"][:2] == (0, 0) and rep["active"] is True
    leaves, y = _forward(layer, xs, cl, cplx)
    g = [torch.randn_like(t) for t in y]
    sum((a * b).sum() for a, b in zip(y, g)).backward()
    for k, yk in enumerate(y):
        bias = bs[k].detach().to(yk.dtype)
        assert torch.equal(yk.detach(), bias.view(1, -1, *([1] * (yk.dim() - 2))).expand_as(yk))
        dims = [d for d in range(yk.dim()) if d != 1] if kind == "conv" else [0]
        want = g[k].float().sum(dims).cpu().numpy()
        np.testing.assert_allclose(bs[k].grad.cpu().numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    for t in leaves + ws:
        assert t.grad is not None and t.grad.shape == t.shape and (t.grad == 0).all()
    # all ones with the flag on: not active, the dense route's bits
    layer.mask = torch.ones_like(layer.mask)
    assert masked.compaction(layer)[""]["active"] is False
    y_on = _forward(layer, xs, cl, cplx)[1]
    masked.compact_(layer, enabled=False)
    y_off = _forward(layer, xs, cl, cplx)[1]
    assert all(torch.equal(a, b) for a, b in zip(y_on, y_off))


def test_all_zero_mask_circular_padding_not_square():
    """The all-zero mask launches no convolution, so the route works the output shape out itself: circular padding
    (2, 1) widens W by 2 and H by 1 (the reference hands `padding` to F.pad, which starts at the last dimension)."""
    from cplxmodule_amd import Cplx
    from cplxmodule_amd.nn import masked
    torch.manual_seed(14)
    layer = masked.CplxConv2dMasked(3, 4, 3, padding=(2, 1), padding_mode="circular").to(DEV)
    layer.mask = torch.zeros(4, 3, 3, 3)
    x = Cplx(torch.randn(2, 3, 7, 9, device=DEV), torch.randn(2, 3, 7, 9, device=DEV))
    off = layer(x)
    masked.compact_(layer, max_live=1.0)
    assert masked.compaction(layer)[""]["active"] is True
    on = layer(x)
    assert tuple(on.real.shape) == tuple(off.real.shape) == (2, 4, 6, 9)
    assert torch.equal(on.real, off.real) and torch.equal(on.imag, off.imag)


@pytest.mark.parametrize("case", ("cplx_linear_f32", "real_linear_bf16", "cplx_conv_nchw_f32_wide", "real_conv_cl_bf16",
                                  "cplx_conv_cl_bf16", "real_conv_nchw_f32"))
def test_flag_off_is_the_function_the_layer_calls_today(case):
    from cplxmodule_amd import Cplx, conv, cplx as cx, ops
    from cplxmodule_amd.nn import masked
    kind, cplx, dtype, xshape, args, kwargs, lr, lc, cl, tol = CASES[case]
    layer, xs, cl = _make(case)
    masked.compact_(layer, max_live=1.0)
    masked.compact_(layer, enabled=False)
    leaves, y = _forward(layer, xs, cl, cplx)
    x = [t.detach() for t in leaves]       # (gradient mode on: the convolutions pick their route by what needs a gradient)
    if kind == "linear" and cplx:
        w, b = layer.weight, layer.bias
        want = ops.CplxLinearFn.apply(x[0], x[1], w.real, w.imag, b.real, b.imag, 0, layer.mask)
    elif kind == "linear":
        want = (ops.RealLinearFn.apply(x[0], layer.weight, layer.bias, layer.mask),)
    elif cplx:
        r = cx.conv2d(Cplx(*x), layer.weight_masked, layer.bias, layer.stride, layer.padding, layer.dilation, layer.groups,
                      layer.padding_mode)
        want = (r.real, r.imag)
    else:
        want = (conv.RealConv2dFn.apply(x[0], layer.weight_masked, layer.bias, layer.stride, layer.padding,
                                        layer.dilation, layer.groups),)
    assert all(torch.equal(a, b) for a, b in zip(y, want))


def test_mask_change_rebuilds_the_plan():
    from cplxmodule_amd.nn import masked
    layer, xs, cl = _make("cplx_linear_f32")
    masked.compact_(layer, max_live=1.0)

    def both():
        masked.compact_(layer, max_live=1.0)
        on = _forward(layer, xs, cl, True)[1]
        masked.compact_(layer, enabled=False)
        off = _forward(layer, xs, cl, True)[1]
        masked.compact_(layer, max_live=1.0)
        for a, b in zip(on, off):
            a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
            np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-5 * float(np.abs(b).max()))   # (each held to 1e-5)

    both()
    assert masked.compaction(layer)[""] == dict(rows=(20, 64, 70), cols=(50, 64, 130), active=True)
    plan0 = layer._compact_plan
    layer.mask = _structured_mask((70, 130), 5, 70, 11)                 # a new mask by attribute
    assert masked.compaction(layer)[""] == dict(rows=(5, 64, 70), cols=(70, 128, 130), active=True)
    assert layer._compact_plan is not plan0
    both()
    plan1 = layer._compact_plan
    with torch.no_grad():                                               # an edit in place
        dead_col = int(torch.nonzero(layer.mask.ne(0).any(0))[0])
        layer.mask[:, dead_col] = 0
    both()
    assert layer._compact_plan is not plan1
    assert masked.compaction(layer)[""]["cols"] == (69, 128, 130)
    layer.mask = None
    assert masked.compaction(layer)[""] is None
    with pytest.raises(RuntimeError, match="no sparsity mask"):
        _forward(layer, xs, cl, True)


def test_second_derivative_through_compacted_linear():
    """A gradient penalty through a compacted CplxLinearMasked: grad(create_graph=True), then backward, against float64
    autograd (bound of tests/test_gpu_r06.py test_cplx_linear_double_backward: atol 2e-5 max|ref|)."""
    from cplxmodule_amd import Cplx
    from cplxmodule_amd.nn import masked
    torch.manual_seed(5)
    B, I, O = 64, 130, 96
    layer = masked.CplxLinearMasked(I, O).to(DEV)
    with torch.no_grad():
        layer.bias.real.normal_()
        layer.bias.imag.normal_()
    mask = _structured_mask((O, I), 40, 60, 6)
    layer.mask = mask
    masked.compact_(layer, max_live=1.0)
    assert masked.compaction(layer)[""]["active"] is True
    xs = [torch.randn(B, I), torch.randn(B, I)]

    def run(dev):
        dt = torch.float32 if dev == DEV else torch.float64
        x = [t.to(dev, dt).requires_grad_(True) for t in xs]
        if dev == DEV:
            p = [layer.weight.real, layer.weight.imag, layer.bias.real, layer.bias.imag]
            y = layer(Cplx(*x))
            yr, yi = y.real, y.imag
        else:
            p = [t.detach().double().cpu().requires_grad_(True) for t in
                 (layer.weight.real, layer.weight.imag, layer.bias.real, layer.bias.imag)]
            m = mask.double()
            yr = F.linear(x[0], p[0] * m, p[2]) - F.linear(x[1], p[1] * m)
            yi = F.linear(x[0], p[1] * m, p[3]) + F.linear(x[1], p[0] * m)
        loss = (yr ** 2).sum() + (yr * yi).sum()
        g = torch.autograd.grad(loss, x + p[:2], create_graph=True)
        pen = sum((t ** 2).sum() for t in g)
        second = torch.autograd.grad(pen, x + p)
        return [t.detach().double().cpu().numpy() for t in (*g, *second)]

    for a, b in zip(run(DEV), run("cpu")):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * float(np.abs(b).max()))


def _warm_and_capture(step, modules):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for m in modules:
        m.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    return g, out


def test_graph_replay_matches_eager_and_stale_plan_raises():
    from cplxmodule_amd import Cplx
    from cplxmodule_amd._lib import CplxAmdError
    from cplxmodule_amd.nn import masked
    torch.manual_seed(7)
    layer = masked.CplxLinearMasked(256, 192).to(DEV)
    layer.mask = _structured_mask((192, 256), 70, 100, 8)
    masked.compact_(layer, max_live=1.0)
    x = Cplx(torch.randn(32, 256, device=DEV), torch.randn(32, 256, device=DEV))

    def step():
        y = layer(x)
        ((y.real ** 2).sum() + (y.real * y.imag).sum()).backward()
        return y

    g, y = _warm_and_capture(step, [layer])
    g.replay()
    torch.cuda.synchronize()
    got = [y.real.clone(), y.imag.clone()] + [p.grad.clone() for p in layer.parameters()]
    layer.zero_grad(set_to_none=True)
    ye = step()
    want = [ye.real, ye.imag] + [p.grad for p in layer.parameters()]
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got, want))
    # a plan that is stale when the capture starts cannot be rebuilt inside it
    layer.mask = _structured_mask((192, 256), 10, 20, 9)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(CplxAmdError, match="eagerly"):
        with torch.cuda.graph(graph):
            warm = x.real * 1.0                  # noqa: F841  (the capture is not empty)
            layer(x)
    torch.cuda.synchronize()
    layer(x)                                     # eagerly: fine, and the plan is fresh again
    assert masked.compaction(layer)[""]["rows"] == (10, 64, 192)


def test_short_trajectory_route_on_against_off():
    """Five SGD steps of a two-layer CplxLinearMasked net, float32: the parameters of the two routes agree to the
    per-step trajectory bound (README: 1e-5, norm-wise) and masked entries never move."""
    import copy
    from cplxmodule_amd import Cplx
    from cplxmodule_amd.nn import masked
    torch.manual_seed(9)
    net = torch.nn.Sequential(masked.CplxLinearMasked(130, 96), masked.CplxLinearMasked(96, 70)).to(DEV)
    net[0].mask = _structured_mask((96, 130), 40, 60, 12)
    net[1].mask = _structured_mask((70, 96), 30, 40, 13)
    nets = {True: net, False: copy.deepcopy(net)}
    init = {k: v.clone() for k, v in net.state_dict().items()}
    masked.compact_(nets[True], max_live=1.0)
    assert all(v["active"] for v in masked.compaction(nets[True]).values())
    assert not any(v["active"] for v in masked.compaction(nets[False]).values())
    x = Cplx(torch.randn(48, 130, device=DEV), torch.randn(48, 130, device=DEV))
    t = Cplx(torch.randn(48, 70, device=DEV), torch.randn(48, 70, device=DEV))
    opts = {k: torch.optim.SGD(n.parameters(), lr=0.05) for k, n in nets.items()}
    for step in range(5):
        for k, n in nets.items():
            opts[k].zero_grad(set_to_none=True)
            h = n[0](x)
            y = n[1](Cplx(torch.relu(h.real), torch.relu(h.imag)))
            (((y.real - t.real) ** 2).mean() + ((y.imag - t.imag) ** 2).mean()).backward()
            opts[k].step()
        for (name, a), b in zip(nets[True].state_dict().items(), nets[False].state_dict().values()):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5 * float(np.abs(b).max()), err_msg=f"step {step} {name}")
    for n in nets.values():
        for i in (0, 1):
            dead = n[i].mask == 0
            for part in ("real", "imag"):
                assert torch.equal(getattr(n[i].weight, part).detach()[dead], init[f"{i}.weight.{part}"][dead])
