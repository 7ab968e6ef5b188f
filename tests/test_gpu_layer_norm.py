"""cplx.layer_norm and nn.CplxLayerNorm on the GPU (csrc/layer_norm.hip): forward and gradient parity against the
formulas in float64 torch on the CPU (computed from the planes as the kernel received them, torch autograd for the
gradients) on both sides of every plan seam, rows with a large offset, persistent workgroups that loop, layouts read in
place, bit-identical reruns, hipGraph replay and the module.  The errors this file prints: profiles/layer_norm_parity.txt.

Bounds (README "Tolerances"): float32 |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|; bf16 results (out, dx)
|got - ref| <= 2^-8 max|ref| (one rounding at 2^-9, doubled for the float32 arithmetic before it); dW and dB are float32
sums and take the float32 bound for both dtypes."""
import pytest
import torch

from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx, layer_norm, nn

pytestmark = pytest.mark.gpu

EPS = 1e-5
KINDS = ["whiten", "modulus"]
DTYPES = [torch.float32, torch.bfloat16]
_P = layer_norm.plan(10, 8)
SEAMS = sorted({_P["seam_wave"], _P["seam_block"], _P["bwd_seam_block"]})        # read from the plan, not written here
SIZES = sorted({8, 33, 255, 512, 513, 1030} | {s + k for s in SEAMS for k in (0, 1)})


def reference(xr, xi, w, b, kind, eps=EPS):
    cr, ci = xr - xr.mean(-1, keepdim=True), xi - xi.mean(-1, keepdim=True)
    if kind == "modulus":
        v = (cr * cr + ci * ci).mean(-1, keepdim=True) + eps
        yr, yi = cr / v.sqrt(), ci / v.sqrt()
    else:
        a, d = (cr * cr).mean(-1, keepdim=True) + eps, (ci * ci).mean(-1, keepdim=True) + eps
        bb = (cr * ci).mean(-1, keepdim=True)
        s = (a * d - bb * bb).sqrt()
        t = s * (a + d + 2 * s).sqrt()
        p, q, r = (d + s) / t, -bb / t, (a + s) / t
        yr, yi = p * cr + q * ci, q * cr + r * ci
    if w is None:
        return yr, yi
    return w[0, 0] * yr + w[0, 1] * yi + b[0], w[1, 0] * yr + w[1, 1] * yi + b[1]


def planes(lead, N, dtype, seed=0, offset=None):
    g = torch.Generator().manual_seed(seed)
    re, im = torch.randn(*lead, N, generator=g), torch.randn(*lead, N, generator=g)
    if offset is None:
        re = re * 2 + 0.5
        im = 0.5 * im + 0.7 * re                      # correlated planes: b != 0 exercises q
    else:
        re, im = re + offset, im - offset
    w, b = torch.randn(2, 2, N, generator=g), torch.randn(2, N, generator=g)
    up = [torch.randn(*lead, N, generator=g).to(dtype) for _ in range(2)]
    return re.to(dtype), im.to(dtype), w, b, up


def close(got, ref, what, dtype=torch.float32):
    bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().max() if dtype == torch.float32 else 2.0 ** -8 * ref.abs().max()
    err = ((got.double().cpu() - ref).abs() / bound).max().item() if ref.numel() else 0.0
    print(what, str(dtype)[6:], "error / bound", err)
    assert got.shape == ref.shape and err <= 1.0, (what, err)


def check(kind, dtype, affine, lead, N, seed=0, offset=None):
    """forward, dx_r, dx_i, dW and dB of one case against the float64 reference"""
    re, im, w, b, up = planes(lead, N, dtype, seed, offset)
    leaves = [re, im] + ([w, b] if affine else [])
    dev = [t.to(DEV).requires_grad_(True) for t in leaves]
    out = cplx.layer_norm(Cplx(dev[0], dev[1]), N, *dev[2:], eps=EPS, kind=kind)
    got = torch.autograd.grad([out.real, out.imag], dev, [u.to(DEV) for u in up])
    ref_leaves = [t.double().requires_grad_(True) for t in leaves]
    ref = reference(*ref_leaves, *([] if affine else [None, None]), kind)
    want = torch.autograd.grad(list(ref), ref_leaves, [u.double() for u in up])
    assert out.real.dtype == dtype and got[0].dtype == dtype
    tag = f"{kind} N={N} affine={int(affine)}"
    close(out.real, ref[0].detach(), tag + " out_r", dtype)
    close(out.imag, ref[1].detach(), tag + " out_i", dtype)
    for a, r, name in zip(got, want, ("dx_r", "dx_i", "dW", "dB")):
        close(a, r, f"{tag} {name}", dtype if name.startswith("dx") else torch.float32)
    return out, got


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(kind, dtype, affine, N):
    check(kind, dtype, affine, (2, 5), N)


@pytest.mark.parametrize("N", [2, 3, 7])
def test_short_rows_modulus(N):
    """(whiten is ill-conditioned for 2 <= N < 8: the sample covariance is nearly singular)"""
    check("modulus", torch.float32, True, (2, 5), N)


@pytest.mark.parametrize("kind", KINDS)
def test_one_feature(kind):
    """N = 1: c = 0, so the result is the bias exactly and dx is exactly 0"""
    re, im, w, b, up = planes((7,), 1, torch.float32)
    dev = [t.to(DEV).requires_grad_(True) for t in (re, im, w, b)]
    out = cplx.layer_norm(Cplx(dev[0], dev[1]), 1, dev[2], dev[3], kind=kind)
    assert torch.equal(out.real, dev[3][0].expand(7, 1)) and torch.equal(out.imag, dev[3][1].expand(7, 1))
    dx = torch.autograd.grad([out.real, out.imag], dev[:2], [u.to(DEV) for u in up])
    assert not dx[0].any() and not dx[1].any()
    plain = cplx.layer_norm(Cplx(dev[0], dev[1]), 1, kind=kind)
    assert not plain.real.any() and not plain.imag.any()


@pytest.mark.parametrize("N", [33, 1025])
@pytest.mark.parametrize("kind", KINDS)
def test_offset(kind, N):
    """planes at +-64 with unit spread: E[x^2] - m^2 loses 12 bits here, centred moments do not"""
    check(kind, torch.float32, True, (2, 5), N, seed=1, offset=64.0)


@pytest.mark.parametrize("kind", KINDS)
def test_persistent_workgroups_loop(kind):
    """2 x grid x rows-per-workgroup + 3 rows at N = 8: every backward workgroup walks rows and the tail is uneven"""
    p = layer_norm.plan(1 << 40, 8, kind)
    check(kind, torch.float32, True, (2 * p["bwd_grid"] * p["bwd_rows_per_wg"] + 3,), 8, seed=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layouts_reruns_and_shapes(dtype):
    B, L, H, d = 2, 5, 3, 40
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(2, 2, d, generator=g).to(DEV), torch.randn(2, d, generator=g).to(DEV)
    bufs = [torch.randn(B, L, H, d, generator=g).to(dtype).to(DEV) for _ in range(4)]

    def run(xr, xi, ur, ui, shape=d, w=w, b=b):
        xr, xi = xr.detach().requires_grad_(True), xi.detach().requires_grad_(True)
        wl, bl = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
        o = cplx.layer_norm(Cplx(xr, xi), shape, wl, bl)
        return [o.real, o.imag, *torch.autograd.grad([o.real, o.imag], [xr, xi, wl, bl], [ur, ui])]

    heads = [t.transpose(1, 2) for t in bufs]                     # [B, H, L, d] views of [B, L, H, d]
    sliced = [t[:, ::2] for t in bufs]                            # every other row
    for views in (heads, sliced):
        got, want = run(*views), run(*[v.contiguous() for v in views])
        assert all(torch.equal(a, c) for a, c in zip(got[:4], want[:4]))           # per-row results: the same bits
        for a, c, name in zip(got[4:], want[4:], ("dW", "dB")):                    # sums over rows taken in memory order
            close(a, c.double().cpu(), "layout " + name)
    o = run(*heads)[0]
    assert o.transpose(1, 2).is_contiguous() and run(*sliced)[0].is_contiguous()   # the result's order follows the input's
    again = run(*heads)
    assert all(torch.equal(a, c) for a, c in zip(run(*heads), again))             # the same bits, forward and backward
    two = run(*bufs, shape=(H, d), w=w[:, :, None].expand(2, 2, H, d).contiguous(), b=b[:, None].expand(2, H, d).contiguous())
    flat = run(*[t.reshape(B, L, H * d) for t in bufs], shape=H * d, w=w.repeat(1, 1, H), b=b.repeat(1, H))
    assert all(torch.equal(a.reshape(c.shape), c) for a, c in zip(two, flat))
    empty = cplx.layer_norm(Cplx(bufs[0][:0], bufs[1][:0]), d, w, b)
    assert empty.real.shape == (0, L, H, d) and empty.imag.dtype == dtype


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay(kind):
    re, im, w, b, _ = planes((2, 5), 513, torch.float32, seed=4)
    re, im, w, b = (t.to(DEV) for t in (re, im, w, b))
    eager = cplx.layer_norm(Cplx(re, im), 513, w, b, kind=kind)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = cplx.layer_norm(Cplx(re, im), 513, w, b, kind=kind)
    for _ in range(3):
        o.real.zero_()
        o.imag.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.real, eager.real) and torch.equal(o.imag, eager.imag)


def test_module_trains_a_pre_norm_step():
    torch.manual_seed(5)
    norm, att = nn.CplxLayerNorm(64).to(DEV), nn.CplxMultiheadAttention(64, 4).to(DEV)
    other = nn.CplxLayerNorm(64).to(DEV)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn_like(norm.weight))
    other.load_state_dict(norm.state_dict())
    assert set(norm.state_dict()) == {"weight", "bias"} and torch.equal(other.weight, norm.weight)
    x = Cplx(torch.randn(2, 33, 64, device=DEV), torch.randn(2, 33, 64, device=DEV))
    opt = torch.optim.SGD([*norm.parameters(), *att.parameters()], lr=0.1)
    before = norm.weight.detach().clone()
    y = att(norm(x))
    y = Cplx(x.real + y.real, x.imag + y.imag)
    (y.real.square().mean() + y.imag.square().mean()).backward()
    for p in (norm.weight, norm.bias):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    opt.step()
    assert not torch.equal(norm.weight, before)
    ref = reference(x.real.double().cpu(), x.imag.double().cpu(), before.double().cpu(), torch.zeros(2, 64).double(), "whiten")
    got = other(x)
    close(got.real.detach(), ref[0], "module out_r")
    close(got.imag.detach(), ref[1], "module out_i")
