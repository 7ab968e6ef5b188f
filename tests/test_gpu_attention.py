"""cplx.scaled_dot_product_attention on the GPU (csrc/attention.hip): forward and gradient parity against float64 torch
on the CPU (computed from the planes as the kernel received them), the online softmax under scores of +-100, layouts read
in place, bit-identical reruns, hipGraph replay and nn.CplxMultiheadAttention.  The key tile is 32 (float32) and 64
(bfloat16): S = 31, 65, 130, 257 sit one short of / one past multiples of both.

BF16_GRAD_TOL: norm-wise error (max |d - ref| / max |ref|) against float64 of torch's own bf16
F.scaled_dot_product_attention backward on the concatenated planes (score="real", scale = 1 / sqrt(E)), largest value
over the gradient cases below, times 2 for the different summation order (scripts/attention_bf16_bound.py,
profiles/attention_bf16_bound.txt; the errors this file prints: profiles/attention_parity.txt)."""
import math

import pytest
import torch

from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx, nn

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5                  # README "Tolerances": rtol 1e-5 + atol 1e-5 max|ref|
BF16_GRAD_TOL = 1.0566e-2    # 2 x 5.2831e-3 (measured: see the docstring)
DTYPES = [torch.float32, torch.bfloat16]
FWD_SHAPES = [(1, 1, 1, 1), (33, 31, 8, 8), (64, 65, 40, 24), (129, 130, 64, 64), (32, 257, 128, 128)]


def reference(qr, qi, kr, ki, vr, vi, causal, scale, score):
    cr, ci = qr @ kr.mT + qi @ ki.mT, qi @ kr.mT - qr @ ki.mT
    s = scale * (cr if score == "real" else torch.sqrt(cr * cr + ci * ci))
    if causal:
        s = s + torch.full(s.shape[-2:], -math.inf, dtype=s.dtype).triu(1)
    p = torch.softmax(s, -1)
    return p @ vr, p @ vi


def planes(lead, L, S, E, Ev, dtype, seed=0):
    """(q_r, q_i, k_r, k_i, v_r, v_i) on the CPU, already rounded to dtype"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*lead, n, e, generator=g).to(dtype) for n, e in ((L, E), (L, E), (S, E), (S, E), (S, Ev), (S, Ev))]


def run(p, causal=False, scale=None, score="real", grad=False):
    d = [t.to(DEV).requires_grad_(grad) for t in p]
    return d, cplx.scaled_dot_product_attention(Cplx(d[0], d[1]), Cplx(d[2], d[3]), Cplx(d[4], d[5]), is_causal=causal,
                                                scale=scale, score=score)


def close_f32(got, ref, what):
    err = ((got.double().cpu() - ref).abs() / (F32_TOL * ref.abs() + F32_TOL * ref.abs().max())).max().item()
    print(what, "float32 error / bound", err)
    assert err <= 1.0, (what, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("score", ["real", "abs"])
@pytest.mark.parametrize("L,S,E,Ev", FWD_SHAPES)
def test_forward_parity(L, S, E, Ev, score, causal, dtype):
    p = planes((2, 3), L, S, E, Ev, dtype)
    _, o = run(p, causal, None, score)
    ref = reference(*[t.double() for t in p], causal, 1 / math.sqrt(E), score)
    assert o.real.dtype == dtype and o.real.shape == ref[0].shape
    for got, want, name in ((o.real, ref[0], "re"), (o.imag, ref[1], "im")):
        if dtype == torch.float32:
            close_f32(got, want, name)
        else:                    # |o - ref| <= 2^-7 max|v| per (batch, head): p rounds at 2^-9, sum p = 1; o rounds at 2^-9
            vmax = torch.maximum(p[4].abs().amax((-1, -2)), p[5].abs().amax((-1, -2))).double()[..., None, None]
            err = ((got.double().cpu() - want).abs() / (2.0 ** -7 * vmax)).max().item()
            print(name, "bf16 error / bound", err)
            assert err <= 1.0, err


@pytest.mark.parametrize("last", [True, False])
def test_online_softmax_under_large_scores(last):
    """scores span +-100 (a plain exp overflows); the row maximum in the last key tile (every tile rescales) or the first"""
    L, S, E = 32, 130, 8
    p = planes((2,), L, S, E, E, torch.float32, seed=1)
    ramp = torch.linspace(-50, 50, S) if last else torch.linspace(50, -50, S)
    p[0][..., 0], p[2][..., 0] = 2.0, ramp
    _, o = run(p, False, 1.0, "real")
    ref = reference(*[t.double() for t in p], False, 1.0, "real")
    assert torch.isfinite(o.real).all() and torch.isfinite(o.imag).all()
    close_f32(o.real, ref[0], "re")
    close_f32(o.imag, ref[1], "im")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layouts_are_read_in_place(dtype):
    B, H, L, S, E = 2, 3, 33, 31, 8
    bufs = [torch.randn(B, n, H, E, device=DEV).to(dtype) for n in (L, L, S, S, S, S)]
    views = [b.transpose(1, 2) for b in bufs]
    dense = [v.contiguous() for v in views]
    att = lambda t, **kw: cplx.scaled_dot_product_attention(Cplx(t[0], t[1]), Cplx(t[2], t[3]), Cplx(t[4], t[5]), **kw)  # noqa: E731
    o, od = att(views, is_causal=True), att(dense, is_causal=True)
    assert torch.equal(o.real, od.real) and torch.equal(o.imag, od.imag)
    assert o.real.transpose(1, 2).is_contiguous() and od.real.is_contiguous()   # the result's order follows the query's
    sliced = [b[:, :, ::2] for b in dense]                                         # every other query / key
    o, od = att(sliced, score="abs"), att([s.contiguous() for s in sliced], score="abs")
    assert torch.equal(o.real, od.real) and torch.equal(o.imag, od.imag) and o.real.is_contiguous()
    wide = [torch.randn(B, H, n, 2 * E, device=DEV).to(dtype)[..., ::2] for n in (L, L, S, S, S, S)]   # last-dim stride 2
    o, od = att(wide), att([w.contiguous() for w in wide])
    assert torch.equal(o.real, od.real) and torch.equal(o.imag, od.imag)
    assert att([t[:0] for t in dense]).real.shape == (0, H, L, E)                 # an empty batch: no launch


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("score", ["real", "abs"])
@pytest.mark.parametrize("L,S,E,Ev", FWD_SHAPES[1:4])
def test_gradients(L, S, E, Ev, score, causal, dtype):
    p = planes((2, 3), L, S, E, Ev, dtype)
    g = torch.Generator().manual_seed(7)
    up = [torch.randn(2, 3, L, Ev, generator=g).to(dtype) for _ in range(2)]     # a random complex upstream gradient
    d, o = run(p, causal, None, score, grad=True)
    got = torch.autograd.grad([o.real, o.imag], d, [u.to(DEV) for u in up])
    r = [t.double().requires_grad_(True) for t in p]
    ref = reference(*r, causal, 1 / math.sqrt(E), score)
    want = torch.autograd.grad(list(ref), r, [u.double() for u in up])
    for a, b, name in zip(got, want, ("dq_r", "dq_i", "dk_r", "dk_i", "dv_r", "dv_i")):
        assert a.dtype == dtype and a.shape == b.shape
        if dtype == torch.float32:
            close_f32(a, b, name)
        else:
            err = ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
            print(name, "bf16 norm-wise error", err, "bound", BF16_GRAD_TOL)
            assert err <= BF16_GRAD_TOL, (name, err)


@pytest.mark.parametrize("lead", ["heads", "five_runs"])
def test_gradients_through_strided_layouts(lead):
    """forward and backward read views in place (heads: [B, H, L, E] views of [B, L, H, E] leaves, a strided upstream
    gradient) or, beyond three batch runs, through one copy: the same bits as dense operands; a frozen k / v gets None"""
    L, S, E = 33, 31, 8
    if lead == "heads":
        leaves = [torch.randn(2, n, 3, E, device=DEV).requires_grad_(True) for n in (L, L, S, S, S, S)]
        views = [t.transpose(1, 2) for t in leaves]
        up = [torch.randn(2, 3, L, 2 * E, device=DEV)[..., ::2] for _ in range(2)]
    else:
        leaves = [torch.randn(4, 4, 4, 4, n, E, device=DEV).requires_grad_(True) for n in (L, L, S, S, S, S)]
        views = [t[::2, ::2, ::2, ::2] for t in leaves]
        up = [torch.randn(2, 2, 2, 2, L, E, device=DEV) for _ in range(2)]
    dense = [v.detach().contiguous().requires_grad_(True) for v in views]
    att = lambda t: cplx.scaled_dot_product_attention(Cplx(t[0], t[1]), Cplx(t[2], t[3]), Cplx(t[4], t[5]), is_causal=True, score="abs")  # noqa: E731
    o, od = att(views), att(dense)
    assert torch.equal(o.real, od.real) and torch.equal(o.imag, od.imag)
    got = torch.autograd.grad([o.real, o.imag], views, up, retain_graph=True)
    want = torch.autograd.grad([od.real, od.imag], dense, [u.contiguous() for u in up])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    only_q = torch.autograd.grad([o.real, o.imag], views[:2], up)        # k, v frozen: their kernel is not launched
    assert torch.equal(only_q[0], want[0]) and torch.equal(only_q[1], want[1])


def test_second_derivative_raises():
    d, o = run(planes((2,), 33, 31, 8, 8, torch.float32), grad=True)
    (dq,) = torch.autograd.grad(o.real.sum() + o.imag.sum(), d[:1], create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(dq.sum(), d[:1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_reruns_and_graph_replay(dtype):
    p = planes((2, 3), 129, 130, 64, 64, dtype)
    outs = []
    for _ in range(2):
        d, o = run(p, True, None, "abs", grad=True)
        outs.append([o.real, o.imag, *torch.autograd.grad([o.real, o.imag], d, [torch.ones_like(o.real)] * 2)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    d = [t.to(DEV) for t in p]
    att = lambda: cplx.scaled_dot_product_attention(Cplx(d[0], d[1]), Cplx(d[2], d[3]), Cplx(d[4], d[5]), is_causal=True, score="abs")  # noqa: E731
    att()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = att()
    for _ in range(3):
        o.real.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.real, outs[0][0]) and torch.equal(o.imag, outs[0][1])


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_module(cross):
    torch.manual_seed(3)
    m = nn.CplxMultiheadAttention(64, 4).to(DEV)
    B, L, S, H, dh = 2, 33, 31 if cross else 33, 4, 16
    x = Cplx(torch.randn(B, L, 64, device=DEV), torch.randn(B, L, 64, device=DEV))
    mem = Cplx(torch.randn(B, S, 64, device=DEV), torch.randn(B, S, 64, device=DEV)) if cross else x
    y = m(x, mem) if cross else m(x)
    (y.real.square().sum() + y.imag.square().sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in m.parameters())

    def lin(layer, zr, zi):          # the projection in float64 from the module's own weights
        wr, wi = layer.weight.real.detach().double().cpu(), layer.weight.imag.detach().double().cpu()
        br, bi = layer.bias.real.detach().double().cpu(), layer.bias.imag.detach().double().cpu()
        return zr @ wr.T - zi @ wi.T + br, zr @ wi.T + zi @ wr.T + bi
    heads = lambda t: t.view(B, -1, H, dh).transpose(1, 2)  # noqa: E731
    xr, xi, mr, mi = (t.double().cpu() for t in (x.real, x.imag, mem.real, mem.imag))
    q, k, v = lin(m.q_proj, xr, xi), lin(m.k_proj, mr, mi), lin(m.v_proj, mr, mi)
    o = reference(*(heads(t) for t in (*q, *k, *v)), False, 1 / math.sqrt(dh), "real")
    ref = lin(m.out_proj, *(t.transpose(1, 2).reshape(B, L, 64) for t in o))
    close_f32(y.real.detach(), ref[0], "re")
    close_f32(y.imag.detach(), ref[1], "im")
