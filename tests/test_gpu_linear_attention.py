"""cplx.linear_attention on the GPU (csrc/linattn.hip) against the plain float64 loop of
tests/test_linear_attention_host.py on the CPU, computed from the planes as the kernel received them (torch autograd
through the loop for the gradients).  The chunk C is read from linear_attention.plan.  Lead dims are (2, 3).

Bounds.  float32: the README's |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|, outputs and gradients.  bf16: norm-wise error
(max |d - ref| / max |ref|) against the float64 loop of `linear_attention.composed` on the same bf16 operands (torch's
own bf16 products), largest value over the parity cases and over the gradient cases below, times 2 for the different
summation order (scripts/linear_attention_bf16_bound.py, profiles/linear_attention_bf16_bound.txt; the errors this file
prints: profiles/linear_attention_parity.txt)."""
import functools
import math

import pytest
import torch

from gpu_util import DEV
from test_linear_attention_host import loop, z

from cplxmodule_amd import Cplx, cplx, linear_attention as la

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
BF16_FWD_TOL = 3.5866e-2      # 2 x 1.7933e-2 (measured: profiles/linear_attention_bf16_bound.txt, see the docstring)
BF16_GRAD_TOL = 1.9578e-2     # 2 x 9.7892e-3 (likewise)
C = la.plan(1, 8, 8)["chunk"]
SIZES = [1, C - 1, C, C + 1, 2 * C + 1]
HEADS = [(1, 1), (8, 24), (40, 72), (128, 128)]
LEAD = (2, 3)


@functools.lru_cache(maxsize=4)
def operands(T, E, Ev, dtype, lead=LEAD, decay="cplx"):
    """planes on the CPU, rounded to the dtype: q, k, v, lambda (float32; Re in [-0.3, -0.001], Im in [-pi, pi]; `shared`:
    one row per first lead dim), the state and the gradients of o and of the returned state"""
    g = torch.Generator().manual_seed(1000 * T + E)
    pair = lambda *s: tuple(torch.randn(*s, generator=g).to(dtype) for _ in range(2))          # noqa: E731
    q, k, v, go = pair(*lead, T, E), pair(*lead, T, E), pair(*lead, T, Ev), pair(*lead, T, Ev)
    ll = (lead[0], 1) if decay == "shared" else lead
    lam = (-0.001 - 0.299 * torch.rand(*ll, T, generator=g),
           None if decay == "real" else (2 * torch.rand(*ll, T, generator=g) - 1) * math.pi)
    return q, k, v, lam, pair(*lead, E, Ev), go, pair(*lead, E, Ev)


def dev(p, grad=False):
    """a plane pair on the device: a Cplx, or the real plane alone"""
    pr, pi = (None if t is None else t.to(DEV).requires_grad_(grad) for t in p)
    return pr if pi is None else Cplx(pr, pi)


def wide(p):
    return None if p is None else z(tuple(None if t is None else t.double() for t in p))


def check(got, ref, what, dtype, tol):
    """float32: elementwise against the README bound; bf16: norm-wise against `tol`; prints error / bound"""
    got, top = got.detach().double().cpu(), ref.abs().max()
    err = ((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * top)).max().item() if dtype == F32 else \
        ((got - ref).abs().max() / top).item() / tol
    print(what, str(dtype)[6:], "error / bound", err)
    assert got.shape == ref.shape and err <= 1.0, (what, err)


@pytest.mark.parametrize("E,Ev", HEADS)
@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_forward_parity(dtype, T, E, Ev):
    q, k, v, lam, state, _, _ = operands(T, E, Ev, dtype)
    for with_state, reverse in ((False, False), (True, False), (False, True), (True, True)):
        s = state if with_state else None
        ref = loop(wide(q), wide(k), wide(v), wide(lam), wide(s), E ** -0.5, reverse)
        got = cplx.linear_attention(dev(q), dev(k), dev(v), dev(lam), None if s is None else dev(s), return_state=True,
                                    reverse=reverse)
        for o, w, name in zip(got, ref, ("o", "state")):
            assert o.real.dtype == dtype
            for p, r in ((o.real, w.real), (o.imag, w.imag)):
                check(p, r, f"fwd {name} T={T} E={E} Ev={Ev} state={with_state} reverse={reverse}", dtype, BF16_FWD_TOL)


@functools.lru_cache(maxsize=2)
def exact_case(E, Ev, reverse):
    """integer planes in [-2, 2] at T = 2 C + 1 and the loop's o and last state: every partial sum stays below 2^24"""
    g = torch.Generator().manual_seed(E)
    pair = lambda *s: tuple(torch.randint(-2, 3, s, generator=g).float() for _ in range(2))   # noqa: E731
    q, k, v, s = pair(*LEAD, 2 * C + 1, E), pair(*LEAD, 2 * C + 1, E), pair(*LEAD, 2 * C + 1, Ev), pair(*LEAD, E, Ev)
    return q, k, v, s, loop(wide(q), wide(k), wide(v), None, wide(s), 1.0, reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("E,Ev", HEADS)
def test_exact_on_integers_whole_and_cut_in_two(E, Ev, reverse):
    q, k, v, s, ref = exact_case(E, Ev, reverse)
    T, cut = 2 * C + 1, C + 5
    run = lambda lo, hi, st, dtype: cplx.linear_attention(                                             # noqa: E731
        *(dev(tuple(t[..., lo:hi, :].to(dtype) for t in p)) for p in (q, k, v)), state=st, return_state=True, scale=1.0,
        reverse=reverse)
    for dtype in (BF16, F32):
        whole, last = run(0, T, dev(tuple(t.to(dtype) for t in s)), dtype)
        for got, w in ((whole, ref[0]), (last, ref[1])):
            # (bf16: the reference's one round-to-nearest-even)
            assert torch.equal(got.real.cpu(), w.real.float().to(dtype)) and torch.equal(got.imag.cpu(), w.imag.float().to(dtype))
    # float32: a row cut at a step that is no multiple of C, the state handed on, gives the same values
    (lo1, hi1), (lo2, hi2) = ((cut, T), (0, cut)) if reverse else ((0, cut), (cut, T))
    o1, mid = run(lo1, hi1, dev(s), F32)
    o2, end = run(lo2, hi2, mid, F32)
    both = [o2, o1] if reverse else [o1, o2]
    assert torch.equal(torch.cat([o.real for o in both], -2), whole.real) and torch.equal(torch.cat([o.imag for o in both], -2), whole.imag)
    assert torch.equal(end.real, last.real) and torch.equal(end.imag, last.imag)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layouts_reruns_and_empty_batch(dtype):
    T, H, E, Ev = C + 3, 3, 8, 24
    q, k, v, lam, state, _, _ = operands(T, E, Ev, dtype)
    heads = lambda p: Cplx(*(t.to(DEV).transpose(1, 2).contiguous().transpose(1, 2) for t in p))       # noqa: E731  [B, T, H, E] viewed as [B, H, T, E]
    want = cplx.linear_attention(dev(q), dev(k), dev(v), dev(lam), dev(state), return_state=True)
    got = cplx.linear_attention(heads(q), heads(k), heads(v), dev(lam), dev(state), return_state=True)
    assert got[0].real.stride() == (T * H * Ev, Ev, H * Ev, 1)          # the result is a free view of [B, T, H, Ev]
    odd = lambda p: Cplx(*(torch.stack([t, t], -1).to(DEV)[..., 0] for t in p))                        # noqa: E731  last-dim stride 2
    strided = cplx.linear_attention(odd(q), odd(k), odd(v), dev(lam), dev(state), return_state=True)
    again = cplx.linear_attention(dev(q), dev(k), dev(v), dev(lam), dev(state), return_state=True)
    for other in (got, strided, again):
        for a, b in zip(other, want):
            assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)
    none = cplx.linear_attention(*(Cplx(*(t.to(DEV)[:0] for t in p)) for p in (q, k, v)))
    assert none.shape == (0, H, T, Ev)


def test_graph_capture_and_replay():
    T, E, Ev = 2 * C + 1, 40, 72
    q, k, v, lam, state, _, _ = operands(T, E, Ev, F32)
    args = [dev(p) for p in (q, k, v, lam, state)]
    eager = cplx.linear_attention(*args, return_state=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        cplx.linear_attention(*args, return_state=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            o, s = cplx.linear_attention(*args, return_state=True)
    for _ in range(3):
        o.real.zero_(), o.imag.zero_(), s.real.zero_(), s.imag.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip((o, s), eager):
            assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)


@pytest.mark.parametrize("decay", ["cplx", "real", "shared"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("E,Ev", HEADS[1:3])
@pytest.mark.parametrize("T", [C + 1, 2 * C + 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gradients(dtype, T, E, Ev, reverse, decay):
    """dq, dk, dv, dlog_decay (complex, real, broadcast over a lead dim) and dstate of L = Re<g, o> + Re<gS, S_T>"""
    q, k, v, lam, state, go, gs = operands(T, E, Ev, dtype, decay=decay)
    leaves = [wide(p).requires_grad_() for p in (q, k, v, lam, state)]
    if decay == "real":
        leaves[3] = lam[0].double().requires_grad_()
    o, f = loop(*leaves, E ** -0.5, reverse)
    ref = torch.autograd.grad((wide(go).conj() * o).real.sum() + (wide(gs).conj() * f).real.sum(), leaves)
    args = [dev(p, True) for p in (q, k, v, lam, state)]
    o, f = cplx.linear_attention(*args, return_state=True, reverse=reverse)
    (gor, goi), (gsr, gsi) = ((t.to(DEV) for t in p) for p in (go, gs))
    ((o.real * gor).sum() + (o.imag * goi).sum() + (f.real * gsr).sum() + (f.imag * gsi).sum()).backward()
    for name, a, w in zip(("dq", "dk", "dv", "dlog_decay", "dstate"), args, ref):
        planes = ((a.grad, w),) if torch.is_tensor(a) else ((a.real.grad, w.real), (a.imag.grad, w.imag))
        for p, r in planes:
            check(p, r, f"{name} T={T} E={E} Ev={Ev} reverse={reverse} decay={decay}", dtype, BF16_GRAD_TOL)
