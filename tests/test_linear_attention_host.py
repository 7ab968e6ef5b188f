"""cplx.linear_attention without a GPU: the backward's role swaps and decay gradient (linear_attention.gradients) run on
the plain float64 step-by-step loop below and are compared with torch autograd through that loop; the composed route
against the loop; the plan's seams; the argument errors.  tests/test_gpu_linear_attention.py uses the same loop as its
reference."""
import itertools

import pytest
import torch

from cplxmodule_amd import Cplx, cplx, linear_attention as la
from cplxmodule_amd._lib import CplxAmdError

F64 = torch.float64


def loop(q, k, v, lam, state, scale, reverse=False, conj=False, lag=False, scale_in=False):
    """complex128 q, k [*B, T, E], v [*B, T, Ev], lam [*B, T] or None, state [*B, E, Ev] or None -> (o, the last state):
    S <- exp(lam) S + k^H (x) v,  o = scale q S,  one step at a time, with the primitive's four flags"""
    T = q.shape[-2]
    S = torch.zeros(q.shape[:-2] + (q.shape[-1], v.shape[-1]), dtype=q.dtype) if state is None else state
    o, before = [None] * T, None
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        src = before if lag else t
        if lam is not None and src is not None:
            a = lam[..., src].conj() if conj else lam[..., src]
            S = torch.exp(a)[..., None, None] * S
        S = S + (scale if scale_in else 1.0) * k[..., t, :, None].conj() * v[..., t, None, :]
        o[t] = (1.0 if scale_in else scale) * (q[..., t, None, :] @ S).squeeze(-2)
        before = t
    return torch.stack(o, -2), S


def z(p):
    return None if p is None else torch.complex(p[0], torch.zeros_like(p[0]) if p[1] is None else p[1])


def loop_planes(q, k, v, lam, state, scale, reverse=False, conj=False, lag=False, scale_in=False, want_state=True):
    """`loop` with linear_attention.run's signature, on plane pairs"""
    o, f = loop(z(q), z(k), z(v), z(lam), z(state), scale, reverse, conj, lag, scale_in)
    return o.real, o.imag, f.real, f.imag


def case(seed, T=7, E=3, Ev=4, lead=(2,), decay="cplx", with_state=True):
    g = torch.Generator().manual_seed(seed)
    pair = lambda *s: (torch.randn(*s, generator=g, dtype=F64), torch.randn(*s, generator=g, dtype=F64))      # noqa: E731
    q, k, v, gr = pair(*lead, T, E), pair(*lead, T, E), pair(*lead, T, Ev), pair(*lead, T, Ev)
    lam = None
    if decay:
        lam = (-0.3 * torch.rand(*lead, T, generator=g, dtype=F64), None if decay == "real" else pair(*lead, T)[0])
    state, gf = (pair(*lead, E, Ev), pair(*lead, E, Ev)) if with_state else (None, None)
    return q, k, v, lam, state, gr, gf


@pytest.mark.parametrize("reverse,conj,lag,scale_in", list(itertools.product([False, True], repeat=4)))
@pytest.mark.parametrize("decay,with_state", [("cplx", True), ("real", False), (None, True), (None, False)])
def test_the_loop_is_the_quadratic_form_under_every_flag(reverse, conj, lag, scale_in, decay, with_state):
    """o[p] = scale sum_{s <= p} exp(M[p] - M[s]) (q[p] k[s]^H) v[s] + scale exp(M[p]) q[p] S0, M the prefix of mu in
    processing order: what the flags mean, written out independently of the recurrence"""
    q, k, v, lam, state, _, _ = (z(p) for p in case(1, decay=decay, with_state=with_state))
    o, f = loop(q, k, v, lam, state, 0.7, reverse, conj, lag, scale_in)
    T = q.shape[-2]
    order = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    mu = torch.zeros(q.shape[:-1], dtype=q.dtype)
    if lam is not None:
        for p, t in enumerate(order):
            src = order[p - 1] if lag else t
            if not (lag and p == 0):
                mu[..., p] = lam[..., src].conj() if conj else lam[..., src]
    M = mu.cumsum(-1)
    for p, t in enumerate(order):
        S = sum(torch.exp(M[..., p] - M[..., s])[..., None, None] * k[..., u, :, None].conj() * v[..., u, None, :]
                for s, u in enumerate(order[:p + 1]))
        S = S if state is None else S + torch.exp(M[..., p])[..., None, None] * state / (0.7 if scale_in else 1.0)
        torch.testing.assert_close(0.7 * (q[..., t, None, :] @ S).squeeze(-2), o[..., t, :], rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("decay,with_state", [("cplx", True), ("cplx", False), ("real", True), (None, True), (None, False)])
def test_role_swapped_calls_are_the_gradients(reverse, decay, with_state):
    """dq, dk, dv, dstate from three role-swapped calls of the loop and dlambda from the U / W formula, against torch
    autograd through the loop of L = Re<g, o> + Re<gS, S_T>; and the adjoint identity of each linear slot"""
    q, k, v, lam, state, g, gf = case(2, decay=decay, with_state=with_state)
    leaves = [z(p).requires_grad_() if p is not None else None for p in (q, k, v, lam, state)]
    if decay == "real":
        leaves[3] = lam[0].clone().requires_grad_()
    o, f = loop(*leaves, 0.6, reverse)
    L = (z(g).conj() * o).real.sum() + (0 if gf is None else (z(gf).conj() * f).real.sum())
    ref = torch.autograd.grad(L, [t for t in leaves if t is not None])
    final = (f.detach().real, f.detach().imag)
    got = la.gradients(loop_planes, q, k, v, lam, state, final, g, gf, 0.6, reverse, (True,) * 5)
    for name, d, w in zip("q k v lam state".split(), [d for d, t in zip(got, leaves) if t is not None], ref):
        d = d[0] if not w.is_complex() else z(d)
        torch.testing.assert_close(d, w, rtol=1e-10, atol=1e-10, msg=lambda m: f"d{name}: {m}")
    # o is linear in q: <g, o> = <dq, q>
    torch.testing.assert_close((z(g).conj() * o).sum().real, (z(got[0]).conj() * z(q)).sum().real, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("decay,with_state", [("cplx", True), ("real", False), (None, True)])
def test_composed_is_the_loop_and_float64_takes_it(reverse, decay, with_state):
    q, k, v, lam, state, _, _ = case(3, T=9, lead=(2, 3), decay=decay, with_state=with_state)
    ref = loop(z(q), z(k), z(v), z(lam), z(state), 3 ** -0.5, reverse)
    wrap = lambda p: None if p is None else (p[0] if p[1] is None else Cplx(*p))      # noqa: E731
    for fn in (la.composed, cplx.linear_attention):
        got = fn(Cplx(*q), Cplx(*k), Cplx(*v), wrap(lam), wrap(state), return_state=True, reverse=reverse)
        for o, w in zip(got, ref):
            torch.testing.assert_close(torch.complex(o.real, o.imag), w, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("E", [1, 32, 33, 128])
@pytest.mark.parametrize("Ev", [1, 32, 33, 128])
def test_plan_seams(E, Ev):
    p = la.plan(100, E, Ev, batch=6, dtype=torch.bfloat16)
    C, sl = p["chunk"], p["slice"]
    assert p["head_e"] == (32 if E <= 32 else 64 if E <= 64 else 128) and p["head_e"] >= E
    assert p["slices"] == -(-Ev // sl) and p["head_v"] == p["slices"] * sl and p["grid"] == 6 * p["slices"]
    assert p["chunks"] == -(-100 // C) and p["threads"] == 256 and 0 < p["lds_bytes"] <= 160 * 1024
    assert la.plan(0, E, Ev)["chunks"] == 0


@pytest.mark.parametrize("E,Ev", [(129, 8), (8, 129), (0, 8)])
def test_plan_rejects_heads_outside_1_to_128(E, Ev):
    with pytest.raises(CplxAmdError):
        la.plan(64, E, Ev)
    with pytest.raises(CplxAmdError):
        la.plan(64, 8, 8, dtype=torch.float64)


def test_argument_errors():
    c = lambda *s: Cplx(torch.zeros(*s), torch.zeros(*s))                             # noqa: E731
    q, k, v = c(2, 5, 4), c(2, 5, 4), c(2, 5, 6)
    for bad in ((q.real, k, v), (q, torch.zeros(2, 5, 4, dtype=torch.complex64), v), (q, k, None)):
        with pytest.raises(CplxAmdError):
            cplx.linear_attention(*bad)
    with pytest.raises(CplxAmdError):
        cplx.linear_attention(c(2, 5, 129), c(2, 5, 129), v)
    with pytest.raises(CplxAmdError):
        cplx.linear_attention(q, k, v, log_decay=torch.zeros(2, 5, dtype=torch.complex64))
    with pytest.raises(CplxAmdError):
        cplx.linear_attention(q, k, v, state=torch.zeros(2, 4, 6))
    with pytest.raises(CplxAmdError):
        cplx.linear_attention(q, k, Cplx(v.real.double(), v.imag.double()))
    with pytest.raises(CplxAmdError, match="cuda"):
        cplx.linear_attention(q, k, v)                    # float32 on the CPU: there is no CPU path
    for bad in (dict(key=c(2, 5, 3)), dict(value=c(2, 4, 6)), dict(key=c(3, 5, 4)), dict(log_decay=torch.zeros(2, 4)),
                dict(log_decay=torch.zeros(3, 5)), dict(state=c(2, 4, 5))):
        with pytest.raises(ValueError):
            cplx.linear_attention(**{**dict(query=q, key=k, value=v), **bad})
    o, s = cplx.linear_attention(c(2, 0, 4), c(2, 0, 4), c(2, 0, 6), return_state=True)          # T = 0: no launch
    assert o.shape == (2, 0, 6) and s.shape == (2, 4, 6) and not s.real.any()
