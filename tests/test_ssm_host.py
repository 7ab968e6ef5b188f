"""cplx.ssm_scan without a GPU: cplxamd_ssm_plan (csrc/ssm.hip), the argument errors, and the identities
cplxmodule_amd/ssm.py builds its backward from, on the plain loop of tests/ssm_cases.py in float64."""
import itertools

import pytest
import torch

from scan_cases import reference
from ssm_cases import loop

from cplxmodule_amd import Cplx, cplx, ssm
from cplxmodule_amd._lib import CplxAmdError


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cx,vary", itertools.product([True, False], repeat=2))
def test_plan(dtype, cx, vary):
    p = ssm.plan(5003, 16, 300, dtype, cx, vary)
    assert (p["chunk"], p["tile"], p["tiles"], p["threads"], p["grid"]) == (16, 4096, 2, 256, 300)
    assert p["group"] == (2 if cx and vary else 4) and p["window"] == 4096 and ssm.plan(7, 16)["window"] == 7
    # the carried states (double-buffered) and the waves' totals of one group (double-buffered), float32 words
    assert p["lds_bytes"] == 4 * (2 * 256 * (2 if cx else 1) + 2 * 4 * p["group"] * (4 if cx else 2))
    assert ssm.plan(0, 1, 5)["grid"] == 0 and ssm.plan(9, 256, 0)["grid"] == 0
    for bad in (lambda: ssm.plan(64, 0), lambda: ssm.plan(64, 257), lambda: ssm.plan(64, 4, dtype=torch.float64),
                lambda: ssm.plan(64, 4, dtype=torch.float16), lambda: ssm.plan(1 << 41, 4)):
        with pytest.raises(CplxAmdError):
            bad()


def test_argument_errors_need_no_device():
    x, s = torch.zeros(3, 8), torch.zeros(3, 4, 8)
    for bad in (lambda: cplx.ssm_scan(s, s, s, x),                                           # CPU tensors
                lambda: cplx.ssm_scan(s, s, s, x, dt=Cplx(x, x)), lambda: cplx.ssm_scan(s, s, s, x.double()),
                lambda: cplx.ssm_scan(s.half(), s.half(), s.half(), x.half()),
                lambda: cplx.ssm_scan(torch.zeros(3, 4, 8, dtype=torch.complex64), s, s, x),
                lambda: cplx.ssm_scan(torch.zeros(3, 0, 8), torch.zeros(3, 0, 8), torch.zeros(3, 0, 8), x),
                lambda: cplx.ssm_scan(torch.zeros(257, 1), torch.zeros(257, 1), torch.zeros(257, 1), x),
                lambda: cplx.ssm_scan(s, s, None, x)):
        with pytest.raises(CplxAmdError):
            bad()
    for bad in (lambda: cplx.ssm_scan(s, s, s[:, :3], x), lambda: cplx.ssm_scan(s, s, s[..., :5], x),
                lambda: cplx.ssm_scan(s, s, s, x, dt=x), lambda: cplx.ssm_scan(s[..., :1], s, s, x, dt=x[:, :5]),
                lambda: cplx.ssm_scan(s, s, s, x, h0=torch.zeros(3, 5)), lambda: cplx.ssm_scan(x[0], s, s, x)):
        with pytest.raises(ValueError):
            bad()


def _inner(u, v):
    return (u.conj() * v).sum().real


def _case(with_dt, seed=1, N=3, T=23):
    g = torch.Generator().manual_seed(seed)
    z = lambda *s: torch.randn(*s, dtype=torch.complex128, generator=g)          # noqa: E731
    a = z(2, N, 1) - 1 if with_dt else 0.9 * z(2, N, T)
    dt = 0.1 + torch.rand(2, T, dtype=torch.float64, generator=g) if with_dt else None
    return a, z(2, N, T), z(2, N, T), z(2, T), dt, z(2, N), z(2, T), z(2, N)


@pytest.mark.parametrize("with_dt", [False, True])
@pytest.mark.parametrize("reverse,conj,lag,dt_out", itertools.product([False, True], repeat=4))
def test_the_adjoint_is_the_primitive_with_b_and_c_swapped_and_every_flag_flipped(reverse, conj, lag, dt_out, with_dt):
    """(y, hT) is linear in (x, h0): <g, y> + <gf, hT> = <dx, x> + <dh0, h0> with dx the flipped run on (a, c, b, g, dt,
    gf) and dh0 = conj(A_first) times that run's final state.  (A run under lag does not scale its entering state: dh0 is
    then the flipped run's final state itself, and that run scales ITS entering state, so gf stays out.)"""
    a, b, c, x, dt, h0, g, gf = _case(with_dt)
    gf = torch.zeros_like(gf) if lag else gf
    y, hT, _ = loop(a, b, c, x, dt, h0, reverse, conj, lag, dt_out)
    dx, lam0, _ = loop(a, c, b, g, dt, gf, not reverse, not conj, not lag, not dt_out)
    A = (a if dt is None else torch.exp(dt.unsqueeze(-2) * a)).expand(2, 3, 23)[..., -1 if reverse else 0]
    dh0 = lam0 if lag else (A if conj else A.conj()) * lam0
    assert torch.allclose(_inner(g, y) + _inner(gf, hT), _inner(dx, x) + _inner(dh0, h0), rtol=1e-12)


@pytest.mark.parametrize("with_dt", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_the_parameter_gradient_formulas_against_autograd(reverse, with_dt):
    """ssm.parameter_gradients (da, db, dc, ddt) with the float64 loop as its scan primitive, against torch autograd
    through the loop; autograd's convention d/dre + i d/dim of Re <g, y> + Re <gf, hT>"""
    a, b, c, x, dt, h0, g, gf = _case(with_dt, 2)
    leaves = [t.clone().requires_grad_() for t in (a, b, c, x, h0)] + ([dt.clone().requires_grad_()] if with_dt else [])
    y, hT, _ = loop(*leaves[:4], leaves[5] if with_dt else None, leaves[4], reverse)
    want = torch.autograd.grad(_inner(g, y) + _inner(gf, hT), leaves)
    got = ssm.parameter_gradients(a, b, c, x, dt, h0, g, gf, reverse, (True,) * 4, recur=reference)
    got = [got[0].sum(-1, keepdim=True) if with_dt else got[0], got[1], got[2]] + ([got[3]] if with_dt else [])
    for u, v in zip(got, list(want[:3]) + list(want[5:])):
        assert torch.allclose(u, v, rtol=1e-10, atol=1e-10)
