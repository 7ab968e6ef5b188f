"""cplx.linear_recurrence / cumsum / cumprod without a GPU: the argument errors, cplxamd_scan_plan (csrc/scan.hip) and the
adjoint identities cplxmodule_amd/scan.py builds its backward from, on the plain loop of tests/scan_cases.py."""
import itertools

import pytest
import torch

from scan_cases import reference

from cplxmodule_amd import Cplx, cplx, scan
from cplxmodule_amd._lib import CplxAmdError

FLAGS = list(itertools.product([False, True], repeat=3))


def test_argument_errors_need_no_device():
    x, c = torch.zeros(3, 8), torch.zeros(3, 8, dtype=torch.complex64)
    for bad in (lambda: cplx.linear_recurrence(x, x), lambda: cplx.cumsum(Cplx(x, x)), lambda: cplx.cumprod(x),   # CPU tensors
                lambda: cplx.linear_recurrence(x.half(), x.half()), lambda: cplx.linear_recurrence(c, x),
                lambda: cplx.cumsum(c), lambda: cplx.linear_recurrence(x, x.double()),
                lambda: cplx.linear_recurrence(x, x, h0=torch.zeros(3, dtype=torch.bfloat16))):
        with pytest.raises(CplxAmdError):
            bad()
    for bad in (lambda: cplx.linear_recurrence(torch.zeros(()), x), lambda: cplx.cumsum(torch.zeros(())),
                lambda: cplx.linear_recurrence(x, x, h0=torch.zeros(4)), lambda: cplx.linear_recurrence(x, x, h0=x),
                lambda: cplx.linear_recurrence(torch.zeros(3, 5), x)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
@pytest.mark.parametrize("cx", [True, False])
def test_plan(dtype, cx):
    word, nc = (8 if dtype == torch.float64 else 4), (4 if cx else 2)
    row, col = scan.plan(5003, 300, None, dtype, cx), scan.plan(5003, 100, 130, dtype, cx)
    L = row["chunk"]
    assert L == (8 if dtype == torch.float64 else 16)
    assert (row["path"], row["tile"], row["segments"], row["grid"], row["ws_bytes"]) == ("row", 256 * L, 1, 300, 0)
    # a [B, T, D] tensor through a transpose: lanes along D, a unit is 64 channels of a row
    assert (col["path"], col["tile"], col["units"], col["segments"]) == ("column", 4 * L, 100 * 3, 1)
    assert scan.plan(5003, 300, 1, dtype, cx)["path"] == "row"
    assert row["window"] == row["tile"] and scan.plan(7, 300, None, dtype, cx)["window"] == 7
    # few rows of at least four tiles: segments of whole tiles, up to 1024 workgroups, one map per unit and segment
    for rows, T, ch in ((1, 1 << 22, None), (3, 4 * row["tile"], None), (255, 9 * row["tile"] + 1, None), (8, 4096, 1024)):
        p = scan.plan(T, rows, ch, dtype, cx)
        assert p["path"] == "split" and p["seg_len"] % p["tile"] == 0 and p["seg_len"] >= 2 * p["tile"]
        assert p["grid"] == p["units"] * p["segments"] <= 1024 + p["units"] and p["window"] == p["seg_len"]
        assert (p["segments"] - 1) * p["seg_len"] < T <= p["segments"] * p["seg_len"]
        assert p["ws_bytes"] == p["units"] * (p["segments"] - 1) * nc * word * (64 if ch else 1)
    assert scan.plan(3 * row["tile"], 3, None, dtype, cx)["path"] == "row"              # fewer than four tiles
    assert scan.plan(1 << 22, 256, None, dtype, cx)["path"] == "row"                    # the rows fill the chip
    forced = scan.plan(5003, 6, None, dtype, cx, force_segments=7)
    assert (forced["segments"], forced["seg_len"]) == (7, 715) and scan.plan(3, 1, force_segments=7)["segments"] == 3
    for p in (row, col, forced, scan.plan(1 << 22, 1, None, dtype, cx), scan.plan(4096, 8, 1024, dtype, cx)):
        assert p["lds_bytes"] <= 76 << 10 and p["threads"] == 256


def _inner(u, v):
    return (u.conj() * v).sum().real


@pytest.mark.parametrize("reverse,conj,lag", FLAGS)
def test_the_adjoint_is_the_primitive_with_every_flag_flipped(reverse, conj, lag):
    g = torch.Generator().manual_seed(1)
    a, x, up = (torch.randn(3, 41, dtype=torch.complex128, generator=g) for _ in range(3))
    fwd = reference(a, x, None, reverse, conj, lag)
    adj = reference(a, up, None, not reverse, not conj, not lag)
    assert torch.allclose(_inner(up, fwd), _inner(adj, x), rtol=1e-12)


@pytest.mark.parametrize("reverse", [False, True])
def test_the_gradient_formulas_against_autograd(reverse):
    """dx = lambda, da[t] = lambda[t] conj(h[t - 1]) with h[-1] = h0, dh0 = conj(a[0]) lambda[0] (reverse: t + 1, a[T - 1])"""
    g = torch.Generator().manual_seed(2)
    pl = [torch.randn(3, 29, dtype=torch.float64, generator=g).requires_grad_() for _ in range(4)]
    pl += [torch.randn(3, dtype=torch.float64, generator=g).requires_grad_() for _ in range(2)]
    a, x, h0 = (torch.complex(pl[k], pl[k + 1]) for k in (0, 2, 4))
    up = torch.randn(3, 29, dtype=torch.complex128, generator=g)
    h = reference(a, x, h0, reverse)
    grads = torch.autograd.grad(_inner(up, h), pl)                  # d/dre + i d/dim of Re <up, h>
    da, dx, dh0 = (torch.complex(grads[k], grads[k + 1]) for k in (0, 2, 4))
    lam = reference(a, up, None, not reverse, True, True)
    first = h0.unsqueeze(-1)
    before = torch.cat([h[..., 1:], first], -1) if reverse else torch.cat([first, h[..., :-1]], -1)
    at = -1 if reverse else 0
    for got, want in ((lam, dx), (lam * before.conj(), da), (a[..., at].conj() * lam[..., at], dh0)):
        assert torch.allclose(got.detach(), want, rtol=1e-11, atol=1e-11)
