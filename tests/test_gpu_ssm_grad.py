"""The backward of cplx.ssm_scan on the parameter-gradient kernel (csrc/ssm_grad.hip) against torch autograd through the
plain float64 loop of tests/ssm_cases.py on the CPU.  L, the tile and the group are read from ssm.plan and ssm.grad_plan.
Rows are [2, 3]; the outputs are y and hT with upstream g and gf; every leaf requires grad.  Operands are drawn once,
rounded to bfloat16 (exact in float32 too: one reference serves both dtypes).  `wide`: b and c vary along time, else they
are [.., N, 1]; `shared`: b and c are [2, 1, N, .], expanded over the 3 by stride 0; a is [2, 3, N, T] per step and
[3, N, 1] else (shared by the batch).  The errors this file prints: profiles/ssm_parity.txt.

Bounds, those of tests/test_gpu_ssm.py, none widened: float32 |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|; bf16 dx and dh0
2^-8 max|ref|; bf16 da, db, dc, ddt 2^-7 max|ref|.  Where a float32 case passes half its bound the float32 loop on the CPU
(reference against reference) is printed beside it."""
import functools
import math

import pytest
import torch

from gpu_util import DEV
from ssm_cases import loop

from cplxmodule_amd import Cplx, cplx, ssm

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
MODES = ("const", "vary", "dt")
L, TILE = (ssm.plan(5003, 16)[k] for k in ("chunk", "tile"))
assert (L, TILE) == tuple(ssm.grad_plan(5003, 16)[k] for k in ("chunk", "tile"))


def group(cx, mode):
    return ssm.grad_plan(5003, 16, cplx=cx, time_varying=mode != "const")["group"]


def zc(t):
    return torch.complex(t[0], t[1]) if t.shape[0] == 2 else t[0]


def gradients(pl, up, reverse, kind):
    """autograd through the loop in `kind` of Re <g, y> + Re <gf, hT> -> the gradient of every plane of `pl`"""
    lv = {k: t.to(kind).requires_grad_() for k, t in pl.items()}
    y, hT, _ = loop(zc(lv["a"]), zc(lv["b"]), zc(lv["c"]), zc(lv["x"]), lv["dt"][0] if "dt" in lv else None,
                    zc(lv["h0"]) if "h0" in lv else None, reverse)
    planes = lambda o: (o.real, o.imag) if o.is_complex() else (o,)              # noqa: E731
    loss = sum((p * u.to(kind)).sum() for o, w in zip((y, hT), up) for p, u in zip(planes(o), w))
    return dict(zip(lv, torch.autograd.grad(loss, list(lv.values()))))


@functools.lru_cache(maxsize=None)
def case(T, N, cx, mode, wide, shared, reverse, with_h0, exact=False):
    """-> (planes by name, each [1 or 2, ...]; the upstream (g, gf); the float64 gradients).  Smooth: test_gpu_ssm.py's
    ranges (Re a in [-1, -0.01], Im a in [-pi, pi], dt in [1e-3, 1e-1]; without dt |a| in [0.8, 1)).  `exact`: a in
    {1, -1, i, -i} with about one zero in 50, everything else Gaussian integers in [-2, 2]."""
    g = torch.Generator().manual_seed(1000 * T + N)
    P, rows, tb = (2 if cx else 1), ((2, 1) if shared else (2, 3)), (T if wide else 1)
    u = lambda *s: torch.rand(*s, generator=g)                                   # noqa: E731
    n = ((lambda *s: torch.randint(-2, 3, (P, *s), generator=g).float()) if exact else
         (lambda *s: torch.randn(P, *s, generator=g)))
    if exact:
        k = torch.randint(0, 4 if cx else 2, (2, 3, N, T), generator=g)
        a = torch.stack([torch.tensor([1., -1, 0, 0])[k], torch.tensor([0., 0, 1, -1])[k]])[:P] * (u(*k.shape) >= 0.02)
    elif mode == "dt":
        a = torch.stack([-0.011 - 0.98 * u(3, N, 1), math.pi * (2 * u(3, N, 1) - 1)])[:P]
    else:
        s = (2, 3, N, T) if mode == "vary" else (3, N, 1)
        r, th = 0.8 + 0.19 * u(*s), 2 * math.pi * u(*s) if cx else math.pi * torch.randint(0, 2, s, generator=g)
        a = torch.stack([r * th.cos(), r * th.sin()])[:P]
    pl = {"a": a, "b": n(*rows, N, tb), "c": n(*rows, N, tb), "x": n(2, 3, T)}
    if with_h0:
        pl["h0"] = n(2, 3, N)
    if mode == "dt":
        pl["dt"] = 1.1e-3 + (1e-1 - 1.2e-3) * u(1, 2, 3, T)
    pl = {k: t.bfloat16().float() for k, t in pl.items()}
    up = (n(2, 3, T).bfloat16().float(), n(2, 3, N).bfloat16().float())
    return pl, up, gradients(pl, up, reverse, torch.float64)


def backward(pl, up, reverse, dtype):
    """cplx.ssm_scan and its backward on the device -> the gradient of every plane of `pl`"""
    lv = {k: t.to(dtype).to(DEV).requires_grad_() for k, t in pl.items()}

    def op(t, over=False):
        p = [q.expand(2, 3, *q.shape[2:]) if over else q for q in t]
        return Cplx(*p) if len(p) == 2 else p[0]
    y, hT = cplx.ssm_scan(op(lv["a"]), op(lv["b"], True), op(lv["c"], True), op(lv["x"]), dt=lv["dt"][0] if "dt" in lv else None,
                          h0=op(lv["h0"]) if "h0" in lv else None, return_state=True, reverse=reverse)
    planes = lambda o: [o.real, o.imag] if isinstance(o, Cplx) else [o]          # noqa: E731
    outs = torch.autograd.grad(planes(y) + planes(hT), list(lv.values()),
                               [w.to(dtype).to(DEV) for v in up for w in v[:len(planes(y))]])
    return dict(zip(lv, outs))


def close(got, ref, what, dtype, loose):
    top = ref.abs().max()
    bound = 1e-5 * ref.abs() + 1e-5 * top if dtype == F32 else 2.0 ** (-7 if loose else -8) * top
    err = ((got.detach().double().cpu() - ref).abs() / bound).max().item() if top > 0 else float((got != 0).any())
    print(what, str(dtype)[6:], "error / bound", err)
    return err


def check(key, dtype):
    pl, up, ref = case(*key)
    got = backward(pl, up, key[6], dtype)
    errs = {k: close(got[k], ref[k], f"{key} d{k}", dtype, k not in ("x", "h0")) for k in pl}
    if dtype == F32 and max(errs.values()) > 0.5:                # reference against reference
        f32 = gradients(pl, up, key[6], F32)
        for k in pl:
            close(f32[k], ref[k], f"{key} d{k}: the float32 loop against the float64 loop", F32, False)
    assert all(got[k].shape == pl[k].shape and e <= 1.0 for k, e in errs.items()), errs


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cx", [True, False])
def test_small_seams(cx, mode, dtype):
    G = group(cx, mode)
    for i, (T, N) in enumerate((T, N) for T in (1, L - 1, L + 1) for N in sorted({1, G, G + 1, 17})):
        # (the other axes take turns: wide, shared, reverse, with h0)
        check((T, N, cx, mode, i % 2 == 0, i % 3 == 0, i % 4 < 2, i % 5 < 3), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cx", [True, False])
def test_one_tile_seam(cx, mode, reverse, dtype):
    # one value per state in b and c with the constant coefficient (every gradient summed on chip), chunks otherwise
    check((TILE + 1, 5, cx, mode, mode != "const", mode != "vary", reverse, True), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_two_tiles(mode, reverse, dtype):
    """the prologue, the workspace and the reversed walk over the tiles"""
    check((2 * TILE + 5, 5, True, mode, mode != "dt", mode == "dt", reverse, not reverse), dtype)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", [L + 1, TILE + 1])
def test_exact(T, reverse):
    """integer operands, everything varying along time: nothing is reduced over time and float32 is exact"""
    N = group(True, "vary") + 1
    pl, up, ref = case(T, N, True, "vary", True, False, reverse, True, True)
    # every partial sum stays below 2^24: h and lambda whatever the order of composition, and their products
    a, b, c, x, h0 = (zc(pl[k].double()) for k in ("a", "b", "c", "x", "h0"))
    g, gf = zc(up[0].double()), zc(up[1].double())
    h = loop(a, b, c, x, None, h0, reverse)[2]
    lam = loop(a, c, b, g, None, gf, not reverse, True, True)[2]
    assert (b.abs() * x.abs().unsqueeze(-2)).sum(-1).max() + h0.abs().max() < 2 ** 24
    assert (c.abs() * g.abs().unsqueeze(-2)).sum(-1).max() + gf.abs().max() < 2 ** 24
    assert 2 * h.abs().max() * lam.abs().max() < 2 ** 24 and 2 * (b.abs() * lam.abs()).sum(-2).max() < 2 ** 24
    got = backward(pl, up, reverse, F32)
    for k in ("a", "b", "c", "x"):
        assert torch.equal(got[k].double().cpu(), ref[k]), k


@pytest.mark.parametrize("kind,planes", [("s4d", 1), ("mamba", 5)])
def test_memory_of_the_backward(kind, planes):
    """S4D-like (a, b, c [D, N, 1]): nothing of size B D N T is allocated.  Mamba-like (b, c [B, 1, N, T] expanded, dt):
    the per-row db and dc, two planes each, and one plane of slack for everything small."""
    B, D, N, T = 2, 8, 16, TILE + 1
    r = lambda *s: torch.randn(*s, device=DEV).requires_grad_()                  # noqa: E731
    wide = lambda t: t.expand(B, D, N, T)                                        # noqa: E731
    if kind == "s4d":
        th = 6.28 * torch.rand(D, N, 1, device=DEV)
        a, dt = Cplx((0.9 * th.cos()).requires_grad_(), (0.9 * th.sin()).requires_grad_()), None
        b, c = Cplx(r(D, N, 1), r(D, N, 1)), Cplx(r(D, N, 1), r(D, N, 1))
    else:
        a = Cplx((-0.01 - torch.rand(D, N, 1, device=DEV)).requires_grad_(), r(D, N, 1))
        b, c = Cplx(wide(r(B, 1, N, T)), wide(r(B, 1, N, T))), Cplx(wide(r(B, 1, N, T)), wide(r(B, 1, N, T)))
        dt = (1e-3 + 0.1 * torch.rand(B, D, T, device=DEV)).requires_grad_()
    y = cplx.ssm_scan(a, b, c, Cplx(r(B, D, T), r(B, D, T)), dt=dt)
    loss = y.real.square().sum() + y.imag.square().sum()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss.backward()
    peak = torch.cuda.max_memory_allocated() - before
    print(kind, "peak of the backward in float32 planes of B D N T:", peak / (B * D * N * T * 4))
    assert peak < planes * B * D * N * T * 4
