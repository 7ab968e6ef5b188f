"""cplx.pfb_analysis and pfb_synthesis on the GPU (csrc/pfb.hip) against plain float64 references on the CPU, computed from
the planes as the kernel received them (bf16 inputs are rounded first); torch autograd through the references for the
gradients.  The packing seam, the frames per tile and the staged / direct seam are read from pfb.plan.

Bounds: float32 norm-wise 1e-5 (fft_cases.tol); bf16 no entry outside 2^-8 |ref| + 1e-5 max|ref| (fft_cases.bf16_violations)."""
import functools

import pytest
import torch

from fft_cases import bf16_violations, c128, normwise, tol
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx, pfb

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def ref_analysis(x, h, M, hop):
    fr = x.unfold(-1, h.numel(), hop) * h
    return torch.fft.fft(fr.reshape(*fr.shape[:-1], h.numel() // M, M).sum(-2))


def ref_synthesis(y, g, hop, length):
    (F, M), K = y.shape[-2:], g.numel()
    out = torch.zeros(*y.shape[:-2], length, dtype=torch.complex128)
    for f in range(F):
        out[..., f * hop:f * hop + K] += g * torch.tile(M * torch.fft.ifft(y[..., f, :]), (K // M,))
    return out


def check(got, ref, dtype):
    if dtype == BF16:
        assert bf16_violations(got, ref)[0] == 0, bf16_violations(got, ref)
    else:
        assert normwise(got, ref) <= tol(dtype), normwise(got, ref)


@functools.lru_cache(maxsize=None)
def data(M, P, T, dtype, rows=2):
    """-> (x planes [2, rows, T] and taps [K] on the CPU, rounded to dtype, as float64)"""
    g = torch.Generator().manual_seed(M * 1000 + P)
    return torch.randn(2, rows, T, generator=g).to(dtype).double(), torch.randn(P * M, generator=g).to(dtype).double()


def dev(t, dtype):
    return t.to(dtype).to(DEV)


PACKED = max(M for M in (2 ** k for k in range(1, 13)) if pfb.plan(M, 1)["vectors_per_workgroup"] > 1)
SEAM_P = min(P for P in range(1, 65) if pfb.plan(4096, P)["plan"] == "direct")      # the smallest direct K at 4096 channels


def tile_plus_one(M, P, hop):
    """F = frames per tile + 1 at that very F (two rows)"""
    F = pfb.plan(M, P, hop)["vectors_per_workgroup"] + 1
    assert pfb.plan(M, P, hop, F, 2)["frames_per_tile"] == F - 1
    return F


# (M, P, hop, frames, samples behind the last frame): every leading radix of the engine (M = 2, 8, 16, 32), the packing
# seam, hop = M, M / 2, K, 1 and M / 2 + 1, F = 1, a remainder, F = tile + 1 with two hops, both sides of the staged seam
CASES = [(2, 1, 2, 1, 0), (8, 3, 4, 5, 3), (16, 8, 128, 3, 0), (32, 3, 1, 7, 0), (16, 3, 9, 6, 5),
         (PACKED, 1, PACKED // 2, 3, 1), (2 * PACKED, 3, 2 * PACKED, 2, 0),
         (8, 3, 5, tile_plus_one(8, 3, 5), 2), (64, 8, 32, tile_plus_one(64, 8, 32), 0),
         (4096, SEAM_P - 1, 4096, 2, 0), (4096, SEAM_P, 2049, 2, 7), (4096, 8, 4096, 1, 0)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M, P, hop, F, rem", CASES)
def test_analysis(M, P, hop, F, rem, dtype):
    x, h = data(M, P, (F - 1) * hop + P * M + rem, dtype)
    got = cplx.pfb_analysis(Cplx(dev(x[0], dtype), dev(x[1], dtype)), dev(h, dtype), M, hop)
    assert got.shape == (2, F, M) and got.real.is_contiguous() and got.dtype == dtype
    check(got, ref_analysis(torch.complex(x[0], x[1]), h, M, hop), dtype)


def test_one_tap_per_branch_is_a_framed_fft():
    x, _ = data(32, 1, 200, F32)
    xr, xi = dev(x[0], F32), dev(x[1], F32)
    got = cplx.pfb_analysis(Cplx(xr, xi), torch.ones(32, device=DEV), 32, 16)
    fft = cplx.fft(Cplx(xr.unfold(-1, 32, 16), xi.unfold(-1, 32, 16)))
    assert normwise(got, c128(fft.real, fft.imag)) <= tol(F32)


@pytest.mark.parametrize("M, P, hop", [(8, 3, 5), (2048, 2, 1024), (4096, SEAM_P, 4096)])
def test_real_input_is_a_null_imaginary_plane(M, P, hop):
    x, h = data(M, P, 3 * hop + P * M, F32)
    xr, h = dev(x[0], F32), dev(h, F32)
    a, b = cplx.pfb_analysis(xr, h, M, hop), cplx.pfb_analysis(Cplx(xr, torch.zeros_like(xr)), h, M, hop)
    assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)


def test_layouts_read_in_place():
    """a transposed batch view, a step slice and 1024 expanded rows (no balance cap: tiles of two passes) against their
    dense twins, bit for bit: the plan depends on the number of rows only"""
    M, P, hop = 64, 2, 64
    F = 2 * pfb.plan(M, P, hop, 10 ** 6, 1024)["vectors_per_workgroup"] + 1
    assert pfb.plan(M, P, hop, F, 1024)["frames_per_tile"] == F - 1
    x, h64 = data(M, P, 2 * ((F - 1) * hop + P * M), F32, 15)
    xr, xi, h = dev(x[0], F32), dev(x[1], F32), dev(h64, F32)
    views = [lambda t: t.reshape(3, 5, -1).transpose(0, 1)[..., ::2], lambda t: t[0, ::2].expand(1024, -1)]
    for view in views:
        got = cplx.pfb_analysis(Cplx(view(xr), view(xi)), h, M, hop)
        twin = cplx.pfb_analysis(Cplx(view(xr).contiguous(), view(xi).contiguous()), h, M, hop)
        assert torch.equal(got.real, twin.real) and torch.equal(got.imag, twin.imag)
    check(got[0], ref_analysis(torch.complex(x[0, 0, ::2], x[1, 0, ::2]), h64, M, hop), F32)
    y = cplx.pfb_analysis(Cplx(xr, xi), h, M, hop)                       # synthesis: a frames-minor view of the spectrum
    yt = Cplx(y.real.transpose(-1, -2).contiguous().transpose(-1, -2), y.imag.transpose(-1, -2).contiguous().transpose(-1, -2))
    a, b = cplx.pfb_synthesis(y, h, hop), cplx.pfb_synthesis(yt, h, hop)
    assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M, P, hop, F, extra", [(2, 1, 2, 1, 0), (8, 3, 5, 300, 9), (32, 3, 1, 7, 0), (16, 8, 128, 3, 0),
                                                 (PACKED, 2, PACKED // 2, 5, 3), (2 * PACKED, 3, 2 * PACKED, 2, 0)])
def test_synthesis(M, P, hop, F, extra, dtype):
    y, g = data(M, P, F * M, dtype)
    y = y.reshape(2, 2, F, M)
    least = (F - 1) * hop + P * M
    got = cplx.pfb_synthesis(Cplx(dev(y[0], dtype), dev(y[1], dtype)), dev(g, dtype), hop, least + extra if extra else None)
    assert got.shape == (2, least + extra) and got.dtype == dtype
    check(got, ref_synthesis(torch.complex(y[0], y[1]), g, hop, least + extra), dtype)
    assert not got.real[..., least:].any() and not got.imag[..., least:].any()


def grads(fn, planes, w, order):
    """the gradient of <w, fn(planes)> in the planes (order 1), or of the sum of squares of the gradient of
    sum(re^3 + re im^2) (order 2: through create_graph)"""
    planes = [p.clone().requires_grad_() for p in planes]
    out = fn(*planes)
    if order == 1:
        return torch.autograd.grad([out.real, out.imag], planes, w)
    first = torch.autograd.grad((out.real ** 3 + out.real * out.imag ** 2).sum(), planes, create_graph=True)
    return torch.autograd.grad(sum((f ** 2).sum() for f in first), planes)


@pytest.mark.parametrize("M, P, hop, F, real, dtype, order", [
    (8, 3, 5, 300, False, F32, 1), (8, 3, 5, 300, False, BF16, 1), (2 * PACKED, 2, PACKED, 3, False, F32, 1),
    (32, 3, 17, 9, True, F32, 1), (32, 3, 17, 9, True, BF16, 1), (4096, SEAM_P, 4096, 2, False, F32, 1),
    (16, 2, 8, 20, False, F32, 2), (16, 2, 8, 20, True, F32, 2)])
def test_gradients(M, P, hop, F, real, dtype, order):
    """dx of the analysis (a real x: the real plane only) and dy of the synthesis; T leaves samples behind the last frame"""
    T = (F - 1) * hop + P * M + 3
    scale = 0.125 if order == 2 else 1.0                                  # (a power of two: the planes stay in dtype)
    x, h = data(M, P, T, dtype)
    y, w = data(M, P + 2, F * M, dtype)[0].reshape(2, 2, F, M) * scale, data(M, P + 1, max(F * M, T), dtype)[0]
    x = x * scale
    for syn in (False, True):
        if syn and real:
            continue
        src = y if syn else x[:1] if real else x
        cot = w[..., :T] if syn else w[..., :F * M].reshape(2, 2, F, M)
        pair = lambda p: p[0] if real else Cplx(p[0], p[1])               # noqa: E731
        pair64 = lambda p: torch.complex(p[0], torch.zeros_like(p[0]) if real else p[1])      # noqa: E731
        if syn:
            run = lambda *p: cplx.pfb_synthesis(pair(p), dev(h, dtype), hop, T)               # noqa: E731
            ref = lambda *p: ref_synthesis(pair64(p), h, hop, T)                             # noqa: E731
        else:
            run = lambda *p: cplx.pfb_analysis(pair(p), dev(h, dtype), M, hop)                # noqa: E731
            ref = lambda *p: ref_analysis(pair64(p), h, M, hop)                              # noqa: E731
        got = grads(run, [dev(p, dtype) for p in src], [dev(c, dtype) for c in cot], order)
        want = grads(ref, list(src), list(cot), order)
        assert len(got) == (1 if real else 2) and got[0].dtype == dtype
        z = torch.zeros_like
        check(Cplx(got[0], got[-1] if not real else z(got[0])), torch.complex(want[0], want[-1] if not real else z(want[0])), dtype)


def test_capture_replays_the_eager_bits():
    x, h = data(64, 8, 64 * 40, F32)
    xr, xi, h = dev(x[0], F32).requires_grad_(), dev(x[1], F32).requires_grad_(), dev(h, F32)

    def step():                                           # (one scalar root, made on the capturing stream)
        y = cplx.pfb_analysis(Cplx(xr, xi), h, 64, 32)
        return (y.real, y.imag) + torch.autograd.grad((y.real ** 2).sum() + (y.imag ** 2).sum(), (xr, xi))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()                                    # the eager result, and the warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for _ in range(3):
        held[2].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(held, eager))
    e = cplx.pfb_analysis(Cplx(xr[:0], xi[:0]), h, 64)
    assert e.shape == (0, 33, 64) and cplx.pfb_synthesis(e, h).shape == (0, 32 * 64 + 512)
