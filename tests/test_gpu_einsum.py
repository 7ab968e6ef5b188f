"""cplx.einsum on the MI355X: every fixture case against the reference's outputs and all four gradients (float32, float64),
bf16 against numpy.einsum of the rounded operands, on both routes (CPLXAMD_EINSUM_GEMM = 1 / 0); operand layouts the
fixture cannot express (bit for bit); agreement with `@` and `cplx.linear`; sizes beyond the old grid.z limit and
multi-tile shapes with tails; determinism; second derivatives; hipGraph capture.

Tolerances (README "Tolerances"): float32 |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|; float64 rtol 1e-10; bf16
|got - exp| <= 2^-8 |exp| + 1e-5 max|exp| (one round-to-nearest bf16 step on the result + the float32 accumulation
allowance), exp = complex128 arithmetic on the bf16-rounded operands."""
import numpy as np
import pytest
import torch

from cplxmodule_amd import Cplx, cplx, einsum as E
from cplxmodule_amd._lib import CplxAmdError

from conftest import load_golden
from gpu_util import DEV, N, T, bf16_round

pytestmark = pytest.mark.gpu
ROUTES = ("1", "0")
PLANES = ("ar", "ai", "br", "bi")


@pytest.fixture(scope="module")
def fx():
    return load_golden("einsum")


def tags(fx):
    return [str(t) for t in fx["cases"]]


def check(got, ref, rtol, atol_rel, what):
    """|got - ref| <= rtol |ref| + atol_rel max|ref|, printing the achieved norm-wise error first"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max()) / max(scale, 1e-300) if ref.size else 0.0
    print(f"{what}: max|got - ref| / max|ref| = {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale, err_msg=what)


def run(eq, planes, g, dtype):
    """forward + gradients of sum(re * gr + im * gi) with respect to the four planes"""
    ts = [T(p, dtype).requires_grad_(True) for p in planes]
    out = cplx.einsum(eq, Cplx(ts[0], ts[1]), Cplx(ts[2], ts[3]))
    assert out.real.dtype == dtype and out.imag.dtype == dtype
    loss = (out.real.double() * T(g[0]).double()).sum() + (out.imag.double() * T(g[1]).double()).sum()
    grads = torch.autograd.grad(loss, ts)
    return out, grads


def expected_f64(eq, planes, g):
    """complex128 / float64 arithmetic on the host: numpy.einsum for the value, float64 autograd of the reference's
    four-product formula for the gradients"""
    a = planes[0].astype(np.float64) + 1j * planes[1].astype(np.float64)
    b = planes[2].astype(np.float64) + 1j * planes[3].astype(np.float64)
    want = np.einsum(eq.replace(" ", ""), a, b)
    ts = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)).requires_grad_(True) for p in planes]
    re = torch.einsum(eq, ts[0], ts[2]) - torch.einsum(eq, ts[1], ts[3])
    im = torch.einsum(eq, ts[0], ts[3]) + torch.einsum(eq, ts[1], ts[2])
    loss = (re * torch.from_numpy(np.asarray(g[0], dtype=np.float64))).sum() + \
        (im * torch.from_numpy(np.asarray(g[1], dtype=np.float64))).sum()
    return want, [t.numpy() for t in torch.autograd.grad(loss, ts)]


# ---- the fixture, both routes ---------------------------------------------------------------------------------------
def test_float32_values_and_all_gradients_match_the_reference(fx, monkeypatch):
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        for tag in tags(fx):
            eq = str(fx[f"{tag}_eq"])
            out, grads = run(eq, [fx[f"{tag}_{p}"] for p in PLANES], (fx[f"{tag}_gr"], fx[f"{tag}_gi"]), torch.float32)
            what = f"f32 route={route} {tag}"
            check(N(out.real), fx[f"{tag}_f32_re"], 1e-5, 1e-5, what + " re")
            check(N(out.imag), fx[f"{tag}_f32_im"], 1e-5, 1e-5, what + " im")
            for p, gr in zip(PLANES, grads):
                check(N(gr), fx[f"{tag}_f32_d{p}"], 1e-5, 1e-5, what + " d" + p)


def test_float64_values_and_all_gradients_match_the_reference(fx):
    for tag in tags(fx):
        eq = str(fx[f"{tag}_eq"])
        out, grads = run(eq, [fx[f"{tag}_{p}"] for p in PLANES], (fx[f"{tag}_gr"], fx[f"{tag}_gi"]), torch.float64)
        n64 = lambda t: t.detach().cpu().numpy()  # noqa: E731
        check(n64(out.real), fx[f"{tag}_f64_re"], 1e-10, 1e-10, f"f64 {tag} re")
        check(n64(out.imag), fx[f"{tag}_f64_im"], 1e-10, 1e-10, f"f64 {tag} im")
        for p, gr in zip(PLANES, grads):
            check(n64(gr), fx[f"{tag}_f64_d{p}"], 1e-10, 1e-10, f"f64 {tag} d{p}")


def test_bfloat16_values_and_all_gradients_match_complex128_of_the_rounded_operands(fx, monkeypatch):
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        for tag in tags(fx):
            eq = str(fx[f"{tag}_eq"])
            planes = [bf16_round(fx[f"{tag}_{p}"]) for p in PLANES]
            g = (bf16_round(fx[f"{tag}_gr"]), bf16_round(fx[f"{tag}_gi"]))
            want, wgrads = expected_f64(eq, planes, g)
            out, grads = run(eq, planes, g, torch.bfloat16)
            what = f"bf16 route={route} {tag}"
            check(N(out.real), want.real, 2.0 ** -8, 1e-5, what + " re")
            check(N(out.imag), want.imag, 2.0 ** -8, 1e-5, what + " im")
            for p, gr, w in zip(PLANES, grads, wgrads):
                check(N(gr), w, 2.0 ** -8, 1e-5, what + " d" + p)


# ---- layouts the fixture cannot express ------------------------------------------------------------------------------
def _layouts(x):
    """name -> (view, the same values in contiguous storage): transposed storage, a slice at an odd element offset (no
    16-byte loads), every other element, and the first slice expanded along the leading dimension (stride 0)"""
    out = {}
    if x.dim() >= 2:
        out["transposed"] = (x.transpose(0, -1).contiguous().transpose(0, -1), x)
    flat = torch.zeros(x.numel() + 3, dtype=x.dtype, device=x.device)
    flat[3:] = x.reshape(-1)
    out["offset"] = (flat[3:].view(x.shape), x)
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], dtype=x.dtype, device=x.device)
    wide[..., ::2] = x
    out["every_other"] = (wide[..., ::2], x)
    e = x[:1].expand(x.shape)
    out["expanded"] = (e, e.contiguous())
    return out


def test_operand_layouts_give_the_same_bits(fx, monkeypatch):
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        for tag in tags(fx):
            eq = str(fx[f"{tag}_eq"])
            ar, ai, br, bi = (T(fx[f"{tag}_{p}"]) for p in PLANES)
            la_r, la_i, lb_r, lb_i = _layouts(ar), _layouts(ai), _layouts(br), _layouts(bi)
            for name in ("transposed", "offset", "every_other", "expanded"):
                for which in ("a", "b", "ab"):
                    pick = lambda lay, x, on: lay.get(name, (x, x)) if on else (x, x)  # noqa: E731
                    (xr, xr0), (xi, xi0) = pick(la_r, ar, "a" in which), pick(la_i, ai, "a" in which)
                    (yr, yr0), (yi, yi0) = pick(lb_r, br, "b" in which), pick(lb_i, bi, "b" in which)
                    got = cplx.einsum(eq, Cplx(xr, xi), Cplx(yr, yi))
                    base = cplx.einsum(eq, Cplx(xr0, xi0), Cplx(yr0, yi0))
                    routes = [E.plan(eq, [u.shape, v.shape], [u.stride(), v.stride()]).route for u, v in ((xr, yr), (xr0, yr0))]
                    what = f"layout route={route} {tag} {name}/{which}"
                    if routes[0] == routes[1]:
                        assert torch.equal(got.real, base.real) and torch.equal(got.imag, base.imag), what
                    else:
                        # exactly one of the two layouts fused into one M, one N and one K mode and ran the GEMM family
                        # (split-K: its own summation order), the other ran the contraction kernel: with
                        # CPLXAMD_EINSUM_GEMM=1 only, e.g. `linear` / `two_k_modes` / `diag_operand` on views that no
                        # longer fuse, `ref_3` / `ref_4` on a transposed B whose two K modes become adjacent
                        assert route == "1" and "cgemm" in routes, what
                        check(N(got.real), N(base.real), 1e-5, 1e-5, what + " re")
                        check(N(got.imag), N(base.imag), 1e-5, 1e-5, what + " im")


def test_expanded_operands_and_their_gradients(monkeypatch):
    """stride-0 operands are read in place; the gradient is written at full size and summed by autograd's expand"""
    rs = np.random.RandomState(5)
    w = [rs.randn(33, 20).astype(np.float32) for _ in range(2)]
    x = [rs.randn(7, 9, 20).astype(np.float32) for _ in range(2)]
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        wr, wi = (T(v).requires_grad_(True) for v in w)
        dense = [T(v) for v in x]
        big = Cplx(wr.expand(7, 33, 20), wi.expand(7, 33, 20))
        out = cplx.einsum("bsi,boi->bso", Cplx(*dense), big)
        ref = cplx.einsum("bsi,boi->bso", Cplx(*dense), Cplx(big.real.contiguous(), big.imag.contiguous()))
        assert torch.equal(out.real, ref.real) and torch.equal(out.imag, ref.imag)
        gr, gi = torch.autograd.grad(out.real.sum() - out.imag.sum(), (wr, wi))
        X = x[0].astype(np.float64) + 1j * x[1]
        d = np.einsum("bso,bsi->oi", np.full((7, 9, 33), 1 - 1j), X.conj())
        check(N(gr), d.real, 1e-5, 1e-5, f"expand route={route} dwr")
        check(N(gi), d.imag, 1e-5, 1e-5, f"expand route={route} dwi")


# ---- agreement with what exists ----------------------------------------------------------------------------------------
def test_agrees_with_matmul_and_linear(fx, monkeypatch):
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        for dtype, rtol in ((torch.float32, 1e-5), (torch.bfloat16, 2.0 ** -8)):
            p = Cplx(T(fx["bmm_ar"], dtype), T(fx["bmm_ai"], dtype))
            q = Cplx(T(fx["bmm_br"], dtype), T(fx["bmm_bi"], dtype))
            got, ref = cplx.einsum("bmk,bkn->bmn", p, q), p @ q
            check(N(got.real), N(ref.real), rtol, 1e-5, f"vs @ route={route} {dtype} re")
            check(N(got.imag), N(ref.imag), rtol, 1e-5, f"vs @ route={route} {dtype} im")
            x = Cplx(T(fx["linear_ar"], dtype), T(fx["linear_ai"], dtype))
            w = Cplx(T(fx["linear_br"], dtype), T(fx["linear_bi"], dtype))
            got, ref = cplx.einsum("bsi,oi->bso", x, w), cplx.linear(x, w)
            check(N(got.real), N(ref.real), rtol, 1e-5, f"vs linear route={route} {dtype} re")
            check(N(got.imag), N(ref.imag), rtol, 1e-5, f"vs linear route={route} {dtype} im")


# ---- sizes ---------------------------------------------------------------------------------------------------------
def test_seventy_thousand_small_products_in_one_call():
    rs = np.random.RandomState(6)
    a = [rs.randn(70000, 8, 8).astype(np.float32) for _ in range(2)]
    b = [rs.randn(70000, 8, 8).astype(np.float32) for _ in range(2)]
    out = cplx.einsum("zmk,zkn->zmn", Cplx(T(a[0]), T(a[1])), Cplx(T(b[0]), T(b[1])))
    want = np.einsum("zmk,zkn->zmn", a[0].astype(np.float64) + 1j * a[1], b[0].astype(np.float64) + 1j * b[1])
    check(N(out.real), want.real, 1e-5, 1e-5, "70000 x (8 x 8 x 8) re")
    check(N(out.imag), want.imag, 1e-5, 1e-5, "70000 x (8 x 8 x 8) im")


def test_bf16_multi_tile_shape_with_tails():
    rs = np.random.RandomState(7)
    a = [bf16_round(rs.randn(3, 257, 1000) * 0.7) for _ in range(2)]
    b = [bf16_round(rs.randn(3, 1000, 130) * 0.7) for _ in range(2)]
    want = np.einsum("bmk,bkn->bmn", a[0].astype(np.float64) + 1j * a[1], b[0].astype(np.float64) + 1j * b[1])
    bf = torch.bfloat16
    for name, bt in (("B as stored [b, k, n]", lambda v: T(v, bf)),
                     ("B K-contiguous", lambda v: T(np.ascontiguousarray(v.transpose(0, 2, 1)), bf).transpose(1, 2))):
        out = cplx.einsum("bmk,bkn->bmn", Cplx(T(a[0], bf), T(a[1], bf)), Cplx(bt(b[0]), bt(b[1])))
        check(N(out.real), want.real, 2.0 ** -8, 1e-5, f"bf16 3 x 257 x 130 x 1000, {name}, re")
        check(N(out.imag), want.imag, 2.0 ** -8, 1e-5, f"bf16 3 x 257 x 130 x 1000, {name}, im")
    # the same in float32 on the 128-wide tile, result permuted
    out = cplx.einsum("bmk,bkn->nbm", Cplx(T(a[0]), T(a[1])), Cplx(T(b[0]), T(b[1])))
    check(N(out.real), want.real.transpose(2, 0, 1), 1e-5, 1e-5, "f32 3 x 257 x 130 x 1000 -> nbm, re")
    check(N(out.imag), want.imag.transpose(2, 0, 1), 1e-5, 1e-5, "f32 3 x 257 x 130 x 1000 -> nbm, im")


def test_the_128_wide_tile_in_both_precisions_and_every_load_path():
    """16 x 4 x 4 tiles of 128 x 128 select the large tile (the shapes above run on the 64-wide one); M and N tails;
    B as stored is N-contiguous (16-byte loads of 8 rows in bf16), its transposed copy K-contiguous, the offset view
    takes the scalar paths: equal bits in all three"""
    rs = np.random.RandomState(9)
    a = [bf16_round(rs.randn(16, 500, 72) * 0.7) for _ in range(2)]
    b = [bf16_round(rs.randn(16, 72, 504) * 0.7) for _ in range(2)]
    want = np.einsum("bmk,bkn->bmn", a[0].astype(np.float64) + 1j * a[1], b[0].astype(np.float64) + 1j * b[1])

    def off(t):
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)

    for dtype, rtol in ((torch.bfloat16, 2.0 ** -8), (torch.float32, 1e-5)):
        p = Cplx(T(a[0], dtype), T(a[1], dtype))
        q = Cplx(T(b[0], dtype), T(b[1], dtype))
        out = cplx.einsum("bmk,bkn->bmn", p, q)
        check(N(out.real), want.real, rtol, 1e-5, f"128 tile {dtype} re")
        check(N(out.imag), want.imag, rtol, 1e-5, f"128 tile {dtype} im")
        qt = Cplx(q.real.transpose(1, 2).contiguous().transpose(1, 2), q.imag.transpose(1, 2).contiguous().transpose(1, 2))
        for name, (u, v) in (("B K-contiguous", (p, qt)), ("odd offsets", (Cplx(off(p.real), off(p.imag)), Cplx(off(q.real), off(q.imag))))):
            o2 = cplx.einsum("bmk,bkn->bmn", u, v)
            assert torch.equal(o2.real, out.real) and torch.equal(o2.imag, out.imag), (dtype, name)
        o3 = cplx.einsum("bmk,bkn->nbm", p, q)             # C's unit stride in M: the operands swap roles
        check(N(o3.real), want.real.transpose(2, 0, 1), rtol, 1e-5, f"128 tile {dtype} -> nbm re")
        check(N(o3.imag), want.imag.transpose(2, 0, 1), rtol, 1e-5, f"128 tile {dtype} -> nbm im")


def test_extent_zero_and_scalar_results():
    z = lambda *s: Cplx(torch.randn(*s, device=DEV), torch.randn(*s, device=DEV))  # noqa: E731
    out = cplx.einsum("ij,jk->ik", z(0, 3), z(3, 4))
    assert out.shape == (0, 4)
    out = cplx.einsum("ij,jk->ik", z(2, 0), z(0, 4))
    assert out.shape == (2, 4) and not out.real.any() and not out.imag.any()
    a, b = z(5), z(5)
    out = cplx.einsum("i,i->", a, b)
    assert out.shape == ()
    want = (N(a.real).astype(np.float64) + 1j * N(a.imag)) @ (N(b.real).astype(np.float64) + 1j * N(b.imag))
    np.testing.assert_allclose(complex(out.item()), want, rtol=1e-5, atol=1e-5)
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.einsum("i,i->", a, Cplx(b.real.cpu(), b.imag.cpu()))
    with pytest.raises(RuntimeError, match="does not broadcast"):
        cplx.einsum("ij,jk->ik", z(2, 3), z(4, 4))


# ---- determinism, higher derivatives, graphs -------------------------------------------------------------------------------
def test_two_runs_give_equal_bits(fx):
    for dtype in (torch.float32, torch.bfloat16):
        for tag in ("heads", "k_split_order", "dot", "bmm_out_perm"):
            eq = str(fx[f"{tag}_eq"])
            runs = [run(eq, [fx[f"{tag}_{p}"] for p in PLANES], (fx[f"{tag}_gr"], fx[f"{tag}_gi"]), dtype) for _ in range(2)]
            (o1, g1), (o2, g2) = runs
            assert torch.equal(o1.real, o2.real) and torch.equal(o1.imag, o2.imag), (tag, dtype)
            assert all(torch.equal(u, v) for u, v in zip(g1, g2)), (tag, dtype)


def test_second_derivatives_against_the_float64_route(fx, monkeypatch):
    for route in ROUTES:
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", route)
        for tag in ("heads", "linear", "ellipsis_bcast"):
            eq = str(fx[f"{tag}_eq"])
            res = {}
            for dtype in (torch.float32, torch.float64):
                ts = [T(fx[f"{tag}_{p}"], dtype).requires_grad_(True) for p in PLANES]
                out = cplx.einsum(eq, Cplx(ts[0], ts[1]), Cplx(ts[2], ts[3]))
                loss = (out.real * T(fx[f"{tag}_gr"], dtype)).sum() + (out.imag * T(fx[f"{tag}_gi"], dtype)).sum()
                first = torch.autograd.grad(loss, ts, create_graph=True)
                # a scalar of the first derivatives that couples the operands: its gradient is a second derivative
                s = sum((g * g).sum() for g in first)
                res[dtype] = [t.detach().double().cpu().numpy() for t in torch.autograd.grad(s, ts)]
            for p, got, ref in zip(PLANES, res[torch.float32], res[torch.float64]):
                check(got, ref, 1e-5, 1e-5, f"second derivative route={route} {tag} {p}")


def test_forward_and_backward_replay_in_a_graph(fx):
    tag = "heads"
    eq = str(fx[f"{tag}_eq"])
    ts = [T(fx[f"{tag}_{p}"]).requires_grad_(True) for p in PLANES]
    g_r, g_i = T(fx[f"{tag}_gr"]), T(fx[f"{tag}_gi"])

    def step():
        out = cplx.einsum(eq, Cplx(ts[0], ts[1]), Cplx(ts[2], ts[3]))
        grads = torch.autograd.grad((out.real * g_r).sum() + (out.imag * g_i).sum(), ts)
        return (out.real, out.imag) + tuple(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    rs = np.random.RandomState(8)
    for _ in range(2):
        with torch.no_grad():
            for t in ts:
                t.copy_(T(rs.randn(*t.shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for c, e in zip(captured, eager):
            assert torch.equal(c, e)
