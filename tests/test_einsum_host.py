"""cplx.einsum without a GPU: the fixture against numpy.einsum, the host planner (group classification, fusion, routes,
and the plan EXECUTED by a numpy loop over its offsets -- the descriptor is what the kernel walks), the error contract,
one-operand equations, and the argument checks of cplxamd_ceinsum."""
import ctypes

import numpy as np
import pytest
import torch

from cplxmodule_amd import Cplx, cplx, einsum as E
from cplxmodule_amd._lib import CplxAmdError

from conftest import load_golden


@pytest.fixture(scope="module")
def fx():
    return load_golden("einsum")


def tags(fx):
    return [str(t) for t in fx["cases"]]


def operands(fx, tag):
    a = fx[f"{tag}_ar"].astype(np.float64) + 1j * fx[f"{tag}_ai"]
    b = fx[f"{tag}_br"].astype(np.float64) + 1j * fx[f"{tag}_bi"]
    return str(fx[f"{tag}_eq"]), a, b


def offsets(group, attr):
    o = np.zeros(1, dtype=np.int64)
    for md in group:                       # the last mode runs fastest
        o = (o[:, None] + np.arange(md.extent, dtype=np.int64) * getattr(md, attr)).ravel()
    return o


def run_plan(p, a_flat, b_flat, a0=0, b0=0):
    """C = the plan's contraction, by its offsets alone: what csrc/einsum.hip computes."""
    A = a_flat[a0 + offsets(p.batch, "sa")[:, None, None] + offsets(p.m, "sa")[None, :, None] + offsets(p.k, "sa")]
    B = b_flat[b0 + offsets(p.batch, "sb")[:, None, None] + offsets(p.n, "sb")[None, :, None] + offsets(p.k, "sb")]
    if p.conj_a:
        A = A.conj()
    if p.conj_b:
        B = B.conj()
    c = np.zeros(int(np.prod(p.out_shape, dtype=np.int64)), dtype=np.complex128)
    idx = offsets(p.batch, "sc")[:, None, None] + offsets(p.m, "sc")[None, :, None] + offsets(p.n, "sc")[None, None, :]
    assert len(np.unique(idx)) == idx.size == c.size          # every output element written exactly once
    c[idx] = np.einsum("bmk,bnk->bmn", A, B)
    return c.reshape(p.out_shape)


# ---- the fixture itself ------------------------------------------------------------------------------------------
def test_fixture_agrees_with_numpy_einsum(fx):
    assert len(tags(fx)) == 21
    for tag in tags(fx):
        eq, a, b = operands(fx, tag)
        want = np.einsum(eq.replace(" ", ""), a, b)
        for prec, tol in (("f64", 1e-12), ("f32", 1e-5)):
            for part, w in (("re", want.real), ("im", want.imag)):
                got = fx[f"{tag}_{prec}_{part}"]
                assert got.shape == w.shape, (tag, prec, part)
                np.testing.assert_allclose(got, w, rtol=tol, atol=tol * np.abs(w).max(), err_msg=f"{tag} {prec} {part}")
            for name, ref in (("dar", "ar"), ("dai", "ai"), ("dbr", "br"), ("dbi", "bi")):
                assert fx[f"{tag}_{prec}_{name}"].shape == fx[f"{tag}_{ref}"].shape
                np.testing.assert_allclose(fx[f"{tag}_f32_{name}"], fx[f"{tag}_f64_{name}"], rtol=1e-5,
                                           atol=1e-5 * np.abs(fx[f"{tag}_f64_{name}"]).max(), err_msg=f"{tag} {name}")


# ---- planner -----------------------------------------------------------------------------------------------------
def test_plan_of_every_fixture_case_reproduces_numpy(fx, monkeypatch):
    for gemm in ("1", "0"):
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", gemm)
        for tag in tags(fx):
            eq, a, b = operands(fx, tag)
            p = E.plan(eq, [a.shape, b.shape])
            assert p.route in (("cgemm", "kernel") if gemm == "1" else ("kernel",)), tag
            for g in p.groups:
                assert 1 <= len(g) <= E.MAX_MODES
            want = np.einsum(eq.replace(" ", ""), a, b)
            assert p.out_shape == want.shape, tag
            np.testing.assert_allclose(run_plan(p, a.ravel(), b.ravel()), want, rtol=1e-12, atol=1e-12, err_msg=tag)


def test_plan_groups_fusion_and_routes_literally(monkeypatch):
    monkeypatch.delenv("CPLXAMD_EINSUM_GEMM", raising=False)
    M = E.Mode
    one = (M(1, 0, 0, 0, ""),)
    p = E.plan("bhqd,bhkd->bhqk", [(3, 4, 19, 16), (3, 4, 23, 16)])
    assert p.batch == (M(12, 19 * 16, 23 * 16, 19 * 23, "bh"),)
    assert p.m == (M(19, 16, 0, 23, "q"),) and p.n == (M(23, 0, 16, 1, "k"),) and p.k == (M(16, 1, 1, 0, "d"),)
    assert p.route == "kernel" and p.out_shape == (3, 4, 19, 23)

    p = E.plan("bsi,oi->bso", [(5, 6, 70), (48, 70)])
    assert p.route == "cgemm" and p.batch == one
    assert p.m == (M(30, 70, 0, 48, "bs"),) and p.n == (M(48, 0, 70, 1, "o"),) and p.k == (M(70, 1, 1, 0, "i"),)
    monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", "0")
    assert E.plan("bsi,oi->bso", [(5, 6, 70), (48, 70)]).route == "kernel"
    monkeypatch.delenv("CPLXAMD_EINSUM_GEMM")
    # the same on a transposed view of the activation ([S, B, I] storage): b and s no longer fuse, the shape stays
    x = torch.empty(6, 5, 70).transpose(0, 1)
    q = E.plan("bsi,oi->bso", [x.shape, (48, 70)], [x.stride(), (70, 1)])
    assert q.out_shape == p.out_shape == (5, 6, 48) and q.route == "kernel"
    assert q.m == (M(5, 70, 0, 6 * 48, "b"), M(6, 5 * 70, 0, 48, "s"))

    # summed-away subscript: a K mode that the other operand does not move along; diagonal: the strides add up
    p = E.plan("ijk,jl->il", [(6, 8, 5), (8, 9)])
    assert p.k == (M(8, 5, 9, 0, "j"), M(5, 1, 0, 0, "k"))
    p = E.plan("iij,jk->ik", [(8, 8, 12), (12, 5)])
    assert p.m == (M(8, 8 * 12 + 12, 0, 5, "i"),)
    # broadcast ellipsis dimension: A does not depend on it, it is a free index of B
    p = E.plan("...ik,...kj->...ij", [(2, 1, 9, 31), (3, 31, 5)])
    assert p.batch == one and [md.extent for md in p.m] == [2, 9] and [md.extent for md in p.n] == [3, 5]
    # empty groups are one mode of extent 1; extent-1 modes are dropped
    p = E.plan("ij,ij->ij", [(13, 29), (13, 29)])
    assert p.batch == (M(377, 1, 1, 1, "ij"),) and p.m == p.n == p.k == one
    assert E.plan("ik,kj->ij", [(20, 1), (1, 30)]).k == one
    # implicit output: alphabetical, upper case first; spaces are ignored
    assert E.plan(" b A , A c ", [(2, 3), (3, 4)]).out_shape == (2, 4)
    assert E.plan("bA,Ac", [(2, 3), (3, 4)]).m[0].labels == "b"
    # extent 0
    assert E.plan("ij,jk->ik", [(0, 3), (3, 4)]).route == "empty" and E.plan("ij,jk->ik", [(2, 0), (0, 4)]).route == "empty"
    assert E.plan("ij,jk->ik", [(2, 3), (3, 4)], dtype=torch.float64).route == "f64"


def test_plans_of_strided_views_execute_correctly():
    rs = np.random.RandomState(3)
    base_a = torch.from_numpy(rs.randn(2, 7, 12, 40, 2)).to(torch.complex128)
    base_b = torch.from_numpy(rs.randn(2, 7, 12, 46, 2)).to(torch.complex128)
    views = [
        ("bmk,bkn->bmn", base_a[0, :, :, :33, 0].transpose(1, 2)[:, 1::2], base_b[1, :, :, 3:20:2, 1]),
        ("bmk,bkn->nbm", base_a[0, :, 1:, 5:, 1].transpose(1, 2)[:, :, :9], base_b[0, :, :9, ::3, 0]),
        ("bmk,kn->bmn", base_a[1, :, :5, :10, 0], base_b[0, 0, :1, :6, 0].expand(10, 6)),
        ("iij,jk->ki", base_a[0, :, :7, :5, 0], base_b[1, 2, :5, :8, 1]),
    ]
    for eq, a, b in views:
        p = E.plan(eq, [a.shape, b.shape], [a.stride(), b.stride()])
        got = run_plan(p, base_a.reshape(-1).numpy(), base_b.reshape(-1).numpy(), a.storage_offset(), b.storage_offset())
        np.testing.assert_allclose(got, np.einsum(eq, a.numpy(), b.numpy()), rtol=1e-12, atol=1e-12, err_msg=eq)
        # the torch views the autograd path takes give the same strides as the pure planner
        ins, out = E.parse(eq, [a.shape, b.shape])
        ext = E.label_extents(ins, [a.shape, b.shape])
        for t, labs in zip((a, b), ins):
            v, vl = E.operand_views(t, labs, ext)
            assert dict(zip(vl, v.stride())) == E.normalize(labs, t.shape, t.stride(), ext)


def test_backward_plans_execute_correctly():
    """dA = G conj(B) in A's label order and dB = conj(A) G in B's: the same planner with the groups re-labelled."""
    rs = np.random.RandomState(4)
    xl, yl, ol = ("b", "m", "k", "s"), ("b", "n", "k"), ("n", "b", "m")     # s: summed away in the forward
    ext = dict(b=3, m=4, k=5, s=2, n=6)
    cplxr = lambda labs: rs.randn(*[ext[c] for c in labs]) + 1j * rs.randn(*[ext[c] for c in labs])  # noqa: E731
    x, y, g = cplxr(xl), cplxr(yl), cplxr(ol)
    st = lambda labs: dict(zip(labs, E.contiguous_strides([ext[c] for c in labs])))  # noqa: E731
    p = E.contraction_plan(st(ol), st(yl), xl, ext, conj=(False, True))
    assert [md.labels for md in p.m] == ["m", "s"] and p.m[1].sa == 0          # broadcast of G along s
    np.testing.assert_allclose(run_plan(p, g.ravel(), y.ravel()),
                               np.broadcast_to(np.einsum("nbm,bnk->bmk", g, y.conj())[..., None], x.shape), atol=1e-12)
    p = E.contraction_plan(st(xl), st(ol), yl, ext, conj=(True, False))
    np.testing.assert_allclose(run_plan(p, x.ravel(), g.ravel()), np.einsum("bmks,nbm->bnk", x.conj(), g), atol=1e-12)


def test_mode_limit_and_size_limit():
    shape = (2,) * 9 + (3,)
    strides = E.contiguous_strides((4,) * 9 + (3,))          # a [:2] slice of every dimension: nothing fuses
    with pytest.raises(CplxAmdError, match="at most 8"):
        E.plan("abcdefghiz,zy->abcdefghiy", [shape, (3, 5)], [strides, (5, 1)])
    assert len(E.plan("abcdefghiz,zy->abcdefghiy", [shape, (3, 5)]).m) == 1      # contiguous: one fused mode
    with pytest.raises(CplxAmdError, match="2\\^31"):
        E.plan("ab,->ab", [(2 ** 16, 2 ** 16), ()])       # one fused M mode of 2^32 indices


def test_malformed_equations_raise_torchs_own_errors():
    for eq, shapes in [("ijk,ikj", [(6, 16, 24), (6, 24, 15)]), ("ij,jk->iz", [(2, 3), (3, 4)]), ("iij,jk->ik", [(8, 7, 12), (12, 5)]),
                       ("ij,jk->ii", [(2, 3), (3, 4)]), ("ij,j.k", [(2, 3), (3, 4)]), ("ijk,jk", [(2, 3), (3, 4)])]:
        with pytest.raises(RuntimeError) as mine:
            E.plan(eq, shapes)
        with pytest.raises(RuntimeError) as theirs:
            torch.einsum(eq, *[torch.zeros(s) for s in shapes])
        assert str(mine.value) == str(theirs.value), eq
        assert not isinstance(mine.value, CplxAmdError)


# ---- the public function's error contract (no GPU) ------------------------------------------------------------------
def test_operand_count_and_type_errors():
    z = Cplx(torch.randn(3, 4), torch.randn(3, 4))
    w = Cplx(torch.randn(4, 5), torch.randn(4, 5))
    with pytest.raises(RuntimeError, match="requires at least one tensor"):
        cplx.einsum("ij")
    with pytest.raises(RuntimeError, match="does not support more than 2 tensors. Got 3"):
        cplx.einsum("ij,jk,kl", z, w, w)
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.einsum("ij,jk", z, w.real)
    with pytest.raises(CplxAmdError, match="mixed dtypes"):
        cplx.einsum("ij,jk", z, Cplx(w.real.bfloat16(), w.imag.bfloat16()))
    with pytest.raises(CplxAmdError, match="float16"):
        cplx.einsum("ij,jk", Cplx(z.real.half(), z.imag.half()), Cplx(w.real.half(), w.imag.half()))
    with pytest.raises(CplxAmdError, match="no CPU path"):
        cplx.einsum("ij,jk", z, w)


def test_one_operand_equations_on_cpu_equal_the_fixture(fx):
    assert len(fx["cases1"]) == 8
    for tag in (str(t) for t in fx["cases1"]):
        z = Cplx(torch.from_numpy(fx[f"{tag}_zr"]).double(), torch.from_numpy(fx[f"{tag}_zi"]).double())
        out = cplx.einsum(str(fx[f"{tag}_eq"]), z)
        np.testing.assert_allclose(out.real.numpy(), fx[f"{tag}_re"], rtol=1e-12, atol=1e-12, err_msg=tag)
        np.testing.assert_allclose(out.imag.numpy(), fx[f"{tag}_im"], rtol=1e-12, atol=1e-12, err_msg=tag)
    with pytest.raises(RuntimeError, match="but the sizes don't match"):
        cplx.einsum("iij", Cplx(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5)))


# ---- C ABI: every argument check happens before any GPU call -----------------------------------------------------------
def test_ceinsum_rejects_bad_arguments_without_a_gpu():
    from cplxmodule_amd import _lib, ops
    L = _lib.load()
    ok = ctypes.c_void_p(256)
    d = ops.einsum_desc(E.plan("bmk,bkn->bmn", [(2, 3, 4), (2, 4, 5)]))
    call = lambda d, a=ok, dt=(_lib.F32, _lib.F32): L.cplxamd_ceinsum(a, ok, ok, ok, ok, ok, ctypes.byref(d), 0, 0, *dt, None)  # noqa: E731
    assert ctypes.sizeof(d) == 912 < 1024
    assert call(d, a=None) == -1
    assert L.cplxamd_ceinsum(ok, ok, ok, ok, ok, ok, None, 0, 0, _lib.F32, _lib.F32, None) == -1
    assert call(d, dt=(_lib.F16, _lib.F16)) == -3 and call(d, dt=(_lib.F64, _lib.F64)) == -3 and call(d, dt=(_lib.BF16, _lib.F32)) == -3
    d.nmodes[1] = 9
    assert call(d) == -1
    d.nmodes[1] = 1
    d.stride_c[1][0] = 0
    assert call(d) == -1
    d.stride_c[1][0] = 5
    d.extent[3][0] = -4
    assert call(d) == -1
    d.extent[3][0] = 4
    d.extent[2][0] = 0                      # an empty result: success, nothing launched
    assert call(d) == 0
    d.extent[2][0] = 5
    d.nmodes[0] = 2
    d.extent[0][0], d.extent[0][1] = 2 ** 16, 2 ** 16
    d.stride_c[0][0] = d.stride_c[0][1] = 1
    assert call(d) == -3                    # a group beyond 31 bits
