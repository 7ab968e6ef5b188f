"""Shared checks of tests/test_init_host.py and tests/test_gpu_init.py: the same properties, asked of host and of device
tensors.  `u` is the unit roundoff throughout: 2^-24 (float32), 2^-53 (float64), 2^-9 (bfloat16)."""
import functools

import numpy as np
import pytest
import torch

from cplxmodule_amd import Cplx
from cplxmodule_amd.nn import init
from cplxmodule_amd._lib import CplxAmdError

from conftest import load_golden

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -9}
KINDS = ("glorot", "xavier", "kaiming", "he")
NEW = ("cplx_kaiming_normal_", "cplx_xavier_normal_", "cplx_xavier_uniform_", "cplx_trabelsi_standard_",
       "cplx_trabelsi_independent_")
# Gaussian Z under fixed seeds: tall, wide, square (the worst conditioned), k = 1, sizes off every tile multiple
POLAR_SHAPES = ((21, 25), (25, 21), (64, 64), (33, 33), (130, 67), (2048, 9), (1, 7), (5, 1))
POLAR_BOUND = {torch.float32: 64, torch.float64: 128}          # max |M - U V^H| in units of u


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("init")


def tag(shape):
    return "x".join(map(str, shape))


def c128(w):
    """Cplx (any device / dtype) -> numpy complex128."""
    return w.real.detach().double().cpu().numpy() + 1j * w.imag.detach().double().cpu().numpy()


def matrix_of(w):
    """The matrix the orthogonal initialiser fills: the weight itself, or (prod(shape[:2]), prod(shape[2:]))."""
    m = c128(w)
    return m if m.ndim == 2 else m.reshape(m.shape[0] * m.shape[1], -1)


def gram_defect(m):
    """max |G / c - I| of the Gram matrix on the short side, in float64; c = the mean of its diagonal."""
    g = m.conj().T @ m if m.shape[0] >= m.shape[1] else m @ m.conj().T
    c = np.real(np.diag(g)).mean()
    return np.abs(g / c - np.eye(g.shape[0])).max()


def orthogonality_bound(dtype):
    # float32 / float64: 32 u (four times the 8.4 u of the CPU experiment, for another summation order); bfloat16: the
    # rounding on store, 2 * 2^-9 on a diagonal entry of the Gram matrix, plus the float32 compute term
    return 2 * U[torch.bfloat16] + 32 * U[torch.float32] if dtype == torch.bfloat16 else 32 * U[dtype]


def check_independent(w, kind="glorot"):
    """Orthogonality (test 2) and standard deviation (test 3) of a weight that cplx_trabelsi_independent_ filled."""
    fx = fixture()
    m = matrix_of(w)
    assert np.isfinite(m).all()
    defect = gram_defect(m)
    print(f"trabelsi_independent_ {tuple(w.shape)} {w.dtype} {w.device.type}: defect {defect / U[w.dtype]:.2f} u")
    assert defect <= orthogonality_bound(w.dtype)
    scale = float(fx[f"std_{tag(w.shape)}_{kind.lower()}"])       # M.std() of a reference run ...
    np.testing.assert_allclose(scale, float(fx[f"scale_{tag(w.shape)}_{kind.lower()}"]), rtol=1e-12)   # ... is the formula
    if w.dtype != torch.bfloat16:
        np.testing.assert_allclose(m.std(), scale, rtol=1e-5 if w.dtype == torch.float32 else 1e-12)
    else:      # (not among the issue's cases: every entry is rounded to 2^-9 relative, so is the root mean square)
        np.testing.assert_allclose(m.std(), scale, rtol=U[torch.bfloat16])


def gaussian(shape, dtype, seed):
    rs = np.random.RandomState(seed)
    z = rs.randn(2, *shape)
    return Cplx(torch.from_numpy(z[0]).to(dtype), torch.from_numpy(z[1]).to(dtype))


def svd_polar(z):
    """U V^H of the float64 SVD of the values z holds (numpy.linalg.svd(full_matrices=False), the reference's routine)."""
    u, _, vh = np.linalg.svd(c128(z), full_matrices=False)
    return u @ vh


def polar_error(z, m):
    """max |M - U V^H| in units of u of z's dtype."""
    assert m.shape == z.shape and m.dtype == z.dtype and m.device == z.device
    got = c128(m)
    assert np.isfinite(got).all()
    return np.abs(got - svd_polar(z)).max() / U[z.dtype]


# ---- the contract (test 6), on any device -----------------------------------------------------------------------------
def check_seeding(device):
    for name in NEW:
        fn = getattr(init, name)
        a, b, c = (Cplx.empty(12, 20, device=device) for _ in range(3))
        torch.manual_seed(11)
        fn(a)
        fn(c)
        torch.manual_seed(11)
        fn(b)
        assert np.array_equal(c128(a), c128(b)), name
        assert not np.array_equal(c128(a), c128(c)), name


def check_layers(device):
    from cplxmodule_amd.nn import CplxConv2d, CplxLinear
    for layer in (CplxLinear(20, 12).to(device), CplxConv2d(6, 8, 3).to(device)):
        before = c128(layer.weight)
        for kind in KINDS:
            out = init.cplx_trabelsi_independent_(layer.weight, kind=kind)
            assert out.real is layer.weight.real and out.imag is layer.weight.imag        # the Parameters themselves
            assert isinstance(layer.weight.real, torch.nn.Parameter) and layer.weight.real.requires_grad
            assert layer.weight.real.grad_fn is None and layer.weight.imag.grad_fn is None
            m = matrix_of(layer.weight)
            assert not np.array_equal(c128(layer.weight), before)
            fan_in, fan_out = init.get_fans(layer.weight)
            want = 1 / np.sqrt(fan_in + fan_out) if kind in ("glorot", "xavier") else 1 / np.sqrt(fan_in)
            np.testing.assert_allclose(m.std(), want, rtol=1e-5)
            assert gram_defect(m) <= orthogonality_bound(torch.float32)
        init.cplx_trabelsi_standard_(layer.weight)
        assert dict(layer.named_parameters())["weight.real"] is layer.weight.real


def check_strided(device):
    for name in ("cplx_trabelsi_independent_", "cplx_trabelsi_standard_", "cplx_xavier_normal_"):
        fn = getattr(init, name)
        base = Cplx(torch.full((25, 21), 7.0, device=device), torch.full((25, 21), 7.0, device=device))
        view = base.t()
        assert not view.real.is_contiguous()
        dense = Cplx.empty(21, 25, device=device)
        torch.manual_seed(5)
        assert fn(view) is view
        torch.manual_seed(5)
        fn(dense)
        assert np.array_equal(c128(base), c128(view).T) and not np.any(c128(base).real == 7.0), name
        if name == "cplx_trabelsi_independent_":      # (torch's own fills may draw in another order on a strided tensor)
            assert np.array_equal(c128(view), c128(dense)), name
    # every second row of a larger buffer: the rows in between stay untouched
    buf = Cplx(torch.zeros(12, 9, device=device), torch.zeros(12, 9, device=device))
    init.cplx_trabelsi_independent_(buf[::2])
    assert np.all(c128(buf)[1::2] == 0) and np.all(c128(buf)[::2] != 0)
    assert gram_defect(c128(buf)[::2]) <= orthogonality_bound(torch.float32)


def check_autograd_flags(device):
    for name in NEW:
        fn = getattr(init, name)
        for rg in (False, True):
            w = Cplx.empty(6, 10, device=device, requires_grad=rg)
            assert fn(w) is w, name
            for plane in (w.real, w.imag):
                assert plane.requires_grad is rg and plane.grad_fn is None and plane.is_leaf, name


def check_rejections(device):
    for name in NEW + ("cplx_polar_factor",):
        with pytest.raises(ValueError, match="fewer than 2 dimensions"):
            getattr(init, name)(Cplx.empty(32, device=device))
    for fn in (init.cplx_trabelsi_standard_, init.cplx_trabelsi_independent_):
        for kind in ("orthogonal", "", "glorot "):
            with pytest.raises(AssertionError):
                fn(Cplx.empty(4, 6, device=device), kind=kind)


def check_polar_failures(device):
    """CplxAmdError, promptly, on inputs without a (unique) polar factor -- never a hang, never NaN."""
    for dtype in (torch.float32, torch.float64):
        bad = {"zeros": Cplx.zeros(4, 4, dtype=dtype, device=device)}
        z = gaussian((4, 4), dtype, 1).to(device)
        z.imag[2, 1] = float("nan")
        bad["nan"] = z
        z = gaussian((4, 4), dtype, 1).to(device)
        z.real[0, 3] = float("inf")
        bad["inf"] = z
        z = gaussian((6, 4), dtype, 2).to(device)
        z.real[:, 2], z.imag[:, 2] = z.real[:, 0].clone(), z.imag[:, 0].clone()
        bad["equal columns"] = z
        for what, z in bad.items():
            with pytest.raises(CplxAmdError) as e:
                init.cplx_polar_factor(z)
            if what == "equal columns":
                steps = int(str(e.value).split("after ")[1].split()[0])
                assert steps <= 100, str(e.value)


def check_redraw(device, monkeypatch):
    """A draw of Z that does not reach the threshold within the step cap is drawn again, not reported: the initialiser
    must not fail at random on its own Z.  torch.randn is made to hand out rank-deficient matrices (two equal columns)."""
    real_randn, calls = torch.randn, []

    def randn(*size, **kw):
        z = real_randn(*size, **kw)
        calls.append(tuple(size))
        if len(calls) <= bad_draws:
            z[:, :, 2] = z[:, :, 0]
        return z
    monkeypatch.setattr(torch, "randn", randn)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        bad_draws, w = 2, Cplx.zeros(6, 4, dtype=dtype, device=device)
        del calls[:]
        torch.manual_seed(41)
        assert init.cplx_trabelsi_independent_(w) is w
        assert calls == [(2, 6, 4)] * 3                         # two draws discarded, the third kept
        m = matrix_of(w)
        assert gram_defect(m) <= orthogonality_bound(dtype)
        np.testing.assert_allclose(m.std(), 1 / np.sqrt(10), rtol=1e-5 if dtype != torch.bfloat16 else U[dtype])
        # the result is a function of the seed alone: the same as keeping the third draw of that stream
        ref = Cplx.zeros(6, 4, dtype=dtype, device=device)
        bad_draws = 0
        torch.manual_seed(41)
        real_randn(2, 6, 4, dtype=init._compute_dtype(dtype), device=device)
        real_randn(2, 6, 4, dtype=init._compute_dtype(dtype), device=device)
        init.cplx_trabelsi_independent_(ref)
        assert np.array_equal(c128(w), c128(ref))
    # a generator that never delivers a full-rank matrix: the error comes after the bounded number of draws, the tensor
    # is left as it was
    bad_draws, w = 10 ** 9, Cplx.zeros(6, 4, device=device)
    del calls[:]
    with pytest.raises(CplxAmdError, match="not converged"):
        init.cplx_trabelsi_independent_(w)
    assert len(calls) == init._MAX_DRAWS == 16 and not np.any(c128(w))
    # cplx_polar_factor on a caller's matrix still reports it
    z = real_randn(2, 6, 4, device=device)
    z[:, :, 2] = z[:, :, 0]
    with pytest.raises(CplxAmdError, match="not converged"):
        init.cplx_polar_factor(Cplx(z[0], z[1]))
