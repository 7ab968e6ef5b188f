"""The full spectrum of cplx.stft / istft on the GPU (the complex kernels under csrc/stft_c2c*.hip): stft of a `Cplx`
signal, stft of a real signal with `onesided=False` (a null imaginary plane), and istft with `return_complex=True`, over
every path of the underlying complex transform, the framing and workgroup seams, layouts, bf16, the round trip, the
adjoint identity, gradients of first and second order, reruns and capture.  Cases and references as in test_gpu_stft.py:
`torch.stft` / `torch.istft` in complex128 on the CPU from the values the kernel was given; bounds: fft_cases.py."""
import pytest
import torch

import fft_cases as fc
import rfft_cases as rc
import stft_cases as sc
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import stft as hoststft
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

WIDE = [torch.float32, torch.float64]
WIDE_IDS = ["f32", "f64"]


def dev_win(win):
    return None if win is None else win.to(DEV)


def dev_cplx(re, im, requires_grad=False):
    return Cplx(re.to(DEV).requires_grad_(requires_grad), im.to(DEV).requires_grad_(requires_grad))


def ones_if_none(win, n_fft, win_length=None):
    return torch.ones(win_length or n_fft, dtype=torch.float64) if win is None else win.double()


def ref_cstft(re, im, n_fft, hop_length=None, win_length=None, window=None, **kw):
    """torch.stft in complex128 on the CPU of the signal re + i im [..., T] -> complex128 [..., n_fft, frames]"""
    z = fc.c128(re, im)
    out = torch.stft(z.reshape(-1, z.shape[-1]), n_fft, hop_length, win_length, ones_if_none(window, n_fft, win_length),
                     return_complex=True, **kw)
    return out.reshape(*z.shape[:-1], *out.shape[-2:])


def ref_cistft(re, im, n_fft, hop_length=None, win_length=None, window=None, **kw):
    """torch.istft(onesided=False, return_complex=True) in complex128 on the CPU -> complex128 [..., T]"""
    z = fc.c128(re, im)
    out = torch.istft(z.reshape(-1, *z.shape[-2:]), n_fft, hop_length, win_length, ones_if_none(window, n_fft, win_length),
                      onesided=False, return_complex=True, **kw)
    return out.reshape(*z.shape[:-2], out.shape[-1])


def check(got, ref, dtype, what):
    assert got.real.dtype == dtype and got.imag.dtype == dtype and tuple(got.real.shape) == tuple(ref.shape), what
    err = fc.normwise(got, ref)
    print(f"stft_parity full {what} {dtype}: {err:.3g}")
    assert err <= fc.tol(dtype), (what, err)
    return got


# ---- 1. every path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", sc.PATH_LENGTHS)
def test_every_path(n_fft, dtype):
    hop, T, rows = sc.path_geometry(n_fft)
    win = sc.window("rand", n_fft)
    re, im = fc.gaussian((rows, T), dtype, seed=400 + n_fft)
    S = check(cplx.stft(dev_cplx(re, im), n_fft, hop, window=dev_win(win)), ref_cstft(re, im, n_fft, hop, window=win), dtype,
              f"stft Cplx n_fft={n_fft}")
    assert S.real.shape[-2] == n_fft and S.real.transpose(-1, -2).is_contiguous() and S.imag.transpose(-1, -2).is_contiguous()
    check(cplx.stft(re.to(DEV), n_fft, hop, window=dev_win(win), onesided=False),
          sc.ref_stft(re, n_fft, hop, window=win, onesided=False), dtype, f"stft real onesided=False n_fft={n_fft}")
    xr, xi = fc.gaussian((rows, n_fft, S.real.shape[-1]), dtype, seed=401 + n_fft)
    y = cplx.istft(dev_cplx(xr, xi), n_fft, hop, window=dev_win(win), onesided=False, return_complex=True)
    assert isinstance(y, Cplx)
    check(y, ref_cistft(xr, xi, n_fft, hop, window=win), dtype, f"istft return_complex n_fft={n_fft}")


# ---- 2. framing seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [16, 64])
def test_framing_seams(n, dtype):
    for k, (label, T, kw, kind, inverse) in enumerate(sc.seam_cases(n)):
        win = sc.window(kind, kw.get("win_length", n))
        re, im = fc.gaussian((3, T), dtype, seed=500 + k)
        check(cplx.stft(re.to(DEV), n, window=dev_win(win), onesided=False, **kw),
              sc.ref_stft(re, n, window=win, onesided=False, **kw), dtype, f"real onesided=False n_fft={n} {label}")
        S = check(cplx.stft(dev_cplx(re, im), n, window=dev_win(win), **kw), ref_cstft(re, im, n, window=win, **kw), dtype,
                  f"Cplx n_fft={n} {label}")
        if inverse:
            xr, xi = fc.gaussian(tuple(S.real.shape), dtype, seed=600 + k)
            ikw = sc.istft_kwargs(kw)
            check(cplx.istft(dev_cplx(xr, xi), n, window=dev_win(win), return_complex=True, **ikw),
                  ref_cistft(xr, xi, n, window=win, **ikw), dtype, f"istft n_fft={n} {label}")
    win = sc.window("hann", n)
    xr, xi = fc.gaussian((2, n, 9), dtype, seed=700)
    natural = (n // 4) * 8
    for length in (natural - 5, natural + n):
        y = check(cplx.istft(dev_cplx(xr, xi), n, n // 4, window=dev_win(win), return_complex=True, length=length),
                  ref_cistft(xr, xi, n, n // 4, window=win, length=length), dtype, f"istft n_fft={n} length={length}")
        if length > natural + n // 2:
            assert bool((y.real[:, natural + n // 2:] == 0).all()) and bool((y.imag[:, natural + n // 2:] == 0).all())


# ---- 3. workgroup seams ------------------------------------------------------------------------------------------------
def test_a_workgroup_spans_two_rows():
    """n_fft = 64 on the complex kernel packs 32 frames per workgroup: 3 rows x 43 frames put workgroup boundaries inside
    rows and leave a partly filled last workgroup"""
    n, hop, frames = 64, 16, 43
    V = hoststft.plan(n, hop, n + (frames - 1) * hop, 3, 1, full=True)["vectors_per_workgroup"]
    assert V == 32 and (3 * frames) % V and frames % V
    win = sc.window("rand", n)
    re, im = fc.gaussian((3, n + (frames - 1) * hop), torch.float32, seed=800)
    S = check(cplx.stft(dev_cplx(re, im), n, hop, window=dev_win(win), center=False),
              ref_cstft(re, im, n, hop, window=win, center=False), torch.float32, "3 rows x 43 frames")
    assert S.real.shape == (3, 64, 43)
    xr, xi = fc.gaussian((3, 64, 43), torch.float32, seed=801)
    check(cplx.istft(dev_cplx(xr, xi), n, hop, window=dev_win(win), center=False, return_complex=True),
          ref_cistft(xr, xi, n, hop, window=win, center=False), torch.float32, "istft 3 rows x 43 frames")


@pytest.mark.parametrize("n", [16, 64, 1024])
def test_frame_counts_around_the_workgroup(n):
    hop = n // 4
    V = hoststft.plan(n, hop, n, 1, 1, full=True)["vectors_per_workgroup"]
    assert V == {16: 128, 64: 32, 1024: 2}[n]
    win = sc.window("rand", n)
    for frames in (V - 1, V, V + 1):
        re, im = fc.gaussian((1, n + (frames - 1) * hop), torch.float32, seed=810 + frames)
        S = check(cplx.stft(dev_cplx(re, im), n, hop, window=dev_win(win), center=False),
                  ref_cstft(re, im, n, hop, window=win, center=False), torch.float32, f"n_fft={n} frames={frames}")
        assert S.real.shape[-1] == frames


# ---- 4. layouts, and the copies that are made ----------------------------------------------------------------------------
def test_layouts_give_identical_bits_and_only_the_documented_copies(monkeypatch):
    calls, copies = [], []
    orig = hoststft.call
    monkeypatch.setattr(hoststft, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    contiguous = torch.Tensor.contiguous

    def counted(self, *a, **k):                           # only a call that copies counts
        if not self.is_contiguous():
            copies.append(tuple(self.shape))
        return contiguous(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "contiguous", counted)
    n, hop, T = 64, 16, 200
    wd = dev_win(sc.window("hann", n))
    re, im = fc.gaussian((2, 3, T), torch.float32, seed=820)
    z = dev_cplx(re, im)
    base = cplx.stft(z, n, hop, window=wd)
    assert calls == ["cplxamd_stft"] and copies == []
    wide_r, wide_i = torch.zeros(2, 3, 2 * T, device=DEV), torch.zeros(2, 3, 2 * T, device=DEV)
    wide_r[..., ::2], wide_i[..., ::2] = z.real, z.imag
    for what, v, ncopies in (("step-sliced planes", Cplx(wide_r[..., ::2], wide_i[..., ::2]), 0),
                             ("planes of two layouts", Cplx(wide_r[..., ::2], z.imag), 1),
                             ("a 1-d signal", Cplx(z.real[1, 2], z.imag[1, 2]), 0)):
        calls.clear(), copies.clear()
        got = cplx.stft(v, n, hop, window=wd)
        want = Cplx(base.real[1, 2], base.imag[1, 2]) if what == "a 1-d signal" else base
        assert calls == ["cplxamd_stft"] and len(copies) == ncopies, (what, calls, copies)
        assert torch.equal(got.real, want.real) and torch.equal(got.imag, want.imag), what
    # a real signal: in place whatever its strides; its spectrum equals that of the pair with a zero plane, to the bit
    calls.clear(), copies.clear()
    full = cplx.stft(wide_r[..., ::2], n, hop, window=wd, onesided=False)
    zero = cplx.stft(Cplx(z.real, torch.zeros_like(z.real)), n, hop, window=wd)
    assert calls == ["cplxamd_stft"] * 2 and copies == []
    assert torch.equal(full.real, zero.real) and torch.equal(full.imag, zero.imag)
    # the one-sided transform of a strided signal makes no copy either
    cplx.stft(wide_r[..., ::2], n, hop, window=wd)
    assert copies == []
    # istft: frames-major (what stft returns) in place; contiguous as [..., N, frames] is the one documented copy per plane
    xr, xi = fc.gaussian((2, 3, n, 9), torch.float32, seed=821)
    fm = lambda t: contiguous(t.to(DEV).transpose(-1, -2)).transpose(-1, -2)    # noqa: E731
    a, b = fm(xr), fm(xi)
    calls.clear(), copies.clear()
    y0 = cplx.istft(Cplx(a, b), n, hop, window=wd, return_complex=True)
    assert calls == ["cplxamd_istft"] and copies == []
    assert a.data_ptr() != 0 and fc.normwise(y0, ref_cistft(xr, xi, n, hop, window=sc.window("hann", n))) <= fc.F32_TOL
    y1 = cplx.istft(dev_cplx(xr, xi), n, hop, window=wd, return_complex=True)
    assert calls == ["cplxamd_istft"] * 2 and len(copies) == 2
    assert torch.equal(y0.real, y1.real) and torch.equal(y0.imag, y1.imag)
    # the same two rules for a half spectrum and a real result
    hr, hi = rc.half_spectrum((2, 3, n // 2 + 1, 9), torch.float32, seed=822)
    copies.clear()
    r0 = cplx.istft(Cplx(fm(hr), fm(hi)), n, hop, window=wd)
    assert copies == []
    r1 = cplx.istft(dev_cplx(hr, hi), n, hop, window=wd)
    assert len(copies) == 2 and torch.equal(r0, r1)


# ---- 5. bf16 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 400, 1024])
def test_bf16_rounds_once(n_fft):
    hop, T, rows = sc.path_geometry(n_fft)
    wf = sc.window("rand", n_fft).float()                   # the window the kernel uses: float32
    re, im = fc.gaussian((rows, T), torch.bfloat16, seed=830 + n_fft)
    got = cplx.stft(dev_cplx(re, im), n_fft, hop, window=wf.to(DEV))
    assert got.real.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(got, ref_cstft(re, im, n_fft, hop, window=wf))
    xr, xi = fc.gaussian((rows, n_fft, got.real.shape[-1]), torch.bfloat16, seed=831 + n_fft)
    back = cplx.istft(dev_cplx(xr, xi), n_fft, hop, window=wf.to(DEV), return_complex=True)
    assert back.real.dtype == torch.bfloat16
    bad_i, worst_i = fc.bf16_violations(back, ref_cistft(xr, xi, n_fft, hop, window=wf))
    print(f"stft_parity full bf16 n_fft={n_fft}: stft {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} "
          f"of the bound; istft {bad_i}, worst at {worst_i:.3f}")
    assert bad == 0 and bad_i == 0


# ---- 6. round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [16, 400, 2048])
def test_round_trip(n_fft, dtype):
    hop = n_fft // 4
    win = dev_win(sc.window("hann", n_fft))
    re, im = fc.gaussian((2, 9 * hop), dtype, seed=840 + n_fft)
    back = cplx.istft(cplx.stft(dev_cplx(re, im), n_fft, hop, window=win), n_fft, hop, window=win, return_complex=True)
    err = fc.normwise(back, fc.c128(re, im))
    print(f"stft_parity full round trip n_fft={n_fft} {dtype}: {err:.3g}")
    assert back.real.shape == re.shape and err <= fc.tol(dtype)


# ---- 7. the adjoint identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 15])
@pytest.mark.parametrize("hop", [1, 5, "n_fft", "n_fft + 4"])
def test_adjoint_identity_in_float64(n_fft, hop):
    hop = {"n_fft": n_fft, "n_fft + 4": n_fft + 4}.get(hop, hop)
    T = 3 * n_fft + 7
    win = sc.window("rand", n_fft)
    for kw in (dict(), dict(pad_mode="constant"), dict(center=False)):
        re, im = fc.gaussian((2, T), torch.float64, seed=850 + hop)
        z = dev_cplx(re, im, True)
        S = cplx.stft(z, n_fft, hop, window=dev_win(win), **kw)
        yr, yi = fc.gaussian(tuple(S.real.shape), torch.float64, seed=851 + hop)
        lhs = (S.real * yr.to(DEV)).sum() + (S.imag * yi.to(DEV)).sum()
        gr, gi = torch.autograd.grad(lhs, (z.real, z.imag))
        rhs = (z.real.detach() * gr).sum() + (z.imag.detach() * gi).sum()
        assert abs(float(lhs) - float(rhs)) <= fc.F64_TOL * max(abs(float(lhs)), float(gr.norm() * z.real.norm())), (kw, lhs, rhs)
        # a real signal with the full spectrum: the gradient is the real plane of the same adjoint, to the bit
        x = z.real.detach().clone().requires_grad_()
        R = cplx.stft(x, n_fft, hop, window=dev_win(win), onesided=False, **kw)
        g, = torch.autograd.grad((R.real * yr.to(DEV)).sum() + (R.imag * yi.to(DEV)).sum(), x)
        assert torch.equal(g, gr), kw
    if hop <= n_fft:
        for kw in (dict(), dict(center=False), dict(length=2 * n_fft + 3), dict(length=5 * n_fft)):
            frames = 9 if hop > 1 else 2 * n_fft
            xr, xi = fc.gaussian((2, n_fft, frames), torch.float64, seed=852 + hop)
            z = dev_cplx(xr, xi, True)
            y = cplx.istft(z, n_fft, hop, window=dev_win(win), return_complex=True, **kw)
            vr, vi = fc.gaussian(tuple(y.real.shape), torch.float64, seed=853)
            lhs = (y.real * vr.to(DEV)).sum() + (y.imag * vi.to(DEV)).sum()
            gr, gi = torch.autograd.grad(lhs, (z.real, z.imag))
            rhs = (z.real.detach() * gr).sum() + (z.imag.detach() * gi).sum()
            assert abs(float(lhs) - float(rhs)) <= fc.F64_TOL * max(abs(float(lhs)), float(y.real.norm() * vr.norm())), (kw, lhs, rhs)


# ---- 8. gradients against torch's CPU float64 autograd of the same expression ------------------------------------------------
def power(re, im, p):
    return ((re.double() ** 2 + im.double() ** 2) ** (p // 2)).sum()


def cstft_graph(a, b, n_fft, hop, win, **kw):
    return torch.stft(torch.complex(a, b), n_fft, hop, None, win, return_complex=True, **kw)


def cistft_graph(a, b, n_fft, hop, win, **kw):
    return torch.istft(torch.complex(a, b), n_fft, hop, None, win, onesided=False, return_complex=True, **kw)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [8, 9, 100, 1024])
def test_first_order_gradients(n_fft, dtype):
    hop = max(1, n_fft // 4)
    win = sc.window("hann", n_fft)
    re, im = fc.gaussian((2, 7 * hop + 3), dtype, seed=860)
    for kw in (dict(), dict(pad_mode="constant", normalized=True), dict(center=False)):
        a, b = re.double().requires_grad_(), im.double().requires_grad_()
        Sc = cstft_graph(a, b, n_fft, hop, win, **kw)
        ref = torch.autograd.grad(power(Sc.real, Sc.imag, 2), (a, b))
        z = dev_cplx(re, im, True)
        S = cplx.stft(z, n_fft, hop, window=dev_win(win), **kw)
        got = torch.autograd.grad(power(S.real, S.imag, 2), (z.real, z.imag))
        assert got[0].dtype == dtype and got[1].shape == im.shape
        e_s = fc.normwise(fc.c128(*got), torch.complex(*ref))
        # a real signal, full spectrum
        xc = re.double().requires_grad_()
        Rc = torch.stft(xc, n_fft, hop, None, win, return_complex=True, onesided=False, **kw)
        rref, = torch.autograd.grad(power(Rc.real, Rc.imag, 2), xc)
        xg = re.to(DEV).requires_grad_()
        R = cplx.stft(xg, n_fft, hop, window=dev_win(win), onesided=False, **kw)
        rgot, = torch.autograd.grad(power(R.real, R.imag, 2), xg)
        e_r = rc.real_normwise(rgot, rref)
        print(f"stft_parity full gradients n_fft={n_fft} {dtype} {kw}: stft Cplx {e_s:.3g} real {e_r:.3g}")
        assert e_s <= fc.tol(dtype) and e_r <= fc.tol(dtype), (kw, e_s, e_r)
    xr, xi = fc.gaussian((2, n_fft, 9), dtype, seed=861)
    for kw in (dict(), dict(normalized=True, length=6 * hop + 1), dict(length=9 * hop + n_fft)):
        a, b = xr.double().requires_grad_(), xi.double().requires_grad_()
        yc = cistft_graph(a, b, n_fft, hop, win, **kw)
        w = rc.real_gaussian(tuple(yc.shape), torch.float64, seed=862)
        ref = torch.autograd.grad(((yc.real ** 2 + 2 * yc.imag ** 2) * w).sum(), (a, b))
        z = dev_cplx(xr, xi, True)
        y = cplx.istft(z, n_fft, hop, window=dev_win(win), return_complex=True, **kw)
        got = torch.autograd.grad(((y.real.double() ** 2 + 2 * y.imag.double() ** 2) * w.to(DEV)).sum(), (z.real, z.imag))
        e_i = fc.normwise(fc.c128(*got), torch.complex(*ref))
        print(f"stft_parity full gradients n_fft={n_fft} {dtype} {kw}: istft {e_i:.3g}")
        assert e_i <= fc.tol(dtype), (kw, e_i)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [8, 100])
def test_hessian_vector_products(n_fft, dtype):
    hop = n_fft // 4
    win = sc.window("hann", n_fft)
    re, im = fc.gaussian((2, 7 * hop + 3), dtype, seed=870)
    vr, vi = fc.gaussian((2, 7 * hop + 3), torch.float64, seed=871)

    def hvp(fn, a, b, va, vb):
        S = fn(a, b)
        g = torch.autograd.grad(power(S.real, S.imag, 4), (a, b), create_graph=True)
        return torch.autograd.grad((g[0].double() * va).sum() + (g[1].double() * vb).sum(), (a, b))

    ref = hvp(lambda a, b: cstft_graph(a, b, n_fft, hop, win), re.double().requires_grad_(), im.double().requires_grad_(), vr, vi)
    got = hvp(lambda a, b: cplx.stft(Cplx(a, b), n_fft, hop, window=dev_win(win)), re.to(DEV).requires_grad_(),
              im.to(DEV).requires_grad_(), vr.to(DEV), vi.to(DEV))
    e_s = fc.normwise(fc.c128(*got), torch.complex(*ref))
    xr, xi = fc.gaussian((2, n_fft, 9), dtype, seed=872)
    wr, wi = fc.gaussian((2, n_fft, 9), torch.float64, seed=873)
    ref = hvp(lambda a, b: cistft_graph(a, b, n_fft, hop, win), xr.double().requires_grad_(), xi.double().requires_grad_(), wr, wi)
    got = hvp(lambda a, b: cplx.istft(Cplx(a, b), n_fft, hop, window=dev_win(win), return_complex=True),
              xr.to(DEV).requires_grad_(), xi.to(DEV).requires_grad_(), wr.to(DEV), wi.to(DEV))
    e_i = fc.normwise(fc.c128(*got), torch.complex(*ref))
    print(f"stft_parity full second order n_fft={n_fft} {dtype}: stft {e_s:.3g} istft {e_i:.3g}")
    assert e_s <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_s, e_i)


# ---- 9. reruns and capture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [100, 2048, 8194])
def test_reruns_are_bit_identical(n_fft):
    hop, T, rows = sc.path_geometry(n_fft)
    wd = dev_win(sc.window("rand", n_fft))
    z = dev_cplx(*fc.gaussian((rows, T), torch.float32, seed=880 + n_fft))
    a, b = cplx.stft(z, n_fft, hop, window=wd), cplx.stft(z, n_fft, hop, window=wd)
    assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)
    ya, yb = (cplx.istft(s, n_fft, hop, window=wd, return_complex=True) for s in (a, b))
    assert torch.equal(ya.real, yb.real) and torch.equal(ya.imag, yb.imag)


def test_graph_replay_equals_eager():
    n, hop = 200, 50
    wd = sc.window("hann", n).float().to(DEV)

    def step(re, im):
        S = cplx.stft(Cplx(re, im), n, hop, window=wd)
        back = cplx.istft(Cplx(S.real * 0.5, S.imag), n, hop, window=wd, return_complex=True, check_nola=False)
        g = torch.autograd.grad((back.real.float() ** 2).sum() + (back.imag.float() ** 2).sum(), (re, im))
        return (S.real, S.imag, back.real, back.imag) + g

    re0, im0 = fc.gaussian((4, 3, 1000), torch.bfloat16, seed=890)
    sr, si = re0.to(DEV).requires_grad_(), im0.to(DEV).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sr, si)                                      # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sr, si)
    re, im = fc.gaussian((4, 3, 1000), torch.bfloat16, seed=891)
    with torch.no_grad():
        sr.copy_(re), si.copy_(im)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(re.to(DEV).requires_grad_(), im.to(DEV).requires_grad_())
    for o, e in zip(outs, eager):
        assert o.dtype == torch.bfloat16 and torch.equal(o, e)


# ---- 10. errors and empty batches ------------------------------------------------------------------------------------------
def test_errors_and_empty_batches():
    z = lambda *shape, **kw: torch.zeros(*shape, device=DEV, **kw)      # noqa: E731
    with pytest.raises(RuntimeError, match="onesided") as e:
        cplx.stft(Cplx(z(4, 64), z(4, 64)), 16, onesided=True)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(RuntimeError, match="onesided") as e:
        cplx.istft(Cplx(z(4, 9, 5), z(4, 9, 5)), 16, return_complex=True)
    assert not isinstance(e.value, CplxAmdError)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.stft(Cplx(z(4, 64), z(4, 64, dtype=torch.float64)), 16)
    with pytest.raises(CplxAmdError, match="different devices|no CPU path"):
        cplx.stft(Cplx(z(4, 64), torch.zeros(4, 64)), 16)
    # zero rows in every pad mode, real and Cplx: empty results without a launch, and gradients of the right shape
    for mode in hoststft.PAD_MODES:
        empty = z(0, 64, requires_grad=True)
        out = cplx.stft(empty, 16, pad_mode=mode)
        assert out.real.shape == (0, 9, 17), mode
        (out.real.sum() + out.imag.sum()).backward()
        assert empty.grad.shape == (0, 64)
        ez = Cplx(z(2, 0, 64, requires_grad=True), z(2, 0, 64, requires_grad=True))
        out = cplx.stft(ez, 16, pad_mode=mode)
        assert out.real.shape == (2, 0, 16, 17) and out.imag.shape == (2, 0, 16, 17), mode
        (out.real.sum() + out.imag.sum()).backward()
        assert ez.real.grad.shape == (2, 0, 64) and ez.imag.grad.shape == (2, 0, 64)
    es = Cplx(z(0, 16, 17, requires_grad=True), z(0, 16, 17, requires_grad=True))
    back = cplx.istft(es, 16, return_complex=True)
    assert back.real.shape == (0, 64) and back.imag.shape == (0, 64)
    (back.real.sum() + back.imag.sum()).backward()
    assert es.real.grad.shape == (0, 16, 17)
