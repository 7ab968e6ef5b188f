"""cplx.stft / istft on the GPU (csrc/stft.hip through cplxmodule_amd/stft.py): every path of the underlying real transform
against float64, the framing, padding and workgroup seams, layout independence in one launch each, the single rounding of
bf16, the round trip, the adjoint identity that pins the fold, gradients of first and second order against torch's CPU
autograd, bit-identical reruns, hipGraph replay, NOLA and the errors raised on the device.  Cases: stft_cases.py;
reference (torch.stft / torch.istft in float64 / complex128 on the CPU) and bounds: fft_cases.py."""
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


def dev_win(win, dtype=None):
    return None if win is None else (win if dtype is None else win.to(dtype)).to(DEV)


def dev_cplx(re, im, requires_grad=False):
    return Cplx(re.to(DEV).requires_grad_(requires_grad), im.to(DEV).requires_grad_(requires_grad))


def check_stft(x, n_fft, win, dtype, what, **kw):
    """cplx.stft of x (CPU, dtype) against torch.stft in float64 of the same values, at the dtype's bound"""
    got = cplx.stft(x.to(DEV), n_fft, window=dev_win(win), **kw)
    ref = sc.ref_stft(x, n_fft, window=win, **kw)
    assert got.real.dtype == dtype and got.imag.dtype == dtype and tuple(got.real.shape) == tuple(ref.shape), what
    # torch's memory order: dense as [..., frames, N]
    assert got.real.transpose(-1, -2).is_contiguous() and got.imag.transpose(-1, -2).is_contiguous(), what
    err = fc.normwise(got, ref)
    print(f"stft_parity stft {what} {dtype}: {err:.3g}")
    assert err <= fc.tol(dtype), (what, err)
    return got


def check_istft(xr, xi, n_fft, win, dtype, what, **kw):
    got = cplx.istft(dev_cplx(xr, xi), n_fft, window=dev_win(win), **kw)
    ref = sc.ref_istft(xr, xi, n_fft, window=win, **kw)
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), what
    err = rc.real_normwise(got, ref)
    print(f"stft_parity istft {what} {dtype}: {err:.3g}")
    assert err <= fc.tol(dtype), (what, err)
    return got


# ---- 1. every path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", sc.PATH_LENGTHS)
def test_every_path(n_fft, dtype):
    x, win, S, xr, xi, y = sc.path_case(n_fft, dtype)
    hop = sc.path_geometry(n_fft)[0]
    got = cplx.stft(x.to(DEV), n_fft, hop, window=dev_win(win))
    assert got.real.dtype == dtype and tuple(got.real.shape) == tuple(S.shape)
    e_s = fc.normwise(got, S)
    back = cplx.istft(dev_cplx(xr, xi), n_fft, hop, window=dev_win(win), onesided=True)
    assert back.dtype == dtype and tuple(back.shape) == tuple(y.shape)
    e_i = rc.real_normwise(back, y)
    print(f"stft_parity every path n_fft={n_fft} {dtype}: stft {e_s:.3g} istft {e_i:.3g}")
    assert e_s <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_s, e_i)
    # the imaginary parts of DC and (even n_fft) Nyquist are stored as exact zeros
    assert bool((got.imag[:, 0] == 0).all())
    if n_fft % 2 == 0:
        assert bool((got.imag[:, n_fft // 2] == 0).all())


# ---- 2. framing seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n", [16, 64])
def test_framing_seams(n, dtype):
    for k, (label, T, kw, kind, inverse) in enumerate(sc.seam_cases(n)):
        win = sc.window(kind, kw.get("win_length", n))
        x = rc.real_gaussian((3, T), dtype, seed=100 + k)
        S = check_stft(x, n, win, dtype, f"n_fft={n} {label}", **kw)
        if inverse:
            xr, xi = rc.half_spectrum(tuple(S.real.shape), dtype, seed=200 + k)
            check_istft(xr, xi, n, win, dtype, f"n_fft={n} {label}", **sc.istft_kwargs(kw))
    # `length` shorter and longer than the frames give: trimmed, and zero-extended with exact zeros
    win = sc.window("hann", n)
    xr, xi = rc.half_spectrum((2, n // 2 + 1, 9), dtype, seed=300)
    natural = (n // 4) * 8
    for length in (natural - 5, natural + 1, natural + n):
        y = check_istft(xr, xi, n, win, dtype, f"n_fft={n} length={length}", hop_length=n // 4, length=length)
        if length > natural + n // 2:
            assert bool((y[:, natural + n // 2:] == 0).all())


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
def test_a_real_result_from_a_full_spectrum_reads_its_first_half(dtype):
    """onesided=False with return_complex=False: torch slices the first n_fft / 2 + 1 bins, and so does istft (a view)"""
    n, hop = 16, 4
    win = sc.window("hann", n)
    xr, xi = rc.half_spectrum((3, n, 9), dtype, seed=310)              # no Hermitian symmetry: the upper half is ignored
    for kw in (dict(), dict(onesided=False), dict(onesided=False, length=30)):
        check_istft(xr, xi, n, win, dtype, f"full spectrum {kw}", hop_length=hop, **kw)


# ---- 3. workgroup seams ------------------------------------------------------------------------------------------------
def test_a_workgroup_spans_two_rows():
    """n_fft = 64 packs 64 frames per workgroup: 3 rows x 43 frames are two full workgroups plus one frame, and both
    workgroup boundaries fall inside a row"""
    n, hop, frames = 64, 16, 43
    assert hoststft.plan(n, hop, n + (frames - 1) * hop, 3, 1)["vectors_per_workgroup"] == 64
    win = sc.window("rand", n)
    x = rc.real_gaussian((3, n + (frames - 1) * hop), torch.float32, seed=60)
    S = check_stft(x, n, win, torch.float32, "3 rows x 43 frames", hop_length=hop, center=False)
    assert S.real.shape == (3, 33, 43)
    xr, xi = rc.half_spectrum((3, 33, 43), torch.float32, seed=61)
    check_istft(xr, xi, n, win, torch.float32, "3 rows x 43 frames", hop_length=hop, center=False)


@pytest.mark.parametrize("n", [16, 64, 2048])
def test_frame_counts_around_the_workgroup(n):
    hop = n // 4
    V = hoststft.plan(n, hop, n, 1, 1)["vectors_per_workgroup"]
    assert V == {16: 256, 64: 64, 2048: 2}[n]
    win = sc.window("rand", n)
    for frames in (V - 1, V, V + 1):
        x = rc.real_gaussian((1, n + (frames - 1) * hop), torch.float32, seed=70 + frames)
        S = check_stft(x, n, win, torch.float32, f"n_fft={n} frames={frames}", hop_length=hop, center=False)
        assert S.real.shape[-1] == frames
        xr, xi = rc.half_spectrum((1, n // 2 + 1, frames), torch.float32, seed=71 + frames)
        check_istft(xr, xi, n, win, torch.float32, f"n_fft={n} frames={frames}", hop_length=hop, center=False)


# ---- 4. layouts ----------------------------------------------------------------------------------------------------------
def test_layouts_give_identical_bits_in_one_launch_each(monkeypatch):
    calls = []
    orig = hoststft.call
    monkeypatch.setattr(hoststft, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    n, hop, T = 64, 16, 200
    win = sc.window("hann", n)
    wd = dev_win(win)
    x = rc.real_gaussian((2, 3, T), torch.float32, seed=80)
    ref = sc.ref_stft(x, n, hop, window=win)
    xd = x.to(DEV)
    base = cplx.stft(xd, n, hop, window=wd)
    assert calls == ["cplxamd_stft"] and fc.normwise(base, ref) <= fc.F32_TOL
    wide = torch.zeros(2, 3, 2 * T, device=DEV)
    wide[..., ::2] = xd
    tall = torch.zeros(2, 6, T, device=DEV)
    tall[:, ::2] = xd
    gap = torch.zeros(2, 4, T, device=DEV)
    gap[:, :3] = xd
    # (rows that are no single run are the documented copy: still one launch, the same bits)
    for what, v in (("a step-sliced signal", wide[..., ::2]), ("sliced rows", tall[:, ::2]), ("rows that are no single run", gap[:, :3]),
                    ("a float32 window", None), ("a 1-d signal", None), ("an expanded row", None)):
        calls.clear()
        if what == "a float32 window":
            got, want = cplx.stft(xd, n, hop, window=win.float().to(DEV)), base
        elif what == "a 1-d signal":
            got, want = cplx.stft(xd[1, 2], n, hop, window=wd), Cplx(base.real[1, 2], base.imag[1, 2])
            assert got.real.shape == (33, ref.shape[-1])
        elif what == "an expanded row":
            got = cplx.stft(xd[0, 1].expand(4, T), n, hop, window=wd)
            want = Cplx(base.real[0, 1].expand(4, -1, -1), base.imag[0, 1].expand(4, -1, -1))
        else:
            assert not v.is_contiguous()
            got, want = cplx.stft(v, n, hop, window=wd), base
        assert calls == ["cplxamd_stft"], (what, calls)
        assert torch.equal(got.real, want.real) and torch.equal(got.imag, want.imag), what
    # istft: torch's frames-major order (what stft returns), [..., N, frames]-contiguous, and planes of different layouts
    xr, xi = rc.half_spectrum((2, 3, 33, 9), torch.float32, seed=81)
    yref = sc.ref_istft(xr, xi, n, hop, window=win)
    fm = lambda t: t.to(DEV).transpose(-1, -2).contiguous().transpose(-1, -2)    # noqa: E731
    calls.clear()
    y0 = cplx.istft(Cplx(fm(xr), fm(xi)), n, hop, window=wd)
    assert calls == ["cplxamd_istft"] and rc.real_normwise(y0, yref) <= fc.F32_TOL
    for what, z in (("contiguous as [..., N, frames]", dev_cplx(xr, xi)), ("planes of two layouts", Cplx(fm(xr), xi.to(DEV))),
                    ("a 2-d spectrogram", None)):
        calls.clear()
        if z is None:
            got, want = cplx.istft(Cplx(fm(xr)[1, 0], fm(xi)[1, 0]), n, hop, window=wd), y0[1, 0]
        else:
            got, want = cplx.istft(z, n, hop, window=wd), y0
        assert calls == ["cplxamd_istft"], (what, calls)
        assert torch.equal(got, want), what


# ---- 5. bf16 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 400, 1024])
def test_bf16_rounds_once(n_fft):
    x, win, _, xr, xi, _ = sc.path_case(n_fft, torch.bfloat16)
    hop = sc.path_geometry(n_fft)[0]
    wf = win.float()                                        # the window the kernel uses: float32
    got = cplx.stft(x.to(DEV), n_fft, hop, window=wf.to(DEV))
    assert got.real.dtype == torch.bfloat16
    bad, worst = fc.bf16_violations(got, sc.ref_stft(x, n_fft, hop, window=wf))
    back = cplx.istft(dev_cplx(xr, xi), n_fft, hop, window=wf.to(DEV))
    assert back.dtype == torch.bfloat16
    bad_i, worst_i = rc.bf16_real_violations(back, sc.ref_istft(xr, xi, n_fft, hop, window=wf))
    print(f"stft_parity bf16 n_fft={n_fft}: stft {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f} of "
          f"the bound; istft {bad_i}, worst at {worst_i:.3f}")
    assert bad == 0 and bad_i == 0


# ---- 6. round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [16, 400, 2048])
def test_round_trip(n_fft, dtype):
    hop = n_fft // 4
    win = dev_win(sc.window("hann", n_fft))
    x = rc.real_gaussian((2, 9 * hop), dtype, seed=90 + n_fft)
    back = cplx.istft(cplx.stft(x.to(DEV), n_fft, hop, window=win), n_fft, hop, window=win)
    err = rc.real_normwise(back, x.double())
    print(f"stft_parity round trip n_fft={n_fft} {dtype}: {err:.3g}")
    assert back.shape == x.shape and err <= fc.tol(dtype)
    back = cplx.istft(cplx.stft(x.to(DEV), n_fft, hop, window=win, normalized=True), n_fft, hop, window=win, normalized=True,
                      length=x.shape[-1] - 3)
    assert rc.real_normwise(back, x.double()[:, :-3]) <= fc.tol(dtype)


# ---- 7. the adjoint identity: <stft(x), Y> = <x, grad>, the narrow test of the fold ----------------------------------------
@pytest.mark.parametrize("n_fft", [16, 15])
@pytest.mark.parametrize("hop", [1, 5, "n_fft", "n_fft + 4"])
def test_adjoint_identity_in_float64(n_fft, hop):
    hop = {"n_fft": n_fft, "n_fft + 4": n_fft + 4}.get(hop, hop)
    T = 3 * n_fft + 7
    win = sc.window("rand", n_fft)
    for kw in (dict(), dict(pad_mode="constant"), dict(center=False), dict(pad_mode="replicate")):
        x = rc.real_gaussian((2, T), torch.float64, seed=110 + hop)
        xd = x.to(DEV).requires_grad_()
        S = cplx.stft(xd, n_fft, hop, window=dev_win(win), **kw)
        yr, yi = fc.gaussian(tuple(S.real.shape), torch.float64, seed=111 + hop)
        lhs = (S.real * yr.to(DEV)).sum() + (S.imag * yi.to(DEV)).sum()
        g, = torch.autograd.grad(lhs, xd)
        rhs = (xd.detach() * g).sum()
        assert abs(float(lhs) - float(rhs)) <= fc.F64_TOL * max(abs(float(lhs)), float(g.norm() * xd.norm())), (kw, lhs, rhs)
        # and the gradient itself is torch's
        xc = x.clone().requires_grad_()
        Sc = sc.ref_stft_graph(xc, n_fft, hop, win, **kw)
        gref, = torch.autograd.grad((Sc.real * yr).sum() + (Sc.imag * yi).sum(), xc)
        assert rc.real_normwise(g, gref) <= fc.F64_TOL, kw
    if hop > n_fft:
        # the samples no frame covers: an exact zero gradient
        xd = rc.real_gaussian((1, 4 * hop), torch.float64, seed=5).to(DEV).requires_grad_()
        S = cplx.stft(xd, n_fft, hop, window=dev_win(win), center=False)
        g, = torch.autograd.grad((S.real ** 2).sum() + (S.imag ** 2).sum(), xd)
        for f in range(S.real.shape[-1] - 1):
            assert bool((g[0, f * hop + n_fft:(f + 1) * hop] == 0).all())
    if hop <= n_fft:
        for kw in (dict(), dict(center=False), dict(length=2 * n_fft + 3), dict(length=5 * n_fft)):
            frames = 9 if hop > 1 else 2 * n_fft
            xr, xi = fc.gaussian((2, n_fft // 2 + 1, frames), torch.float64, seed=112 + hop)
            z = dev_cplx(xr, xi, True)
            y = cplx.istft(z, n_fft, hop, window=dev_win(win), **kw)
            v = rc.real_gaussian(tuple(y.shape), torch.float64, seed=113).to(DEV)
            lhs = (y * v).sum()
            gr, gi = torch.autograd.grad(lhs, (z.real, z.imag))
            # Im X_0 and (even n_fft) Im X_n/2 do not enter: the pairing runs over what does
            rhs = (z.real.detach() * gr).sum() + (z.imag.detach() * gi).sum()
            assert abs(float(lhs) - float(rhs)) <= fc.F64_TOL * max(abs(float(lhs)), float(y.norm() * v.norm())), (kw, lhs, rhs)
            assert bool((gi[:, 0] == 0).all())


# ---- 8. gradients against torch's CPU float64 autograd of the same expression ------------------------------------------------
def stft_loss(S, power):
    return ((S.real.double() ** 2 + S.imag.double() ** 2) ** (power // 2)).sum()


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [8, 9, 100, 1024])
def test_first_order_gradients(n_fft, dtype):
    hop = max(1, n_fft // 4)
    win = sc.window("hann", n_fft)
    x = rc.real_gaussian((2, 3, 7 * hop + 3), dtype, seed=120)
    for kw in (dict(), dict(pad_mode="constant", normalized=True), dict(center=False)):
        xc = x.double().requires_grad_()
        ref, = torch.autograd.grad(stft_loss(sc.ref_stft_graph(xc, n_fft, hop, win, **kw), 2), xc)
        xg = x.to(DEV).requires_grad_()
        got, = torch.autograd.grad(stft_loss(cplx.stft(xg, n_fft, hop, window=dev_win(win), **kw), 2), xg)
        assert got.dtype == dtype and got.shape == x.shape
        e_s = rc.real_normwise(got, ref)
        print(f"stft_parity gradients n_fft={n_fft} {dtype} {kw}: stft {e_s:.3g}")
        assert e_s <= fc.tol(dtype), (kw, e_s)
    re, im = rc.half_spectrum((2, 3, n_fft // 2 + 1, 9), dtype, seed=121)
    for kw in (dict(), dict(normalized=True, length=6 * hop + 1), dict(length=9 * hop + n_fft)):
        a, b = re.double().requires_grad_(), im.double().requires_grad_()
        yc = sc.ref_istft_graph(a, b, n_fft, hop, win, **kw)
        w = rc.real_gaussian(tuple(yc.shape), torch.float64, seed=122)
        ref = torch.autograd.grad(((yc ** 2) * w).sum(), (a, b))
        z = dev_cplx(re, im, True)
        y = cplx.istft(z, n_fft, hop, window=dev_win(win), **kw)
        got = torch.autograd.grad(((y.double() ** 2) * w.to(DEV)).sum(), (z.real, z.imag))
        assert got[0].dtype == dtype and got[0].shape == re.shape
        e_i = fc.normwise(torch.complex(got[0].double().cpu(), got[1].double().cpu()), torch.complex(ref[0], ref[1]))
        print(f"stft_parity gradients n_fft={n_fft} {dtype} {kw}: istft {e_i:.3g}")
        assert e_i <= fc.tol(dtype), (kw, e_i)


@pytest.mark.parametrize("dtype", WIDE, ids=WIDE_IDS)
@pytest.mark.parametrize("n_fft", [8, 100])
def test_hessian_vector_products(n_fft, dtype):
    """d <d sum|S|^4 / dx, v> / dx for S = stft(x), and the same for sum w y^4 with y = istft(X)"""
    hop = n_fft // 4
    win = sc.window("hann", n_fft)
    x = rc.real_gaussian((2, 7 * hop + 3), dtype, seed=130)
    v = rc.real_gaussian((2, 7 * hop + 3), torch.float64, seed=131)

    def hvp(fn, t, vec):
        g, = torch.autograd.grad(stft_loss(fn(t), 4), t, create_graph=True)
        return torch.autograd.grad((g.double() * vec).sum(), t)[0]

    ref = hvp(lambda t: sc.ref_stft_graph(t, n_fft, hop, win), x.double().requires_grad_(), v)
    got = hvp(lambda t: cplx.stft(t, n_fft, hop, window=dev_win(win)), x.to(DEV).requires_grad_(), v.to(DEV))
    e_s = rc.real_normwise(got, ref)
    re, im = rc.half_spectrum((2, n_fft // 2 + 1, 9), dtype, seed=132)
    vr, vi = fc.gaussian((2, n_fft // 2 + 1, 9), torch.float64, seed=133)
    w = rc.real_gaussian((2, 8 * hop), torch.float64, seed=134)

    def hvp2(fn, a, b, va, vb, weight):
        g = torch.autograd.grad(((fn(a, b).double() ** 4) * weight).sum(), (a, b), create_graph=True)
        return torch.autograd.grad((g[0].double() * va).sum() + (g[1].double() * vb).sum(), (a, b))

    ref = hvp2(lambda a, b: sc.ref_istft_graph(a, b, n_fft, hop, win), re.double().requires_grad_(), im.double().requires_grad_(),
               vr, vi, w)
    got = hvp2(lambda a, b: cplx.istft(Cplx(a, b), n_fft, hop, window=dev_win(win)), re.to(DEV).requires_grad_(),
               im.to(DEV).requires_grad_(), vr.to(DEV), vi.to(DEV), w.to(DEV))
    e_i = fc.normwise(torch.complex(got[0].double().cpu(), got[1].double().cpu()), torch.complex(ref[0], ref[1]))
    print(f"stft_parity second order n_fft={n_fft} {dtype}: stft {e_s:.3g} istft {e_i:.3g}")
    assert e_s <= fc.tol(dtype) and e_i <= fc.tol(dtype), (e_s, e_i)


# ---- 9. reruns and capture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [100, 2048, 8194])
def test_reruns_are_bit_identical(n_fft):
    x, win, _, xr, xi, _ = sc.path_case(n_fft, torch.float32)
    hop = sc.path_geometry(n_fft)[0]
    xd, z, wd = x.to(DEV), dev_cplx(xr, xi), dev_win(win)
    a, b = cplx.stft(xd, n_fft, hop, window=wd), cplx.stft(xd, n_fft, hop, window=wd)
    assert torch.equal(a.real, b.real) and torch.equal(a.imag, b.imag)
    assert torch.equal(cplx.istft(z, n_fft, hop, window=wd), cplx.istft(z, n_fft, hop, window=wd))
    assert torch.equal(cplx.istft(a, n_fft, hop, window=wd), cplx.istft(b, n_fft, hop, window=wd))


def test_graph_replay_equals_eager():
    n, hop = 200, 50
    wd = dev_win(sc.window("hann", n), torch.float32)

    def step(x):
        S = cplx.stft(x, n, hop, window=wd)
        back = cplx.istft(Cplx(S.real * 0.5, S.imag), n, hop, window=wd, check_nola=False)
        g, = torch.autograd.grad((back.float() ** 2).sum(), x)
        return S.real, S.imag, back, g

    x0 = rc.real_gaussian((4, 3, 1000), torch.bfloat16, seed=140)
    sx = x0.to(DEV).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx)                                          # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx)
    for seed in (141, 142):
        x = rc.real_gaussian((4, 3, 1000), torch.bfloat16, seed=seed)
        with torch.no_grad():
            sx.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(x.to(DEV).requires_grad_())
        for o, e in zip(outs, eager):
            assert o.dtype == torch.bfloat16 and torch.equal(o, e)


def test_the_nola_check_cannot_run_inside_a_capture():
    wd = dev_win(sc.window("hann", 64), torch.float32)
    z = dev_cplx(*rc.half_spectrum((2, 33, 9), torch.float32, seed=150))
    cplx.istft(z, 64, 16, window=wd)                      # warm-up: allocations outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(CplxAmdError, match="check_nola=False"):
            cplx.istft(z, 64, 16, window=wd)
        out = cplx.istft(z, 64, 16, window=wd, check_nola=False)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, cplx.istft(z, 64, 16, window=wd))


# ---- 10. errors ----------------------------------------------------------------------------------------------------------
def test_nola(monkeypatch):
    n = 64
    hann = sc.window("hann", n)
    xr, xi = rc.half_spectrum((2, 33, 5), torch.float32, seed=160)
    with pytest.raises(RuntimeError):                     # Hann's first sample is 0 and with hop = n_fft nothing overlaps it
        sc.ref_istft(xr, xi, n, n, window=hann)
    with pytest.raises(RuntimeError, match="window overlap add min") as e:
        cplx.istft(dev_cplx(xr, xi), n, n, window=dev_win(hann))
    assert not isinstance(e.value, CplxAmdError)
    # without the check nothing is read on the host: no .item(), no float(), no sync
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (_ for _ in ()).throw(AssertionError("a device value was read")))
    monkeypatch.setattr(torch.Tensor, "__float__", lambda self: (_ for _ in ()).throw(AssertionError("a device value was read")))
    y = cplx.istft(dev_cplx(xr, xi), n, n, window=dev_win(hann), check_nola=False)
    monkeypatch.undo()
    assert y.shape == (2, 4 * n) and not bool(torch.isfinite(y).all())      # 0 / 0 where the envelope is 0, as torch's result


def test_device_errors_and_empty_batches():
    z = lambda *shape, **kw: torch.zeros(*shape, device=DEV, **kw)      # noqa: E731
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.istft(Cplx(z(4, 9, 5), z(4, 9, 5, dtype=torch.bfloat16)), 16)
    with pytest.raises(CplxAmdError, match="float32, bfloat16 or float64"):
        cplx.stft(z(4, 64, dtype=torch.float16), 16)
    with pytest.raises(CplxAmdError, match="not a real torch.Tensor"):
        cplx.stft(z(4, 64, dtype=torch.complex64), 16)
    with pytest.raises(CplxAmdError, match="not a Cplx"):
        cplx.istft(z(4, 9, 5), 16)
    with pytest.raises(CplxAmdError, match="different devices|no CPU path"):
        cplx.istft(Cplx(z(4, 9, 5), torch.zeros(4, 9, 5)), 16)
    with pytest.raises(CplxAmdError, match="different devices|no CPU path"):
        cplx.stft(z(4, 64), 16, window=torch.ones(16))
    with pytest.raises(CplxAmdError, match="must be a real floating tensor"):
        cplx.stft(z(4, 64), 16, window=z(16, dtype=torch.complex64))
    with pytest.raises(CplxAmdError, match="requires grad"):
        cplx.stft(z(4, 64), 16, window=torch.ones(16, device=DEV, requires_grad=True))
    with pytest.raises(CplxAmdError, match="requires grad"):
        cplx.istft(Cplx(z(4, 9, 5), z(4, 9, 5)), 16, window=torch.ones(16, device=DEV, requires_grad=True))
    # argument errors keep torch's type on the device too
    with pytest.raises(RuntimeError) as e:
        cplx.stft(z(4, 8), 16)
    assert not isinstance(e.value, CplxAmdError)
    empty = z(0, 64, requires_grad=True)
    out = cplx.stft(empty, 16)
    assert out.real.shape == (0, 9, 17) and out.imag.shape == (0, 9, 17)
    (out.real.sum() + out.imag.sum()).backward()
    assert empty.grad.shape == (0, 64)
    ez = Cplx(z(0, 9, 17, requires_grad=True), z(0, 9, 17, requires_grad=True))
    back = cplx.istft(ez, 16)
    assert back.shape == (0, 64)
    back.sum().backward()
    assert ez.real.grad.shape == (0, 9, 17) and ez.imag.grad.shape == (0, 9, 17)
    assert cplx.stft(z(2, 0, 64), 16).real.shape == (2, 0, 9, 17)
