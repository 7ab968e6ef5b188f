"""cplx.filtfilt / cplx.sosfiltfilt on the GPU (csrc/filtfilt.hip through cplxmodule_amd/filtfilt.py): bit-exact on integer
operands (every padtype and dtype, the chunk and tile seams of the extended row, explicit padlens, an extension longer
than a tile, the forced split path on both passes), Gaussian data against the complex128 oracle and scipy's recorded
outputs, the routes (two launches, operands read in place, one workspace, the composed routes), gradcheck and
gradgradcheck, bit-identical reruns, hipGraph replay, empty inputs and errors.  Cases, oracle and bounds:
filtfilt_cases.py (whose headroom test_filtfilt_host.py asserts on the very data used here)."""

import numpy as np
import pytest
import torch

import fft_cases as fc
import filtfilt_cases as ff
import iir_cases as ic
from gpu_util import DEV

from cplxmodule_amd import Cplx, cplx
from cplxmodule_amd import filtfilt as hostff
from cplxmodule_amd import iir as hostiir
from cplxmodule_amd._lib import CplxAmdError

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
IDS = ["f32", "bf16", "f64"]
KINDS = {"cc": (True, True), "rc": (False, True), "cr": (True, False), "rr": (False, False)}
EXACT = [("ba", n) for n in ff.EXACT_FILTERS] + [("sos", n) for n in ff.EXACT_CASCADES]
GC = dict(eps=1e-6, atol=1e-7, rtol=1e-6)
PASS = "cplxamd_filtfilt_pass"


def dev(z, dtype, real=False, grad=False):
    """a numpy complex array -> a Cplx (or, `real`, the real plane as a tensor) on the device, rounded to dtype"""
    z = np.asarray(z, dtype=np.complex128)
    re = torch.from_numpy(z.real.copy()).to(dtype).to(DEV).requires_grad_(grad)
    return re if real else Cplx(re, torch.from_numpy(z.imag.copy()).to(dtype).to(DEV).requires_grad_(grad))


def rounded(z, dtype):
    """the values the kernel is given: complex128 of the planes rounded to dtype"""
    z = np.asarray(z, dtype=np.complex128)
    q = lambda p: torch.from_numpy(p.copy()).to(dtype).double().numpy()        # noqa: E731
    return q(z.real) + 1j * q(z.imag)


def planes(y):
    return (y, None) if torch.is_tensor(y) else (y.real, y.imag)


def c128(y):
    yr, yi = planes(y)
    return torch.complex(yr.detach().double().cpu(), torch.zeros_like(yr).double().cpu() if yi is None else yi.detach().double().cpu())


def assert_equal(got, ref, dtype, what=""):
    """`got` (Cplx or real tensor) EQUALS the complex128 numpy reference rounded once to dtype"""
    gr, gi = planes(got)
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert gr.dtype == dtype and gr.shape == ref.shape, (what, gr.shape, ref.shape)
    assert float(max(ref.real.abs().max(), ref.imag.abs().max())) < 2 ** (53 if dtype == torch.float64 else 24), what
    assert torch.equal(gr.double().cpu(), ref.real.to(dtype).double()), f"real plane {what}"
    if gi is None:
        assert not bool(ref.imag.any()), what
    else:
        assert torch.equal(gi.double().cpu(), ref.imag.to(dtype).double()), f"imaginary plane {what}"


def error(got, ref):
    return fc.normwise(c128(got), torch.from_numpy(np.ascontiguousarray(ref)))


def same_bits(p, q):
    return all(torch.equal(u, v) for u, v in zip(planes(p), planes(q)) if u is not None)


def run_exact(kind, name, x, dtype, padtype, padlen):
    f = ff.exact_filter(kind, name)
    if kind == "sos":
        return cplx.sosfiltfilt(dev(f, dtype), x, padtype, padlen)
    return cplx.filtfilt(dev(f[0], dtype), dev(f[1], dtype), x, padtype, padlen)


def recorder(monkeypatch, with_pointers=False):
    """every entry point the host layers of filtfilt and of lfilter call, in order"""
    calls = []
    for mod in (hostff, hostiir):
        orig = mod.call

        def recording(name, *args, orig=orig):
            calls.append((name,) + tuple(None if v is None else v.value for v in args[:2]) if with_pointers else name)
            return orig(name, *args)
        monkeypatch.setattr(mod, "call", recording)
    return calls


# ---- 1. exact: integers in [-4, 4] ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,name", EXACT)
def test_exact_at_the_seams(kind, name, dtype):
    """N = e + 1, the chunk and tile seams of the extended row, one tile, three tiles and a rest, the explicit padlens and
    the extension longer than a tile, for every padtype: the oracle rounded ONCE (a bf16 workspace would round twice).
    float32 arithmetic takes the cases its headroom admits (filtfilt_cases.EXCLUDED), float64 all of them."""
    e = ff.exact_edge(kind, name)
    p = hostff.plan(4097 - 2 * e, e, 2 if kind == "sos" else len(ff.exact_filter(kind, name)[1]) - 1,
                    len(ff.exact_filter(kind, name)) if kind == "sos" else 1, ff.ROWS, 1, dtype)
    assert p["ext_len"] == 4097 and p["tile"] == (2048 if dtype == torch.float64 else 4096) and p["path"] == "row"
    for n, padlen in ff.exact_cases(kind, name, dtype == torch.float64):
        refs, _ = ff.exact_reference(kind, name, n, padlen)
        x = dev(ff.exact_signal(n), dtype)
        for padtype in ff.PADTYPES:
            y = run_exact(kind, name, x, dtype, padtype, padlen)
            assert_equal(y, refs[padtype], dtype, f"{kind} {name} N={n} padlen={padlen} {padtype}")


@pytest.mark.parametrize("segments", ff.SPLIT_SEGMENTS)
def test_exact_forced_split_path(segments, monkeypatch):
    """both passes cut into 2, 3, 7 segments (the last one shorter; with the reversed pass segment 0 is the END of the
    row): four launches each, the scaled state entering the scan"""
    n = ff.SPLIT_N
    calls = recorder(monkeypatch)
    monkeypatch.setattr(hostiir, "_FORCE_SEGMENTS", segments)
    for kind, name in EXACT:
        e = ff.exact_edge(kind, name)
        p = hostff.plan(n, e, 2, 1, ff.ROWS)
        assert p["path"] == "split" and p["segments"] == segments      # (the last segment is shorter for most edges)
        refs, _ = ff.exact_reference(kind, name, n, None)
        for dtype in DTYPES:
            if dtype != torch.float64 and not ff.admitted(kind, name, (n, None)):
                continue
            x = dev(ff.exact_signal(n), dtype)
            for padtype in ff.PADTYPES:
                del calls[:]
                y = run_exact(kind, name, x, dtype, padtype, None)
                assert calls == [PASS, PASS, "cplxamd_iir_scan", PASS] * 2
                assert_equal(y, refs[padtype], dtype, f"{kind} {name} split {segments} {padtype}")


# ---- 2. Gaussian data ---------------------------------------------------------------------------------------------------------
def check(got, ref, dtype, what):
    if dtype == torch.bfloat16:
        bad, worst = fc.bf16_violations(got if not torch.is_tensor(got) else Cplx(got, torch.zeros_like(got)),
                                        torch.from_numpy(np.ascontiguousarray(ref)))
        print(f"filtfilt_parity bf16 {what}: {bad} entries outside 2^-8 |ref| + 1e-5 max|ref|, worst at {worst:.3f}")
        assert bad == 0, what
    else:
        err = error(got, ref)
        print(f"filtfilt_parity {what} {dtype}: {err:.3g}")
        assert err <= fc.tol(dtype), what


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_gaussian_operand_pairs(kind, dtype):
    """every real / complex pair of signal and filter; all-real gives a real tensor"""
    xc, hc = KINDS[kind]
    g = ic.golden()
    b, a = (rounded(g[f"{'cpole' if hc else 'butter2'}_{k}"], dtype) for k in "ba")
    x = rounded(ic.gauss_data((3, 5000), 61, real=not xc), dtype)
    for padtype in ff.PADTYPES:
        y = cplx.filtfilt(dev(b, dtype, not hc), dev(a, dtype, not hc), dev(x, dtype, not xc), padtype)
        assert torch.is_tensor(y) == (kind == "rr")
        check(y, ff.filtfilt(b, a, x, padtype), dtype, f"{kind} {padtype}")
    sos = rounded(g["butter8sos_sos"] * ((1 + 0.5j) if hc else 1), dtype)
    y = cplx.sosfiltfilt(dev(sos, dtype, not hc), dev(x, dtype, not xc))
    assert torch.is_tensor(y) == (kind == "rr")
    check(y, ff.sosfiltfilt(sos, x), dtype, f"{kind} sos")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rows", [1, 3, 300])
def test_gaussian_rows_shared_and_per_channel_filters(rows, dtype):
    g = ic.golden()
    n = 4200
    x = rounded(ic.gauss_data((rows, 3, n), 62), dtype)
    names = ("butter4", "cheby4", "ellip4")
    bb, aa = (rounded(np.stack([g[f"{m}_{k}"] for m in names]), dtype) for k in "ba")
    y = cplx.filtfilt(dev(bb, dtype, True), dev(aa, dtype, True), dev(x, dtype))          # a filter per channel
    ref = np.stack([ff.filtfilt(bb[c], aa[c], x[:, c]) for c in range(3)], 1)
    check(y, ref, dtype, f"per channel rows={rows}")
    y = cplx.filtfilt(dev(bb[0], dtype, True), dev(aa[0], dtype, True), dev(x, dtype), "even", 100)   # one for all
    check(y, ff.filtfilt(bb[0], aa[0], x.reshape(-1, n), "even", 100).reshape(x.shape), dtype, f"shared rows={rows}")
    sos = rounded(np.stack([g["butter8sos_sos"], g["butter8sos_sos"][::-1] * 0.5, g["butter8sos_sos"]]), dtype)
    y = cplx.sosfiltfilt(dev(sos, dtype, True), dev(x, dtype), "constant")
    ref = np.stack([ff.sosfiltfilt(sos[c], x[:, c], "constant") for c in range(3)], 1)
    check(y, ref, dtype, f"sos per channel rows={rows}")
    # butter8 as a direct form (eight states) and as second-order sections
    b8, a8 = rounded(g["butter8_b"], dtype), rounded(g["butter8_a"], dtype)
    check(cplx.filtfilt(dev(b8, dtype, True), dev(a8, dtype, True), dev(x[:, 0], dtype)), ff.filtfilt(b8, a8, x[:, 0]), dtype,
          f"butter8 direct rows={rows}")
    check(cplx.sosfiltfilt(dev(sos[0], dtype, True), dev(x[:, 0], dtype)), ff.sosfiltfilt(sos[0], x[:, 0]), dtype,
          f"butter8 sos rows={rows}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_against_golden_scipy(dtype):
    g = ff.golden()
    padlen = int(g["padlen"])
    for name in ic.GAUSS_BA + ("butter8sos",):
        for kind in ("real", "cplx"):
            x = dev(g[f"x_{kind}"], dtype, kind == "real")
            for padtype in ff.PADTYPES:
                for tag, pl in (("default", None), ("padlen", padlen)):
                    if name == "butter8sos":
                        y = cplx.sosfiltfilt(dev(g["butter8sos_sos"], dtype, True), x, padtype,
                                             int(g["butter8sos_default_padlen"]) if pl is None else pl)
                    else:
                        b, a = g[f"{name}_b"], g[f"{name}_a"]
                        real = not (np.iscomplexobj(b) or np.iscomplexobj(a))
                        y = cplx.filtfilt(dev(b, dtype, real), dev(a, dtype, real), x, padtype, pl)
                    ref = g[f"{name}_{kind}_{ff.key(padtype)}_{tag}"] + 0j
                    assert error(y, ref) <= fc.tol(dtype), (name, kind, padtype, tag)


# ---- 3. the routes --------------------------------------------------------------------------------------------------------------
def test_two_launches_that_read_the_operands_in_place(monkeypatch):
    g = ic.golden()
    n = 4200
    xr, xi = (fc.gaussian((4, 3, n), torch.float32, s)[0].to(DEV) for s in (21, 22))
    b = dev(np.stack([g["butter4_b"], g["cheby4_b"], g["ellip4_b"]]), torch.float32, True)
    a = dev(np.stack([g["butter4_a"], g["cheby4_a"], g["ellip4_a"]]), torch.float32, True)
    sos = dev(g["butter8sos_sos"], torch.float32, True)
    calls = recorder(monkeypatch, with_pointers=True)

    def sliced(t):                                        # every second element of a buffer twice as long
        buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=DEV)
        buf[..., ::2] = t
        return buf[..., ::2]

    def transposed(t):                                    # the leading dims swapped in memory
        return t.transpose(0, 1).contiguous().transpose(0, 1)

    base = cplx.filtfilt(b, a, Cplx(xr, xi))
    base_sos = cplx.sosfiltfilt(sos, Cplx(xr, xi))
    assert [c[0] for c in calls] == [PASS] * 4            # two launches each, nothing else
    for name, fx in (("sliced", sliced), ("transposed", transposed)):
        x = Cplx(fx(xr), fx(xi))
        assert x.real.stride() != xr.stride()
        del calls[:]
        y = cplx.filtfilt(b, a, x)
        ys = cplx.sosfiltfilt(sos, x)
        # the first launch of each reads the planes at their own addresses: no layout copy, no padded copy
        assert [c[0] for c in calls] == [PASS] * 4, name
        assert calls[0][1:] == calls[2][1:] == (x.real.data_ptr(), x.imag.data_ptr()), name
        assert same_bits(y, base) and same_bits(ys, base_sos), name
    # an expanded SIGNAL shares its one row; the bits are those of its contiguous copy
    x1 = Cplx(xr[0, :1].expand(3, n), xi[0, :1].expand(3, n))
    del calls[:]
    y = cplx.filtfilt(b, a, x1)
    assert [c[0] for c in calls] == [PASS] * 2 and calls[0][1:] == (x1.real.data_ptr(), x1.imag.data_ptr())
    assert same_bits(y, cplx.filtfilt(b, a, Cplx(x1.real.contiguous(), x1.imag.contiguous())))
    # an expanded filter: the bits of the per-channel call
    assert same_bits(cplx.filtfilt(b[None].expand(4, 3, 5), a[None].expand(4, 3, 5), Cplx(xr, xi)), base)
    # a real signal through a real filter: the real kernels, two launches
    del calls[:]
    y = cplx.filtfilt(b, a, xr)
    assert torch.is_tensor(y) and [c[0] for c in calls] == [PASS] * 2 and calls[0][1:] == (xr.data_ptr(), None)
    with pytest.raises(RuntimeError):
        cplx.filtfilt(b[:2], a[:2], Cplx(xr, xi))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_one_workspace_is_the_only_intermediate(dtype):
    """the peak of the allocator over the call: y, the compute-type workspace of N + 2 padlen samples, under 1 MiB more"""
    g = ic.golden()
    rows, n = 8, 60000
    x = Cplx(*(p.to(DEV) for p in fc.gaussian((rows, n), dtype, 23)))
    b, a = dev(g["butter4_b"], dtype, True), dev(g["butter4_a"], dtype, True)
    sos = dev(g["butter8sos_sos"], dtype, True)
    for run, e in ((lambda: cplx.filtfilt(b, a, x), 15), (lambda: cplx.sosfiltfilt(sos, x), 27)):
        run()                                             # (the library is loaded, the kernels' attributes set)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = run()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        p = hostff.plan(n, e, 2, 1, rows, 1, dtype, True)
        assert p["signal_bytes"] == rows * (n + 2 * e) * 2 * 4
        out = 2 * y.real.numel() * y.real.element_size()
        assert out + p["signal_bytes"] <= peak <= out + p["signal_bytes"] + (1 << 20), (peak, out, p["signal_bytes"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_composed_routes_agree_with_the_fused_one(dtype, monkeypatch):
    g = ic.golden()
    n = 3000
    x = rounded(ic.gauss_data((2, n), 51), dtype)
    calls = recorder(monkeypatch)
    # requires_grad composes the same filter from lfilter / sosfilt launches: the fused result within tolerance
    b, a = rounded(g["butter4_b"], dtype), rounded(g["butter4_a"], dtype)
    sos = rounded(g["butter8sos_sos"], dtype)
    for padtype in ff.PADTYPES:
        fused = cplx.filtfilt(dev(b, dtype, True), dev(a, dtype, True), dev(x, dtype), padtype)
        assert calls == [PASS] * 2
        del calls[:]
        composed = cplx.filtfilt(dev(b, dtype, True), dev(a, dtype, True), dev(x, dtype, grad=True), padtype)
        assert PASS not in calls and calls.count("cplxamd_iir") == 2
        del calls[:]
        assert composed.real.requires_grad and error(composed, c128(fused).numpy()) <= fc.tol(dtype)
        assert error(composed, ff.filtfilt(b, a, x, padtype)) <= fc.tol(dtype)
        fused = cplx.sosfiltfilt(dev(sos, dtype, True), dev(x, dtype), padtype)
        composed = cplx.sosfiltfilt(dev(sos, dtype, True, grad=True), dev(x, dtype), padtype)
        assert error(composed, c128(fused).numpy()) <= fc.tol(dtype)
        del calls[:]
    # 20 sections: chained launches with the cumulative sosfilt_zi
    sos20 = rounded(np.tile(g["butter8sos_sos"], (5, 1)), dtype)
    y = cplx.sosfiltfilt(dev(sos20, dtype, True), dev(x, dtype))
    assert PASS not in calls and error(y, ff.sosfiltfilt(sos20, x)) <= fc.tol(dtype)
    del calls[:]
    # nb = 40: the numerator as a polyphase launch
    b40 = rounded(ic.gauss_data((40,), 52), dtype)
    y = cplx.filtfilt(dev(b40, dtype), dev(a, dtype, True), dev(x, dtype))
    assert PASS not in calls and error(y, ff.filtfilt(b40, a, x)) <= fc.tol(dtype)
    # D = 0 is a scale, twice
    y = cplx.filtfilt(dev([2 + 1j], dtype), dev([4], dtype), dev(x, dtype))
    assert error(y, x * ((2 + 1j) / 4) ** 2) <= fc.tol(dtype)


# ---- 4. derivatives -------------------------------------------------------------------------------------------------------------
def leaf(shape, seed, scale=1.0):
    return (fc.gaussian(shape, torch.float64, seed)[0] * scale).to(DEV).requires_grad_()


@pytest.mark.parametrize("kind", ["cplx", "real"])
def test_gradcheck_and_gradgradcheck_filtfilt(kind):
    """N = 40, padlen 6, D = 2; leaves x, b, a.  The gradients of real operands are real: the leaves are real planes."""
    n, planes_ = 40, 2 if kind == "cplx" else 1
    padtype = "odd" if kind == "cplx" else "constant"
    rows = 3 - planes_                                    # (the complex case has twice the leaves: one row)
    a0 = torch.tensor([[1.5, -0.4, 0.3], [1.2, 0.5, -0.2]], dtype=torch.float64)[:rows]
    leaves = []
    for p in range(planes_):
        leaves += [leaf((rows, n), 100 + p), leaf((rows, 3), 102 + p), (a0 * (1 if p == 0 else 0.2)).to(DEV).requires_grad_()]

    def fn(*args):
        ops = [args[i] if planes_ == 1 else Cplx(args[i], args[3 + i]) for i in range(3)]
        return tuple(p for p in planes(cplx.filtfilt(ops[1], ops[2], ops[0], padtype, 6)) if p is not None)

    assert torch.autograd.gradcheck(fn, leaves, **GC)
    assert torch.autograd.gradgradcheck(fn, leaves, **GC)


@pytest.mark.parametrize("kind", ["cplx", "real"])
def test_gradcheck_and_gradgradcheck_sosfiltfilt(kind):
    """a 2-section cascade, N = 40, padlen 6; leaves x and sos"""
    n = 40
    sos0 = torch.tensor([[0.5, 0.3, 0.2, 1.5, -0.4, 0.3], [1.0, -0.5, 0.1, 0.8, 0.2, 0.1]], dtype=torch.float64)
    rows = 2 if kind == "real" else 1                     # (the complex case has twice the leaves: one row)
    leaves = [leaf((rows, n), 111), sos0.to(DEV).requires_grad_()]
    if kind == "cplx":
        leaves += [leaf((rows, n), 112), (0.1 * sos0.flip(-1)).to(DEV).requires_grad_()]

    def fn(*args):
        x, sos = (args[0], args[1]) if kind == "real" else (Cplx(args[0], args[2]), Cplx(args[1], args[3]))
        return tuple(p for p in planes(cplx.sosfiltfilt(sos, x, "even", 6)) if p is not None)

    assert torch.autograd.gradcheck(fn, leaves, **GC)
    assert torch.autograd.gradgradcheck(fn, leaves, **GC)


# ---- 5. reruns, hipGraph, empty inputs, errors --------------------------------------------------------------------------------
def test_reruns_are_bit_identical(monkeypatch):
    g = ic.golden()
    x = Cplx(*(fc.gaussian((8, 9000), torch.float32, 70 + i)[0].to(DEV) for i in range(2)))
    b, a = (torch.from_numpy(g[f"butter4_{k}"]).float().to(DEV) for k in "ba")
    sos = torch.from_numpy(g["butter8sos_sos"]).float().to(DEV)
    for force in (0, 3):
        monkeypatch.setattr(hostiir, "_FORCE_SEGMENTS", force)
        assert same_bits(cplx.filtfilt(b, a, x), cplx.filtfilt(b, a, x))
        assert same_bits(cplx.sosfiltfilt(sos, x, "even"), cplx.sosfiltfilt(sos, x, "even"))
        xb = x.real.bfloat16()
        assert same_bits(cplx.filtfilt(b.bfloat16(), a.bfloat16(), xb), cplx.filtfilt(b.bfloat16(), a.bfloat16(), xb))


def test_graph_replay_equals_eager():
    g = ic.golden()
    sos = torch.from_numpy(g["butter8sos_sos"]).float().to(DEV)
    b, a = (torch.from_numpy(g[f"butter2_{k}"]).float().to(DEV) for k in "ba")

    def step(xr, xi):
        y = cplx.sosfiltfilt(sos, Cplx(xr, xi))
        w = cplx.filtfilt(b, a, y, "constant", 100)
        return w.real, w.imag

    shape = (4, 3, 4500)
    inputs = [fc.gaussian(shape, torch.float32, 81 + i)[0].to(DEV) for i in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*inputs)                                     # one eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*inputs)
    for seed in (84, 87):
        fresh = [fc.gaussian(shape, torch.float32, seed + i)[0].to(DEV) for i in range(2)]
        for t, f in zip(inputs, fresh):
            t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, step(*fresh)):
            assert torch.equal(o, e)


def test_errors_and_empty_inputs(monkeypatch):
    x = torch.zeros(4, 64, device=DEV)
    b, a = torch.ones(2, device=DEV), torch.tensor([1.0, -0.5], device=DEV)
    sos = torch.tensor([[1.0, 0, 0, 1, -0.5, 0]], device=DEV)
    calls = recorder(monkeypatch)
    for run in (lambda **k: cplx.filtfilt(b, a, x, **k), lambda **k: cplx.sosfiltfilt(sos, x, **k)):
        with pytest.raises(ValueError, match="greater than padlen, which is 64"):
            run(padlen=64)
        with pytest.raises(ValueError, match="padtype"):
            run(padtype="reflect")
        with pytest.raises(ValueError, match="padlen"):
            run(padlen=-1)
    with pytest.raises(ValueError, match="which is 6"):
        cplx.filtfilt(b, a, x[:, :6])
    with pytest.raises(CplxAmdError, match="sosfiltfilt"):
        cplx.filtfilt(b, torch.ones(10, device=DEV), x)
    with pytest.raises(CplxAmdError, match="different dtypes"):
        cplx.filtfilt(b.bfloat16(), a, x)
    with pytest.raises(CplxAmdError):
        cplx.filtfilt(b.cpu(), a.cpu(), x.cpu())
    with pytest.raises(CplxAmdError):
        cplx.sosfiltfilt(sos.cpu(), x)
    with pytest.raises(CplxAmdError):
        cplx.filtfilt(b.half(), a.half(), x.half())
    with pytest.raises(CplxAmdError):
        cplx.sosfiltfilt(sos.half(), x.half())
    empty = Cplx(torch.zeros(0, 64, device=DEV), torch.zeros(0, 64, device=DEV))
    out = cplx.filtfilt(b, a, empty)
    assert out.real.shape == (0, 64) and out.imag.shape == (0, 64)
    assert cplx.sosfiltfilt(sos, empty).real.shape == (0, 64)
    y = cplx.filtfilt(b, a, torch.zeros(4, 0, device=DEV))
    assert torch.is_tensor(y) and y.shape == (4, 0)
    assert cplx.sosfiltfilt(sos.bfloat16(), torch.zeros(4, 0, device=DEV).bfloat16()).dtype == torch.bfloat16
    assert calls == []                                    # nothing was launched
