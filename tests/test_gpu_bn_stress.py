"""Complex batch norm on ill-conditioned inputs, on every route (csrc/bn.hip, the moment epilogue of csrc/conv_cl2.hip, the
apply pass folded into csrc/conv_cl_wgrad.hip): large mean / std, correlation up to 0.999 and xi = c xr, xi == 0, constant
features, per-feature scales 1e-6 ... 1e6, 1 - 3 positions per feature.  The cases are tests/bn_stress_cases.py; the
margins over the 1e-5 float32 bar are the reference's own float32 error recorded in tests/golden/bn_stress.npz
(scripts/gen_bn_stress_golden.py), capped by tests/test_bn_stress_host.py.  Every comparison is norm-wise PER FEATURE:
a feature of scale 1e-6 next to one of scale 1e6 is held to the same relative bar.

Measured on an MI355X (profiles/bn_stress_parity.txt): see the numbers next to the assertions."""
import numpy as np
import pytest
import torch

import bn_stress_cases as sc
from oracle import cplx_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16_BARS = {"y": 1e-2, "dx": 2e-2, "dweight": 1e-3, "dbias": 1e-3}       # test_batchnorm_channels_last_rows_kernels


def _within(e, tol, what):
    """max_f e[f] <= tol, through assert_allclose on 1 + e against 1 with rtol = tol: the parity report then shows the
    achieved per-feature error (rel_elem) next to the asserted one (rtol_asked)."""
    e = np.asarray(e, np.float64)
    np.testing.assert_allclose(1.0 + e, np.ones_like(e), rtol=tol, atol=0, err_msg=what)


def _layer(case, d):
    from gpu_util import T
    from cplxmodule_amd import nn
    cls = {2: nn.CplxBatchNorm1d, 3: nn.CplxBatchNorm1d, 4: nn.CplxBatchNorm2d}[len(case.shape)]
    bn = cls(case.shape[1], eps=sc.EPS, momentum=sc.MOMENTUM).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(T(d["weight"])); bn.bias.copy_(T(d["bias"]))
    return bn


def _planes(case, d):
    from gpu_util import T
    td = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    put = (lambda a: T(a, td).contiguous(memory_format=torch.channels_last)) if case.cl else (lambda a: T(a, td))
    return tuple(put(d[k]) for k in ("xr", "xi", "gr", "gi"))


def _run(bn, xr, xi, gr, gi):
    from gpu_util import N
    from cplxmodule_amd import Cplx
    bn.zero_grad()
    xr, xi = xr.detach().requires_grad_(True), xi.detach().requires_grad_(True)
    y = bn(Cplx(xr, xi))
    torch.autograd.backward((y.real, y.imag), (gr, gi))
    got = {"y": sc.stack_planes(N(y.real), N(y.imag)), "dx": sc.stack_planes(N(xr.grad), N(xi.grad)),
           "dweight": N(bn.weight.grad), "dbias": N(bn.bias.grad),
           "running_mean": N(bn.running_mean), "running_var": N(bn.running_var)}
    return y, got


@pytest.fixture(scope="module")
def e_ref(golden):
    return golden("bn_stress")


@pytest.mark.parametrize("name", sc.F32_CASES + sc.BF16_CASES)
def test_every_own_pass_route_against_the_float64_oracle(e_ref, name):
    """Forward, backward, running statistics and evaluation mode of the layer's own kernels (reduce planes / small /
    cols / rows, both apply forms, float32 and bf16) against the float64 oracle, per feature.  float32: max(1e-5,
    4 e_ref) -- the statistics are float64 sums here, so what may differ from the float32 reference is rounding order
    in the float32 steps both share (x - (float) mu, the float32 coefficients), hence a small multiple of ITS error and no
    more.  bf16: the oracle on the bf16-rounded values, the bf16 bars of test_batchnorm_channels_last_rows_kernels.
    The cases with 1, 2, 3 positions, constant and xi == 0 features must come out finite on top.
    Achieved (MI355X): float32 <= 0.3 x the asserted margin on every case, bf16 <= 0.15 x -- profiles/bn_stress_parity.txt."""
    case = sc.BY_NAME[name]
    d = sc.build(case)
    floor = sc.floors(d)
    bn = _layer(case, d)
    xr, xi, gr, gi = _planes(case, d)
    if case.cl:
        assert xr.is_contiguous(memory_format=torch.channels_last) and not xr.is_contiguous()
    for mode in ("train", "eval"):
        training = mode == "train"
        if training:
            bn.train()
        else:
            from gpu_util import T
            bn.eval()
            with torch.no_grad():
                bn.running_mean.copy_(T(d["running_mean"])); bn.running_var.copy_(T(d["running_var"]))
        y, got = _run(bn, xr, xi, gr, gi)
        assert y.real.dtype == xr.dtype and y.real.is_contiguous(memory_format=torch.channels_last) == (
            xr.is_contiguous(memory_format=torch.channels_last))
        ref = sc.oracle_results(orc, d, np.float64, training)
        for q in (sc.QUANTITIES if training else sc.EVAL_QUANTITIES):
            assert np.isfinite(got[q]).all(), (name, mode, q)
            e = sc.rel_per_feature(sc.as_feature_rows(q, got[q]), sc.as_feature_rows(q, ref[q]), floor.get(q))
            if q.startswith("running"):
                # (b): the bar the existing tests hold the running statistics to, elementwise -- and the per-feature form
                np.testing.assert_allclose(got[q], ref[q], rtol=1e-5, atol=1e-6, err_msg=f"{name} {q}")
                tol = 1e-5
            elif case.dtype == "bf16":
                tol = BF16_BARS[q]
            else:
                tol = max(1e-5, 4.0 * float(e_ref[f"{name}/{mode}/e_ref/{q}"]))
            f = int(np.argmax(e))
            _within(e, tol, f"{name} {mode} {q}: worst feature {f} {tuple(d['conds'][f])}")


# ---- (c) the statistics out of the convolution's epilogue against the layer's own pass over the same stored output -------
MOM_SHAPES = [(3, 64, 50, 70, 0, 64), (2, 64, 33, 37, 1, 64), (2, 32, 16, 32, 1, 64), (5, 64, 18, 34, 0, 64),
              (300, 64, 20, 40, 1, 64), (70, 32, 30, 60, 1, 128), (40, 64, 34, 66, 0, 256), (1, 32, 16, 32, 1, 128),
              (128, 32, 128, 128, 1, 64)]      # the last one: 4096 tiles, 16 per workgroup -- a lane carries 512 pixels
RATIOS = (0.0, 2.0, 8.0, 32.0)


@pytest.mark.parametrize("B,C,H,W,pad,Nc", MOM_SHAPES)
def test_conv_epilogue_moments_on_offset_outputs(B, C, H, W, pad, Nc):
    """conv.cl_conv(..., moments=True) with a bias that puts mean / std of the bf16 output at 0, 2, 8, 32 over the channels
    (real part; minus half of that on the imaginary part), then the batch-norm forward
    twice on the SAME stored output: from the epilogue's partial rows (cplxamd_bn_fwd_partials) and with its own moment
    pass (cplxamd_bn_fwd_ex).  Mean, covariance, whitening coefficients and running statistics to rtol 2e-5 / atol 2e-6
    (the bar of test_conv_batchnorm_pair_uses_the_epilogue_moments) at every ratio; outputs one bf16 step apart in
    < 1e-3 of the entries.  Route against route: the convolution's own accuracy does not enter.
    Measured (MI355X, largest |difference| over the bar): raw float32 lane sums, which the epilogue kept before it summed
    about a pivot, 1.56 at mean / std 8 and 2.02 at 32 on the 512-pixels-per-lane shape (0.18 at 2); now <= 0.10 on every
    shape and ratio (profiles/bn_stress_parity.txt)."""
    from gpu_util import N
    from cplxmodule_amd import _lib, bn as bnmod, conv, ops
    from cplxmodule_amd._lib import call, ptr, stream_ptr
    bf, cl = torch.bfloat16, torch.channels_last
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + H)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    xr, xi = (mk(B, C, H, W).to(bf).contiguous(memory_format=cl) for _ in range(2))
    xr, xi = xr + 0.5, xi - 0.25
    wr, wi = (mk(Nc, C, 3, 3).mul(0.05).to(bf) for _ in range(2))
    geom, _ = conv._geom(xr.shape, wr.shape, (1, 1), (pad, pad), (1, 1), 1)
    zero = torch.zeros(Nc, device=DEV)
    y0r, y0i = conv.cl_conv(xr, xi, wr, wi, zero, zero, geom)
    ratio = torch.tensor([RATIOS[c % 4] for c in range(Nc)], device=DEV)
    br = (ratio * y0r.float().std((0, 2, 3)) - y0r.float().mean((0, 2, 3))).contiguous()
    bi = (-0.5 * ratio * y0i.float().std((0, 2, 3)) - y0i.float().mean((0, 2, 3))).contiguous()
    del y0r, y0i
    old = conv._MOMENTS
    try:
        conv._MOMENTS = True
        yr, yi = conv.cl_conv(xr, xi, wr, wi, br, bi, geom, moments=True)
        hint = ops.moments_hint(yr, yi)
        conv._MOMENTS = False
        pr, pi = conv.cl_conv(xr, xi, wr, wi, br, bi, geom, moments=True)
    finally:
        conv._MOMENTS = old
    assert hint is not None and ops.moments_hint(pr, pi) is None
    assert torch.equal(yr, pr) and torch.equal(yi, pi)                 # the identical y
    del pr, pi, xr, xi
    got_ratio = N(yr.float().mean((0, 2, 3)) / yr.float().std((0, 2, 3)))
    np.testing.assert_allclose(got_ratio, N(ratio), rtol=0.05, atol=0.05)          # (the stored output IS that offset)
    P, F = yr.shape[0] * yr.shape[2] * yr.shape[3], Nc
    torch.manual_seed(1)
    w = (torch.eye(2, device=DEV).reshape(2, 2, 1) + 0.2 * torch.randn(2, 2, F, device=DEV)).contiguous()
    b = (0.3 * torch.randn(2, F, device=DEV)).contiguous()
    ws = bnmod._ws(torch.device(DEV, torch.cuda.current_device()), F)
    res = []
    for fused in (True, False):
        zr, zi = torch.empty_like(yr), torch.empty_like(yi)
        saved = torch.empty(8, F, device=DEV)
        rm, rv = torch.zeros(2, F, device=DEV), torch.eye(2, device=DEV).reshape(2, 2, 1).repeat(1, 1, F).contiguous()
        if fused:
            call("cplxamd_bn_fwd_partials", ptr(yr), ptr(yi), ptr(zr), ptr(zi), P, F, 1, ptr(w), ptr(b), ptr(rm), ptr(rv),
                 ptr(saved), _lib.BF16, 0.1, 1e-5, None, ptr(hint[0]), hint[1], ptr(ws), ws.numel(), stream_ptr())
        else:
            call("cplxamd_bn_fwd_ex", ptr(yr), ptr(yi), ptr(zr), ptr(zi), P, F, 1, ptr(w), ptr(b), ptr(rm), ptr(rv),
                 ptr(saved), 1, _lib.BF16, 0.1, 1e-5, None, ptr(ws), ws.numel(), stream_ptr())
        torch.cuda.synchronize()
        res.append((zr, zi, saved, rm, rv))
    fu, pl = res
    names = ((2, "saved (mean | whitening p q w | covariance)"), (3, "running_mean"), (4, "running_var"))
    for k, what in names:                        # the figures first (pytest -s / the captured output of a failure) ...
        for r in range(4):
            u, v = N(fu[k])[..., r::4].astype(np.float64), N(pl[k])[..., r::4].astype(np.float64)
            print(f"epilogue moments {(B, C, H, W, pad, Nc)} mean/std {RATIOS[r]:4.0f} {what.split()[0]:13s}"
                  f" max |d| / (2e-6 + 2e-5 |ref|) = {float((np.abs(u - v) / (2e-6 + 2e-5 * np.abs(v))).max()):.3f}")
    for k, what in names:                        # ... then the bar, per group of channels
        for r in range(4):
            np.testing.assert_allclose(N(fu[k])[..., r::4], N(pl[k])[..., r::4], rtol=2e-5, atol=2e-6,
                                       err_msg=f"{what}, channels at mean / std {RATIOS[r]}")
    for a, c in ((fu[0], pl[0]), (fu[1], pl[1])):
        a, c = a.float(), c.float()
        assert float((a - c).abs().max()) <= 2 ** -6 * float(c.abs().max())          # a bf16 ulp of the largest entries
        assert float((a != c).float().mean()) < 1e-3


# ---- (d) the apply pass folded into the weight-gradient launch, on offset / correlated activations ------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64, 64, 64, 1), (3, 64, 64, 40, 72, 1), (2, 64, 128, 48, 64, 0)])
@pytest.mark.parametrize("train", [True, False])
def test_fold_matches_the_separate_launches_on_offset_activations(shape, train):
    """CplxConv2d -> CplxBatchNorm2d whose convolution output has mean / std 0, 2, 8, 32 over the channels (the bias) and
    whose input has offset, strongly correlated parts (xi = 0.8 xr + 0.1 noise): CPLXAMD_BN_FOLD on against off, to the bars
    of test_fold_matches_the_separate_launches, taken per channel instead of over the tensor."""
    from cplxmodule_amd import Cplx, conv as cv, nn
    B, Ci, Co, H, W, pad = shape
    old = cv._CL_FORCE, cv._BN_FOLD
    cv._CL_FORCE = True
    calls = []
    real = cv.cl_wgrad_bn
    cv.cl_wgrad_bn = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        res = {}
        for fold in (False, True):
            cv._BN_FOLD = fold
            torch.manual_seed(11)
            layer, bn = nn.CplxConv2d(Ci, Co, 3, padding=pad).to(DEV), nn.CplxBatchNorm2d(Co).to(DEV)
            base = torch.randn(B, Ci, H, W, device=DEV)
            mk = lambda t: t.bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)  # noqa: E731
            x = Cplx(mk(1.5 * base + 0.7), mk(0.8 * base + 0.1 * torch.randn_like(base) - 0.2))
            with torch.no_grad():
                bn.weight.add_(0.3 * torch.randn_like(bn.weight)); bn.bias.add_(0.3 * torch.randn_like(bn.bias))
                y = layer(Cplx(x.real.detach(), x.imag.detach()))
                ratio = torch.tensor([RATIOS[c % 4] for c in range(Co)], device=DEV)
                layer.bias.real.add_(ratio * y.real.float().std((0, 2, 3)) - y.real.float().mean((0, 2, 3)))
                layer.bias.imag.add_(-0.5 * ratio * y.imag.float().std((0, 2, 3)) - y.imag.float().mean((0, 2, 3)))
                del y
            if not train:
                bn(layer(x)); bn.eval()
            Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
            g = tuple(torch.randn(B, Co, Ho, Wo, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
                      for _ in range(2))
            y = bn(layer(x))
            torch.autograd.backward((y.real, y.imag), g)
            res[fold] = [t.float().clone() for t in (x.real.grad, x.imag.grad, layer.weight.real.grad, layer.weight.imag.grad,
                                                     layer.bias.real.grad, layer.bias.imag.grad, bn.weight.grad, bn.bias.grad)]
    finally:
        cv.cl_wgrad_bn = real
        cv._CL_FORCE, cv._BN_FOLD = old
    assert len(calls) == 1
    a, b = res[False], res[True]
    n = B * Ho * Wo
    chan_max = lambda t, dim: t.abs().amax([k for k in range(t.dim()) if k != dim])  # noqa: E731
    for i, (u, v) in enumerate(zip(a, b)):
        if i < 2:        # dX [B, Ci, H, W]: per input channel
            assert bool((chan_max(u - v, 1) <= 8e-3 * chan_max(u, 1)).all()), i
        elif i < 4:      # dW [Co, Ci, 3, 3]: per output channel = per batch-norm feature
            assert bool((chan_max(u - v, 0) <= 3e-4 * chan_max(u, 0)).all()), i
        elif i < 6:      # the convolution's bias gradient: rounding noise of the stored dX against the analytic value
            noise = 4e-3 * float(a[0].abs().max()) * np.sqrt(n) + 1e-6
            assert float((u - v).abs().max()) <= max(noise, 5e-3 * float(u.abs().max())), i
        else:
            assert torch.equal(u, v), i


# ---- (e) the statistics handed in from outside (the cross-rank route), in one process -------------------------------------
@pytest.mark.parametrize("name", ["cols_hard", "small_hard", "large_hard", "rows_hard", "count2", "rows_bf16"])
def test_moments_in_route_gives_the_bits_of_the_ordinary_call(name):
    """cplxamd_bn_moments -> cplxamd_bn_fwd_sync / _bwd_sync with the call's own totals handed back as the 'summed' ones
    and the count on the device: the same bits as cplxamd_bn_fwd_ex / cplxamd_bn_bwd_sums (the totals are the chunk
    partials summed in the order the finalize uses)."""
    from gpu_util import T
    from cplxmodule_amd import _lib, bn as bnmod
    from cplxmodule_amd._lib import call, ptr, stream_ptr
    case = sc.BY_NAME[name]
    d = sc.build(case)
    xr, xi, gr, gi = _planes(case, d)
    code = _lib.BF16 if case.dtype == "bf16" else _lib.F32
    F = case.shape[1]
    n = int(np.prod(case.shape)) // F
    B, S = (n, 1) if case.cl else (case.shape[0], n // case.shape[0])
    w, b = T(d["weight"]), T(d["bias"])
    ws = bnmod._ws(torch.device(DEV, torch.cuda.current_device()), F)
    rows = bool(_lib.load().cplxamd_bn_rows_path(B, F, S))
    out = []
    for sync in (False, True):
        yr, yi, dxr, dxi = (torch.empty_like(xr) for _ in range(4))
        saved = torch.empty(8, F, device=DEV)
        rm, rv = torch.zeros(2, F, device=DEV), torch.eye(2, device=DEV).reshape(2, 2, 1).repeat(1, 1, F).contiguous()
        dw, db = torch.empty(2, 2, F, device=DEV), torch.empty(2, F, device=DEV)
        sums = torch.empty(2, F, device=DEV) if rows else None
        if not sync:
            call("cplxamd_bn_fwd_ex", ptr(xr), ptr(xi), ptr(yr), ptr(yi), B, F, S, ptr(w), ptr(b), ptr(rm), ptr(rv), ptr(saved),
                 1, code, sc.MOMENTUM, sc.EPS, None, ptr(ws), ws.numel(), stream_ptr())
            call("cplxamd_bn_bwd_sums", ptr(gr), ptr(gi), ptr(xr), ptr(xi), ptr(dxr), ptr(dxi), B, F, S, ptr(w), ptr(saved),
                 ptr(dw), ptr(db), 1, code, ptr(sums), ptr(ws), ws.numel(), stream_ptr())
        else:
            m = torch.empty(F * 5, dtype=torch.float64, device=DEV)
            count = torch.full((1,), float(B * S), dtype=torch.float64, device=DEV)
            call("cplxamd_bn_moments", ptr(xr), ptr(xi), None, None, None, B, F, S, code, ptr(m), ptr(ws), ws.numel(),
                 stream_ptr())
            call("cplxamd_bn_fwd_sync", ptr(xr), ptr(xi), ptr(yr), ptr(yi), B, F, S, ptr(w), ptr(b), ptr(rm), ptr(rv),
                 ptr(saved), code, sc.MOMENTUM, sc.EPS, ptr(m), ptr(count), ptr(ws), ws.numel(), stream_ptr())
            local = torch.empty(F * 6, dtype=torch.float64, device=DEV)
            call("cplxamd_bn_moments", ptr(xr), ptr(xi), ptr(gr), ptr(gi), ptr(saved), B, F, S, code, ptr(local), ptr(ws),
                 ws.numel(), stream_ptr())
            total = local.clone()
            call("cplxamd_bn_bwd_sync", ptr(gr), ptr(gi), ptr(xr), ptr(xi), ptr(dxr), ptr(dxi), B, F, S, ptr(w), ptr(saved),
                 ptr(dw), ptr(db), code, ptr(sums), ptr(total), ptr(local), ptr(count), ptr(ws), ws.numel(), stream_ptr())
        torch.cuda.synchronize()
        out.append(dict(yr=yr, yi=yi, saved=saved, running_mean=rm, running_var=rv, dxr=dxr, dxi=dxi, dweight=dw, dbias=db,
                        **({"dx_sums": sums} if rows else {})))
    for k in out[0]:
        assert bool(torch.isfinite(out[0][k].float()).all()), k
        assert torch.equal(out[0][k], out[1][k]), (name, k)
