"""cplx.conv_transpose3d / nn.CplxConvTranspose3d on the native 3-d kernel (csrc/conv3d.hip): bit-exact on integer-valued
operands over the whole case table of conv_transpose3d_cases.py, the reference's recorded values, Gaussian operands,
adjointness against the 2-d composition behind cplx.conv3d, determinism of the split-K weight gradient, the layer, and
graph capture."""
import contextlib

import numpy as np
import pytest
import torch

import conv_transpose3d_cases as K
from conv_transpose3d_cases import CASES
from gpu_util import DEV, T, N

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
ALLOWED = ("cplxamd_conv3d_dgrad", "cplxamd_conv3d_fwd", "cplxamd_conv3d_wgrad", "cplxamd_conv3d_out_shape",
           "cplxamd_chansum2")


@contextlib.contextmanager
def recorded_calls():
    """Names of the library entry points reached through the `call` / `try_call` of the host modules the operator can
    pass through, for the duration of the block."""
    from cplxmodule_amd import conv, conv3d, ops
    names, saved = [], []

    def wrap(fn):
        def inner(name, *args):
            names.append(name)
            return fn(name, *args)
        return inner

    for mod in (conv3d, conv, ops):
        for attr in ("call", "try_call"):
            saved.append((mod, attr, getattr(mod, attr)))
            setattr(mod, attr, wrap(getattr(mod, attr)))
    try:
        yield names
    finally:
        for mod, attr, fn in saved:
            setattr(mod, attr, fn)


def _layout(t, layout):
    if layout == "permuted":              # the same values behind a permuted view of a [B, D, H, W, C]-ordered buffer
        v = t.permute(0, 4, 2, 3, 1).contiguous().permute(0, 4, 2, 3, 1)
        assert not v.is_contiguous() and torch.equal(v, t)
        return v
    if layout == "channels_last_3d":
        v = t.contiguous(memory_format=torch.channels_last_3d)
        assert not v.is_contiguous() or min(t.shape[1:]) == 1
        return v
    return t


def run(c, d, dtype, layout="contiguous"):
    """The operator and its autograd gradients on operands `d` (numpy) -> (results as float32 numpy, entry points run)."""
    from cplxmodule_amd import Cplx, cplx
    dt = TORCH_DTYPE[dtype]
    t = {}
    for k, v in d.items():
        v = T(np.asarray(v, dtype=np.float32), dt)
        if k[0] == "x":
            v = _layout(v, layout)
        t[k] = v.requires_grad_(k[0] in "xwb")
    bias = Cplx(t["br"], t["bi"]) if c["bias"] else None
    with recorded_calls() as names:
        y = cplx.conv_transpose3d(Cplx(t["xr"], t["xi"]), Cplx(t["wr"], t["wi"]), bias, c["stride"], c["padding"],
                                  c["output_padding"], c["groups"], c["dilation"], c["padding_mode"])
        assert y.real.dtype == dt and y.imag.dtype == dt
        torch.autograd.backward((y.real, y.imag), (t["gr"], t["gi"]))
    out = dict(yr=y.real, yi=y.imag, dxr=t["xr"].grad, dxi=t["xi"].grad, dwr=t["wr"].grad, dwi=t["wi"].grad)
    if c["bias"]:
        out.update(dbr=t["br"].grad, dbi=t["bi"].grad)
    return {k: N(v) for k, v in out.items()}, names


def check_exact(c, dtype, layout="contiguous"):
    d, ref = K.reference(c)
    got, names = run(c, d, dtype, layout)
    bad = [n for n in names if n not in ALLOWED]
    assert not bad, f"entry points other than cplxamd_conv3d_* / cplxamd_chansum2 ran: {sorted(set(bad))}"
    want = {"cplxamd_conv3d_dgrad", "cplxamd_conv3d_fwd", "cplxamd_conv3d_wgrad"} | ({"cplxamd_chansum2"} if c["bias"] else set())
    assert want <= set(names), (want - set(names))
    report = [K.describe_mismatch(got[k], K.expected(ref[k], dtype), k) for k in ref]
    report = [r for r in report if r]
    assert not report, f"{c['name']} {dtype} {layout}\n" + "\n".join(report)
    return got


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_exact(name, dtype):
    check_exact(CASES[name], dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("layout", ["permuted", "channels_last_3d"])
def test_exact_layouts(layout, dtype):
    c = CASES["all_different"]
    got = check_exact(c, dtype, layout)
    plain = check_exact(c, dtype)
    for k in plain:
        assert np.array_equal(got[k], plain[k]), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_empty_batch(dtype):
    from cplxmodule_amd import Cplx, cplx
    c = dict(CASES["all_different"], B=0, name="empty_batch")
    xs, ws, ys = K.shapes(c)
    dt = TORCH_DTYPE[dtype]
    z = lambda s: torch.zeros(s, dtype=dt, device=DEV).requires_grad_(True)  # noqa: E731
    xr, xi, wr, wi, br, bi = z(xs), z(xs), z(ws), z(ws), z(ys[1]), z(ys[1])
    with torch.no_grad():
        wr.fill_(1.0), wi.fill_(-2.0)
    y = cplx.conv_transpose3d(Cplx(xr, xi), Cplx(wr, wi), Cplx(br, bi))
    assert tuple(y.shape) == ys and y.real.numel() == 0
    torch.autograd.backward((y.real, y.imag), (torch.zeros_like(y.real), torch.zeros_like(y.imag)))
    for g, like in ((wr.grad, wr), (wi.grad, wi), (br.grad, br), (bi.grad, bi)):
        assert g.shape == like.shape and not g.any()
    assert xr.grad.shape == xr.shape


# ---- 2. golden -----------------------------------------------------------------------------------------------------------------------
def _tol(ref, r=2e-5):
    return dict(rtol=r, atol=r * float(np.abs(ref).max()))


GOLDEN_KW = {
    "aniso": dict(stride=(1, 2, 3), padding=(0, 1, 2), output_padding=(0, 1, 2), dilation=(2, 1, 1), groups=2),
    "circular": dict(padding=(1, 2, 3), groups=2, padding_mode="circular"),
    "k4s2p1": dict(stride=2, padding=1),
}


@pytest.mark.parametrize("case", list(GOLDEN_KW))
def test_golden(golden, case):
    from cplxmodule_amd import Cplx, cplx
    g = golden("conv_transpose3d")
    assert sorted(GOLDEN_KW) == sorted(str(n) for n in g["cases"])
    k = case + "_"
    names = [n for n in ("xr", "xi", "wr", "wi", "br", "bi") if k + n in g]
    t = {n: T(g[k + n]).requires_grad_(True) for n in names}
    bias = Cplx(t["br"], t["bi"]) if "br" in t else None
    y = cplx.conv_transpose3d(Cplx(t["xr"], t["xi"]), Cplx(t["wr"], t["wi"]), bias, **GOLDEN_KW[case])
    assert y.shape == g[k + "yr"].shape
    np.testing.assert_allclose(N(y.real), g[k + "yr"], **_tol(g[k + "yr"]))
    np.testing.assert_allclose(N(y.imag), g[k + "yi"], **_tol(g[k + "yi"]))
    torch.autograd.backward((y.real, y.imag), (T(g[k + "gr"]), T(g[k + "gi"])))
    for n in names:
        np.testing.assert_allclose(N(t[n].grad), g[k + "d" + n], **_tol(g[k + "d" + n], 5e-5), err_msg=n)


# ---- 3. random values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.RANDOM_CASES)
def test_gaussian_f32(name):
    c = CASES[name]
    d = K.make_inputs(c, gaussian=True)
    d = {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in d.items()}      # what the device holds
    ref = K.torch_reference(c, d)
    got, _ = run(c, d, "f32")
    for k, v in ref.items():
        np.testing.assert_allclose(got[k], v, **_tol(v, 2e-5 if k[0] == "y" else 5e-5), err_msg=k)


@pytest.mark.parametrize("name", K.RANDOM_CASES)
def test_gaussian_bf16(name):
    """float64 on the bf16-rounded operands; |got - ref| <= 2^-8 |ref| (one bf16 ulp: the single rounding) + 1e-5 max|ref|
    (the float32 accumulation, at the package's norm-wise standard)."""
    c = CASES[name]
    d = K.make_inputs(c, gaussian=True)
    d = {k: torch.tensor(v, dtype=torch.float32).bfloat16().double().numpy() for k, v in d.items()}
    ref = K.torch_reference(c, d)
    got, _ = run(c, d, "bf16")
    for k, v in ref.items():
        err, bound = np.abs(got[k] - v), 2.0 ** -8 * np.abs(v) + 1e-5 * np.abs(v).max()
        print(f"{name} bf16 {k}: max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (k, float((err / bound).max()))


# ---- 4. adjointness --------------------------------------------------------------------------------------------------------------------
def test_adjoint_of_conv3d():
    """<conv3d_w(z), x> == <z, conv_transpose3d_conj(w)(x)>: cplx.conv3d is the 2-d composition, so this ties the new kernel
    to the old path."""
    from cplxmodule_amd import Cplx, cplx
    torch.manual_seed(0)
    z = cplx.randn(2, 8, 6, 7, 8, device=DEV)
    w = Cplx(0.1 * torch.randn(16, 8, 3, 3, 3, device=DEV), 0.1 * torch.randn(16, 8, 3, 3, 3, device=DEV))
    x = cplx.randn(2, 16, 4, 5, 6, device=DEV)
    cz = cplx.conv3d(z, w)
    tx = cplx.conv_transpose3d(x, Cplx(w.real, -w.imag))
    assert cz.shape == x.shape and tx.shape == z.shape
    lhs = (cz.real.double() * x.real + cz.imag.double() * x.imag).sum().item()
    rhs = (z.real.double() * tx.real + z.imag.double() * tx.imag).sum().item()
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
def test_split_k_weight_gradient_is_deterministic():
    c = CASES["splitk"]
    d = K.make_inputs(c, gaussian=True)
    a, _ = run(c, d, "f32")
    b, _ = run(c, d, "f32")
    assert np.array_equal(a["dwr"], b["dwr"]) and np.array_equal(a["dwi"], b["dwi"])


# ---- 6. the layer ----------------------------------------------------------------------------------------------------------------------
def test_layer(golden):
    from cplxmodule_amd import cplx
    from cplxmodule_amd._lib import CplxAmdError
    from cplxmodule_amd.nn import CplxConvTranspose3d
    g = golden("conv_transpose3d")
    torch.manual_seed(1)
    layer = CplxConvTranspose3d(4, 6, 3, stride=2, padding=1, bias=True).to(DEV)
    x = cplx.randn(2, 4, 3, 4, 5, device=DEV)
    assert layer(x).shape == (2, 6, 5, 7, 9)
    assert layer(x, output_size=(6, 8, 10)).shape == (2, 6, 6, 8, 10)
    with pytest.raises(ValueError):
        layer(x, output_size=(7, 8, 10))
    state = {str(k): torch.randn(*(int(n) for n in g[f"layer_bias_shape_{k}"])) for k in g["layer_bias_keys"]}
    layer.load_state_dict(state)
    assert torch.equal(layer.weight.real.cpu(), state["weight.real"]) and torch.equal(layer.bias.imag.cpu(), state["bias.imag"])
    out = layer(x, output_size=(6, 8, 10))
    fn = cplx.conv_transpose3d(x, layer.weight, layer.bias, 2, 1, 1)
    assert torch.equal(out.real, fn.real) and torch.equal(out.imag, fn.imag)
    # no float64 form
    with pytest.raises(CplxAmdError, match="float64"):
        layer.double()(cplx.Cplx(x.real.double(), x.imag.double()))
    # no second derivative
    layer.float()
    xr, xi = x.real.clone().requires_grad_(True), x.imag.clone().requires_grad_(True)
    y = layer(cplx.Cplx(xr, xi))
    gx, = torch.autograd.grad(y.real.sum() + y.imag.sum(), xr, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits():
    """Forward and backward of the layer captured in one graph on one stream after an eager warm-up (utils.graphs.GraphedStep:
    no autograd graph of an earlier eager step may be alive when the capture starts, so the eager run comes LAST)."""
    from cplxmodule_amd import Cplx
    from cplxmodule_amd.nn import CplxConvTranspose3d
    from cplxmodule_amd.utils.graphs import GraphedStep
    c = CASES["all_different"]
    torch.manual_seed(2)
    layer = CplxConvTranspose3d(c["cin"], c["cout"], c["k"], bias=True).to(DEV)
    xs, _, ys = K.shapes(c)
    xr, xi = (torch.randn(xs, device=DEV).requires_grad_(True) for _ in range(2))
    gr, gi = torch.randn(ys, device=DEV), torch.randn(ys, device=DEV)
    params = [xr, xi, layer.weight.real, layer.weight.imag, layer.bias.real, layer.bias.imag]

    def step():
        for p in params:
            p.grad = None
        y = layer(Cplx(xr, xi))
        torch.autograd.backward((y.real, y.imag), (gr, gi))
        return [y.real.detach(), y.imag.detach()] + [p.grad for p in params]

    graphed = GraphedStep(step, modules=[layer], warmup=2)
    for o in graphed.outputs:
        o.zero_()
    graphed.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in graphed.outputs]
    assert all(o.any() for o in got)
    want = step()                                                # eager, afterwards
    assert len(got) == 8
    for a, b in zip(got, want):
        assert torch.equal(a, b)
