"""Every convolution kernel behind cplxmodule_amd/conv.py, bit-exactly: integer-valued operands (conv_exact_cases.py) make
every route's result independent of the order of accumulation, so each output tensor must EQUAL the float64 reference
(float32 outputs) or its one round-to-nearest-even (bf16 outputs) -- and the entry points a case was written for must be
the ones that ran and returned success: a case that falls through to another kernel fails."""
import numpy as np
import pytest
import torch

import conv_exact_cases as K
from conv_exact_cases import CASES

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


class Recorder:
    """Recording wrappers around `call` / `try_call` of conv.py (and of ops.py: the 1 x 1 weight gradient is the linear
    layer's GEMM): (phase, entry point, returned success) per call."""

    def __init__(self, monkeypatch):
        from cplxmodule_amd import conv, ops, _lib
        self.log, self.phase = [], "fwd"

        def call(name, *a):
            try:
                _lib.call(name, *a)
            except Exception:
                self.log.append((self.phase, name, False))
                raise
            self.log.append((self.phase, name, True))

        def try_call(name, *a):
            ok = _lib.try_call(name, *a)
            self.log.append((self.phase, name, bool(ok)))
            return ok

        for mod in (conv, ops):
            monkeypatch.setattr(mod, "call", call)
            monkeypatch.setattr(mod, "try_call", try_call)

    def ran(self, phase):
        """The compute kernels that ran and returned success in a phase."""
        return sorted({n for p, n, ok in self.log if p == phase and ok and n in K.COMPUTE})

    def declined(self):
        return sorted({n for p, n, ok in self.log if not ok})


def _dev(a, dtype=torch.float32, layout="nchw", grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)
    if layout == "channels_last" and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(grad)


def _host(t):
    return None if t is None else t.detach().float().cpu().numpy()


def _run(c, layout, rec):
    """-> {result name: tensor} of what the case's operator computed (names as in conv_exact_cases.reference)."""
    from cplxmodule_amd import Cplx, cplx, conv
    d, _ = K.reference(c)
    dt = TORCH_DTYPE[c["dtype"]]
    api = c["api"]
    conv_kw = dict(stride=c["stride"], padding=c["padding"], dilation=c["dilation"], groups=c["groups"])
    act = lambda a, grad=False: _dev(a, dt, layout, grad)  # noqa: E731
    if api in ("cplx", "conv1d", "transpose"):
        xin, gout = ("g", "x") if api == "transpose" else ("x", "g")
        lv = {k: (act(d[k], True) if k[0] == xin else _dev(d[k], grad=True)) for k in d if k[0] in xin + "wb"}
        g = (act(d[gout + "r"]), act(d[gout + "i"]))
        x, w, b = Cplx(lv[xin + "r"], lv[xin + "i"]), Cplx(lv["wr"], lv["wi"]), Cplx(lv["br"], lv["bi"])
        if api == "cplx":
            y = cplx.conv2d(x, w, b, **conv_kw)
        elif api == "transpose":
            y = cplx.conv_transpose2d(x, w, b, stride=c["stride"], padding=c["padding"], output_padding=c["output_padding"],
                                      groups=c["groups"], dilation=c["dilation"])
        else:
            sq = lambda z: Cplx(z.real.squeeze(2), z.imag.squeeze(2))  # noqa: E731
            y = conv.cplx_conv1d(sq(x), sq(w), b, c["stride"][1], c["padding"][1], c["dilation"][1], c["groups"])
            y = Cplx(y.real.unsqueeze(2), y.imag.unsqueeze(2))
        rec.phase = "bwd"
        torch.autograd.backward((y.real, y.imag), g)
        return dict(yr=y.real, yi=y.imag, dxr=lv[xin + "r"].grad, dxi=lv[xin + "i"].grad, dwr=lv["wr"].grad, dwi=lv["wi"].grad,
                    dbr=lv["br"].grad, dbi=lv["bi"].grad)
    if api == "real":
        x, w, b = act(d["x"], True), _dev(d["w"], grad=True), _dev(d["b"], grad=True)
        y = conv.RealConv2dFn.apply(x, w, b, c["stride"], c["padding"], c["dilation"], c["groups"])
        rec.phase = "bwd"
        y.backward(act(d["g"]))
        return dict(y=y, dx=x.grad, dw=w.grad, db=b.grad)
    geom = K.geom_of(c)
    wshape = K.shapes(c)[1]
    out = {}
    if api == "direct":
        xr, xi, gr, gi = (act(d[k]) for k in ("xr", "xi", "gr", "gi"))
        wr, wi = _dev(d["wr"], dt), _dev(d["wi"], dt)
        if c["fwd"]:
            out["yr"], out["yi"] = conv.cl_conv(xr, xi, wr, wi, _dev(d["br"]), _dev(d["bi"]), geom)
        rec.phase = "bwd"
        if c["dgrad"]:
            out["dxr"], out["dxi"] = conv.cl_conv(gr, gi, wr, wi, None, None, geom, dgrad=True)
        if c["wgrad"]:
            out["dwr"], out["dwi"] = conv.cl_wgrad(gr, gi, xr, xi, geom, wshape)
        return out
    assert api == "cl_real"
    x, g, w = act(d["x"]), act(d["g"]), _dev(d["w"], dt)
    if c["fwd"]:
        out["y"] = conv.cl_conv_real(x, w, _dev(d["b"]), geom)
    rec.phase = "bwd"
    if c["dgrad"]:
        out["dx"] = conv.cl_conv_real(g, w, None, geom, dgrad=True)
    if c["wgrad"]:
        out["dw"] = conv.cl_wgrad_real(g, x, geom, wshape)
        out["dw*emul"] = conv.cl_wgrad_real(g, x, geom, wshape, emul=_dev(d["emul"]), emul_exp=False)
    return out


PARAMS = [pytest.param(n, lay, id=f"{n}-{lay}") for n, c in CASES.items() for lay in c["layouts"]]


@pytest.mark.parametrize("name,layout", PARAMS)
def test_conv_route_is_exact(name, layout, monkeypatch):
    c = CASES[name]
    d, ref = K.reference(c)
    rec = Recorder(monkeypatch)
    with K.switches(c):
        got = _run(c, layout, rec)
        torch.cuda.synchronize()
    problems = []
    want_fwd = sorted({K.ENTRY[c["fwd"]]} if c["fwd"] else set())
    want_bwd = sorted({K.ENTRY[r] for r in (c["dgrad"], c["wgrad"]) if r})
    if rec.ran("fwd") != want_fwd:
        problems.append(f"forward ran {rec.ran('fwd')}, expected {want_fwd} (declined: {rec.declined()})")
    if rec.ran("bwd") != want_bwd:
        problems.append(f"backward ran {rec.ran('bwd')}, expected {want_bwd} (declined: {rec.declined()})")
    assert got, "the case computes nothing"
    for k, t in got.items():
        assert t is not None, k
        exact = ref["dw"] * d["emul"] if k == "dw*emul" else ref[k]
        # y and dx come back in the activations' dtype, the weight and bias gradients in float32
        out_dtype = c["dtype"] if k[0] == "y" or k.startswith("dx") else "f32"
        assert t.dtype == TORCH_DTYPE[out_dtype], (k, t.dtype)
        msg = K.describe_mismatch(_host(t), K.expected(exact, out_dtype), c, k)
        if msg:
            problems.append(msg)
    assert not problems, f"{name} [{layout}]\n" + "\n".join(problems)
