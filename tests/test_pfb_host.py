"""cplx.pfb_analysis / pfb_synthesis without a GPU: every argument error with its type, raised on CPU operands before
the device is looked at, and the pure host plan (pfb.plan)."""
import pytest
import torch

from cplxmodule_amd import Cplx, cplx, pfb
from cplxmodule_amd._lib import CplxAmdError

X = Cplx(torch.zeros(2, 64), torch.zeros(2, 64))
H = torch.ones(16)
Y = Cplx(torch.zeros(2, 7, 8), torch.zeros(2, 7, 8))


@pytest.mark.parametrize("err, call", [
    (ValueError, lambda: cplx.pfb_analysis(X, H[:12], 6)),                       # M not a power of two
    (ValueError, lambda: cplx.pfb_analysis(X, H[:1], 1)),                        # M out of range
    (ValueError, lambda: cplx.pfb_analysis(X, torch.ones(8192), 8192)),
    (ValueError, lambda: cplx.pfb_analysis(X, H[:12], 8)),                       # K not a multiple of M
    (ValueError, lambda: cplx.pfb_analysis(Cplx(torch.zeros(260), torch.zeros(260)), torch.ones(130), 2)),   # P > 64
    (ValueError, lambda: cplx.pfb_analysis(X, H, 8, hop=0)),
    (ValueError, lambda: cplx.pfb_analysis(X, H, 8, hop=17)),
    (ValueError, lambda: cplx.pfb_analysis(X[..., :15], H, 8)),                  # T < K
    (ValueError, lambda: cplx.pfb_analysis(Cplx(torch.zeros(()), torch.zeros(())), H, 8)),
    (ValueError, lambda: cplx.pfb_synthesis(Y[..., :6], H[:12])),                # last dim is not a supported M
    (ValueError, lambda: cplx.pfb_synthesis(Y, H, hop=17)),
    (ValueError, lambda: cplx.pfb_synthesis(Y, H, length=6 * 8 + 15)),
    (CplxAmdError, lambda: cplx.pfb_analysis(X, H, 8)),                          # CPU tensors
    (CplxAmdError, lambda: cplx.pfb_synthesis(Y, H)),
    (CplxAmdError, lambda: cplx.pfb_analysis(Cplx(X.real.half(), X.imag.half()), H, 8)),
    (CplxAmdError, lambda: cplx.pfb_analysis(torch.zeros(64, dtype=torch.complex64), H, 8)),
    (CplxAmdError, lambda: cplx.pfb_analysis(Cplx(X.real, X.imag.bfloat16()), H, 8)),
    (CplxAmdError, lambda: cplx.pfb_analysis(Cplx(X.real, X.imag.to("meta")), H, 8)),
    (CplxAmdError, lambda: cplx.pfb_analysis(X, Cplx(H, H), 8)),                 # Cplx taps
    (CplxAmdError, lambda: cplx.pfb_synthesis(Y, H.clone().requires_grad_())),   # taps get no gradient
])
def test_argument_errors(err, call):
    with pytest.raises(err):
        call()


def test_tap_gradient_message():
    with pytest.raises(CplxAmdError, match="no gradient"):
        cplx.pfb_analysis(X, H.clone().requires_grad_(), 8)


@pytest.mark.parametrize("M, P, hop, frames, rows, cx", [
    (64, 8, 64, 1000, 3, True), (64, 8, 1, 5, 1, False), (2, 1, 2, 1, 1, True), (8, 64, 512, 700, 2, True),
    (1024, 8, 512, 37, 4, True), (2048, 2, 2048, 9, 1, True), (4096, 2, 4096, 3, 1, True), (4096, 16, 4096, 40, 2, True)])
def test_plan_covers_the_frames_inside_the_lds(M, P, hop, frames, rows, cx):
    p = pfb.plan(M, P, hop, frames, rows, cx)
    assert p["tiles"] * p["frames_per_tile"] >= frames > (p["tiles"] - 1) * p["frames_per_tile"]
    assert p["grid"] == rows * p["tiles"] and p["frames_per_tile"] % p["vectors_per_workgroup"] == 0
    assert p["lds_bytes"] <= 160 * 1024 and p["threads"] <= 512
    if p["plan"] == "staged":
        assert p["span"] == (p["frames_per_tile"] - 1) * hop + P * M
        assert p["lds_bytes"] >= 4 * (2 if cx else 1) * p["span"]
    assert p["ws_bytes"] == rows * frames * M * 4 * (2 if cx else 1)


def test_plan_seam():
    assert pfb.plan(64, 8)["plan"] == "staged"
    assert pfb.plan(4096, 16)["plan"] == "direct"         # one frame's span alone is 512 KiB
    assert pfb.plan(64, 8, frames=1000)["vectors_per_workgroup"] > 1 == pfb.plan(2048, 8)["vectors_per_workgroup"]
