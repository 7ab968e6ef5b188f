"""cplx.layer_norm without a GPU: the pure plan function at its seams, every argument error (raised before the device is
looked at) and the construction of nn.CplxLayerNorm."""
import pytest
import torch

from cplxmodule_amd import Cplx, cplx, layer_norm, nn
from cplxmodule_amd._lib import CplxAmdError


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["whiten", "modulus"])
def test_plan_at_the_seams(kind, dtype):
    base = layer_norm.plan(10, 8, kind, dtype)
    wave, block, bwd_block = base["seam_wave"], base["seam_block"], base["bwd_seam_block"]
    assert 8 < wave < bwd_block <= block
    want = {wave: ("wave", "wave"), wave + 1: ("block", "block"), bwd_block: ("block", "block"),
            bwd_block + 1: ("block" if bwd_block < block else "stream", "stream"), block: ("block", "stream"),
            block + 1: ("stream", "stream"), 1 << 20: ("stream", "stream")}
    for N, (fwd, bwd) in want.items():
        for rows in (0, 1, 10, 1 << 22):
            p = layer_norm.plan(rows, N, kind, dtype)
            assert (p["plan"], p["bwd_plan"]) == (fwd, bwd), (N, p)
            assert p["rows_per_wg"] == (4 if fwd == "wave" else 1) and p["stat_floats"] == (3 if kind == "modulus" else 5)
            assert p["tile"] >= N or fwd == "stream"
            wgs = -(-rows // p["bwd_rows_per_wg"])
            assert p["grid"] <= -(-rows // p["rows_per_wg"]) and p["bwd_grid"] == min(p["bwd_grid"], wgs)
            assert (p["bwd_grid"] >= 1) == (rows >= 1)
            assert p["ws_bytes"] == p["bwd_grid"] * 24 * N and p["ws_bytes"] <= p["ws_cap"]
    assert layer_norm.plan(1 << 22, 8192, kind, dtype)["bwd_grid"] < layer_norm.plan(1 << 22, 1024, kind, dtype)["bwd_grid"]
    for bad in (lambda: layer_norm.plan(10, 0, kind, dtype), lambda: layer_norm.plan(10, 8, kind, torch.float16)):
        with pytest.raises(CplxAmdError):
            bad()


X = Cplx(torch.randn(2, 5, 8), torch.randn(2, 5, 8))
BAD = {
    "plain": (CplxAmdError, lambda: cplx.layer_norm(torch.randn(2, 5, 8), 8)),
    "torch_complex": (CplxAmdError, lambda: cplx.layer_norm(torch.randn(5, 8, dtype=torch.complex64), 8)),
    "plane_dtype": (CplxAmdError, lambda: cplx.layer_norm(Cplx(X.real, X.imag.double()), 8)),
    "float16": (CplxAmdError, lambda: cplx.layer_norm(Cplx(X.real.half(), X.imag.half()), 8)),
    "cpu": (CplxAmdError, lambda: cplx.layer_norm(X, 8)),
    "kind": (ValueError, lambda: cplx.layer_norm(X, 8, kind="rms")),
    "trailing": (ValueError, lambda: cplx.layer_norm(X, 5)),
    "trailing_2d": (ValueError, lambda: cplx.layer_norm(X, (2, 8))),
    "weight_shape": (ValueError, lambda: cplx.layer_norm(X, 8, torch.ones(2, 8), torch.zeros(2, 8))),
    "bias_shape": (ValueError, lambda: cplx.layer_norm(X, 8, torch.ones(2, 2, 8), torch.zeros(8))),
    "bias_alone": (ValueError, lambda: cplx.layer_norm(X, 8, None, torch.zeros(2, 8))),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_need_no_device(case):
    kind, fn = BAD[case]
    with pytest.raises(kind) as e:
        fn()
    assert type(e.value) is kind


def test_module_constructs():
    m = nn.CplxLayerNorm((3, 8))
    assert isinstance(m, nn.CplxToCplx) and set(m.state_dict()) == {"weight", "bias"}
    assert m.weight.shape == (2, 2, 3, 8) and m.bias.shape == (2, 3, 8) and m.weight.dtype == torch.float32
    assert torch.equal(m.weight, torch.eye(2)[:, :, None, None].expand(2, 2, 3, 8)) and not m.bias.any()
    assert repr(m) == "CplxLayerNorm((3, 8), eps=1e-05, elementwise_affine=True, kind='whiten')"
    plain = nn.CplxLayerNorm(8, elementwise_affine=False, kind="modulus")
    assert plain.weight is None and plain.bias is None and not plain.state_dict() and plain.normalized_shape == (8,)
    with pytest.raises(ValueError):
        nn.CplxLayerNorm(8, kind="rms")
