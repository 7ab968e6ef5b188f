"""cplx.scaled_dot_product_attention without a GPU: every argument error (raised before the device is looked at), the
pure plan function and the construction of nn.CplxMultiheadAttention."""
import pytest
import torch

from cplxmodule_amd import Cplx, cplx, nn
from cplxmodule_amd._lib import CplxAmdError
from cplxmodule_amd import attention


def c(*shape, dtype=torch.float32):
    return Cplx(torch.randn(*shape).to(dtype), torch.randn(*shape).to(dtype))


Q, K, V = c(2, 5, 8), c(2, 7, 8), c(2, 7, 4)
BAD = {
    "attn_mask": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, K, V, attn_mask=torch.ones(5, 7))),
    "dropout": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, K, V, dropout_p=0.1)),
    "cpu": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, K, V)),
    "float16": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(*(c(2, 5, 8, dtype=torch.float16),) * 3)),
    "torch_complex": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(torch.randn(5, 8, dtype=torch.complex64), K, V)),
    "plain": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(torch.randn(2, 5, 8), K, V)),
    "plane_dtype": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Cplx(Q.real, Q.imag.double()), K, V)),
    "operand_dtype": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, c(2, 7, 8, dtype=torch.bfloat16), V)),
    "head_E": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(c(2, 5, 129), c(2, 7, 129), V)),
    "head_Ev": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, K, c(2, 7, 129))),
    "leading": (CplxAmdError, lambda: cplx.scaled_dot_product_attention(Q, c(3, 7, 8), c(3, 7, 4))),
    "score": (ValueError, lambda: cplx.scaled_dot_product_attention(Q, K, V, score="phase")),
    "below_2d": (ValueError, lambda: cplx.scaled_dot_product_attention(c(8), K, V)),
    "E_mismatch": (ValueError, lambda: cplx.scaled_dot_product_attention(Q, c(2, 7, 6), V)),
    "S_mismatch": (ValueError, lambda: cplx.scaled_dot_product_attention(Q, K, c(2, 6, 4))),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_need_no_device(case):
    kind, fn = BAD[case]
    with pytest.raises(kind) as e:
        fn()
    assert type(e.value) is kind                       # (CplxAmdError is a RuntimeError, never a ValueError, and back)
    if case == "attn_mask":
        assert "not offered yet" in str(e.value)


@pytest.mark.parametrize("L,S,E,Ev,batch", [(1, 1, 1, 1, 1), (128, 64, 64, 64, 6), (129, 130, 40, 24, 6), (4097, 33, 128, 128, 64)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plan(L, S, E, Ev, batch, dtype):
    p = attention.plan(L, S, E, Ev, batch, dtype)
    assert p["q_tiles"] == -(-L // p["q_tile"]) and p["grid"] == p["q_tiles"] * batch
    assert p["ws_bytes"] == 4 * batch * L
    assert p["k_tile"] == (64 if dtype == torch.bfloat16 else 32) and p["head"] >= max(E, Ev)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    with pytest.raises(CplxAmdError):
        attention.plan(L, S, 129, Ev, batch, dtype)


def test_module_constructs():
    m = nn.CplxMultiheadAttention(64, 4)
    assert isinstance(m, nn.CplxToCplx)
    want = {f"{p}_proj.{w}.{part}" for p in ("q", "k", "v", "out") for w in ("weight", "bias") for part in ("real", "imag")}
    assert set(m.state_dict()) == want
    assert set(nn.CplxMultiheadAttention(64, 4, bias=False).state_dict()) == {k for k in want if ".weight." in k}
    with pytest.raises(ValueError):
        nn.CplxMultiheadAttention(64, 5)
