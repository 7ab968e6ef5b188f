"""The plan of the parameter-gradient kernel behind cplx.ssm_scan's backward (csrc/ssm_grad.hip): a pure host call."""
import pytest
import torch

from cplxmodule_amd import ssm
from cplxmodule_amd._lib import CplxAmdError


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cx,vary,group", [(True, True, 1), (True, False, 1), (False, True, 2), (False, False, 4)])
def test_plan(cx, vary, group, dtype):
    rows, N = 6, 17
    one, two = (ssm.grad_plan(T, N, rows, dtype, cx, vary) for T in (4096, 5003))
    fwd = ssm.plan(5003, N, rows, dtype, cx, vary)
    assert (two["chunk"], two["tile"], two["tiles"]) == (fwd["chunk"], fwd["tile"], fwd["tiles"]) == (16, 4096, 2)
    assert one["tiles"] == 1 and one["ws_bytes"] == 0
    assert two["ws_bytes"] == rows * 2 * N * 4 * (2 if cx else 1)
    assert two["group"] == group and (two["threads"], two["grid"]) == (256, rows)
    # the carried states, the exchange of both maps and that of the waves' sums, all double-buffered
    ns = 2 if cx else 1
    assert two["lds_bytes"] == 4 * (2 * 256 * ns + 2 * 2 * 4 * group * 2 * ns + 2 * 4 * group * 3 * ns) <= 65536
    assert ssm.grad_plan(0, N, rows, dtype, cx, vary)["grid"] == 0


@pytest.mark.parametrize("bad", [dict(N=0), dict(N=257), dict(dtype=torch.float64)])
def test_plan_rejects(bad):
    with pytest.raises(CplxAmdError):
        ssm.grad_plan(100, **{"N": 16, **bad})
