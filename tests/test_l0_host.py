"""LinearL0 / LinearLASSO (nn/relevance/extensions/real.py) without a GPU: exports, class layout, parameter shapes,
defaults, state dicts against the reference's own (tests/golden/l0.npz, scripts/gen_l0_golden.py), and the C-ABI
entry points of csrc/l0.hip."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("cplxamd_l0_gate_fwd", "cplxamd_l0_gate_bwd", "cplxamd_l0_gate_bwd_ws_bytes", "cplxamd_l1_mask",
               "cplxamd_philox_uniform")


def test_both_import_paths():
    from cplxmodule_amd.nn.relevance import LinearL0, LinearLASSO
    from cplxmodule_amd.nn.relevance import extensions
    from cplxmodule_amd.nn.relevance.extensions import LinearL0 as L0, LinearLASSO as LASSO
    assert L0 is LinearL0 and LASSO is LinearLASSO
    assert {"LinearL0", "LinearLASSO"} <= set(extensions.__all__)


def test_class_layout_matches_reference():
    from cplxmodule_amd.nn.relevance import BaseARD, LinearL0, LinearLASSO
    from cplxmodule_amd.nn.utils.sparsity import SparsityStats
    for cls in (LinearL0, LinearLASSO):
        assert issubclass(cls, torch.nn.Linear) and issubclass(cls, BaseARD) and issubclass(cls, SparsityStats)
        assert cls.__mro__[1] is torch.nn.Linear
    assert LinearL0.__sparsity_ignore__ == ("log_alpha",)
    assert LinearLASSO.__sparsity_ignore__ == ()
    assert (LinearL0.beta, LinearL0.gamma, LinearL0.zeta) == (0.66, -0.1, 1.1)


@pytest.mark.parametrize("group,shape", [(None, (7, 5)), ("input", (1, 5)), ("output", (7, 1)), ("other", (7, 5))])
def test_log_alpha_shape_follows_group(group, shape):
    from cplxmodule_amd.nn.relevance import LinearL0
    layer = LinearL0(5, 7, group=group)
    assert tuple(layer.log_alpha.shape) == shape
    assert layer.log_alpha.dtype == torch.float32
    assert torch.all(layer.log_alpha == torch.tensor(-2.197))


def test_shape_dispatch_case_has_a_row_shaped_log_alpha():
    """LinearL0(I, 1) with group None: log_alpha [1, I], which the forward treats as the input group."""
    from cplxmodule_amd.nn.relevance import LinearL0
    assert tuple(LinearL0(20, 1).log_alpha.shape) == (1, 20)
    assert tuple(LinearL0(1, 20).log_alpha.shape) == (20, 1)


def test_reset_variational_parameters():
    from cplxmodule_amd.nn.relevance import LinearL0
    layer = LinearL0(6, 4)
    with torch.no_grad():
        layer.log_alpha.uniform_(-1, 1)
    layer.reset_variational_parameters()
    assert torch.all(layer.log_alpha == torch.tensor(-2.197))


def _build(name, cfg):
    from cplxmodule_amd.nn.relevance import LinearL0, LinearLASSO
    cls, I, O, group, _ = cfg
    return LinearL0(I, O, group=group) if cls == "L0" else LinearLASSO(I, O)


CASES = {
    "none": ("L0", 20, 12, None, (6,)), "input": ("L0", 24, 12, "input", (2, 3)),
    "output": ("L0", 20, 16, "output", (2, 3)), "dispatch": ("L0", 20, 1, None, (5,)),
    "lasso": ("LASSO", 20, 12, None, (6,)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_state_dicts_travel_with_the_reference(golden, name):
    g = golden("l0")
    k = name + "_"
    layer = _build(name, CASES[name])
    keys = [str(s) for s in g[k + "sd_keys"]]
    ours = layer.state_dict()
    assert list(ours) == keys                                          # same keys, same order
    for kk in keys:
        ref = g[k + "sd_" + kk]
        assert tuple(ours[kk].shape) == ref.shape and str(ours[kk].dtype) == f"torch.{ref.dtype}"
    res = layer.load_state_dict({kk: torch.from_numpy(g[k + "sd_" + kk]) for kk in keys}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if "log_alpha" in keys:
        np.testing.assert_array_equal(layer.log_alpha.detach().numpy(), g[k + "sd_log_alpha"])
    # and back: a state dict of ours holds exactly what the reference module's load_state_dict(strict=True) expects
    for kk, v in layer.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g[k + "sd_" + kk])


def test_trajectory_fixture_handoffs_load_into_our_models(golden):
    """The recorded phase-start state dicts of both tracks load strictly into models built from this package."""
    from collections import OrderedDict
    from cplxmodule_amd.nn import masked, relevance as rel
    g = golden("l0")
    for track, cls1 in (("l0", rel.LinearL0), ("lasso", rel.LinearLASSO)):
        for ph, cls in ((1, cls1), (2, masked.LinearMasked)):
            model = torch.nn.Sequential(OrderedDict([("l1", cls(24, 10, bias=True)), ("act", torch.nn.LeakyReLU()),
                                                     ("l2", cls(10, 8, bias=False))]))
            k = f"traj_{track}_p{ph}_init_"
            state = {n[len(k):]: torch.from_numpy(v) for n, v in g.items() if n.startswith(k)}
            res = model.load_state_dict(state, strict=True)
            assert not res.missing_keys and not res.unexpected_keys


def test_new_entry_points_are_declared_and_bound():
    import re
    from cplxmodule_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cplxamd.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 25
    assert "#define CPLXAMD_ABI_VERSION 25" in src
    assert _lib.KL_KINDS["real_l0"] == 7 and _lib.KL_KINDS["real_l1"] == 8
    lib = ctypes.CDLL(os.path.join(ROOT, "cplxmodule_amd", "libcplxamd.so"))
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert _lib.load().cplxamd_abi_version() == 25


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from cplxmodule_amd import _lib
    lib = _lib.load()
    assert lib.cplxamd_l0_gate_fwd(None, None, None, 0, 0, None, None, None, 0, 0, 0, 0, 0, None, None, None) == -1
    assert lib.cplxamd_l0_gate_bwd(None, None, None, None, 0, 0, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, None, 0,
                                   None) == -1
    assert lib.cplxamd_l1_mask(None, 0.0, None, None, None, 0, None) == -1
    assert lib.cplxamd_philox_uniform(None, 0, 0, 4, None) == -1
    # the per-column backward's workspace: one float32 partial per column and row chunk
    assert lib.cplxamd_l0_gate_bwd_ws_bytes(8192, 4096) % (4 * 4096) == 0
    assert lib.cplxamd_l0_gate_bwd_ws_bytes(8192, 4096) > 0
    assert lib.cplxamd_l0_gate_bwd_ws_bytes(0, 16) == 0
    # a penalty kind past the last one is an argument error
    assert lib.cplxamd_vd_kl_fwd(None, None, None, 9, None, None, None, 0, None) == -1


def test_layers_refuse_cpu_tensors():
    from cplxmodule_amd._lib import CplxAmdError
    from cplxmodule_amd.nn.relevance import LinearL0, LinearLASSO
    with pytest.raises(CplxAmdError):
        LinearL0(4, 3).eval()(torch.randn(2, 4))
    with pytest.raises(CplxAmdError):
        LinearLASSO(4, 3).relevance(threshold=0.0)
