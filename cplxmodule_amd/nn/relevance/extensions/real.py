"""LinearL0 and LinearLASSO (cplxmodule/nn/relevance/extensions/real/ell_zero.py, lasso.py) on the real GEMM, the gate
kernels of csrc/l0.hip and the `real_l0` / `real_l1` penalty kinds of csrc/kl.hip.  Same parameters, state-dict keys,
defaults and numbers as the reference; the uniforms of the L0 gate come from the package's noise source (noise.py)."""
import torch

from ..base import BaseARD
from ..noise import noise
from ...utils.sparsity import SparsityStats
from .... import l0 as _l0
from .... import ops


def _draw_uniform(shape, device):
    """(u or None, seed, offset) for one stochastic forward: u in the reference's layout for the "torch" / "tape" modes,
    else the Philox stream position (a device tensor in "philox-device" mode)."""
    if noise.mode == "torch":
        return torch.rand(*shape, dtype=torch.float32, device=device), 0, 0
    if noise.mode == "tape":
        return noise.pop_tape(shape, torch.empty(0, dtype=torch.float32, device=device), False), 0, 0
    seed, offset = noise.next(device)
    return None, seed, offset


class LinearL0(torch.nn.Linear, BaseARD, SparsityStats):
    """L0 regularised linear layer (Louizos, Welling, Kingma, ICLR 2018) in the reference's -ve log-alpha
    parametrisation: a hard-concrete gate z on every weight (group None), on every input feature ("input") or on every
    output ("output"), drawn once per batch for the weights and once per sample for the groups."""

    __sparsity_ignore__ = ("log_alpha",)

    beta, gamma, zeta = 0.66, -0.1, 1.1

    def __init__(self, in_features, out_features, bias=True, group=None):
        super().__init__(in_features, out_features, bias=bias)
        if group == "input":
            shape = 1, in_features
        elif group == "output":
            shape = out_features, 1
        else:
            shape = out_features, in_features
        self.log_alpha = torch.nn.Parameter(torch.empty(*shape))
        self.reset_variational_parameters()

    def reset_variational_parameters(self):
        # log alpha ~ log p - log(1 - p) for the dropout rate p = 0.9 (ell_zero.py:66-69)
        self.log_alpha.data.fill_(-2.197)

    @property
    def penalty(self):
        """P(z != 0) = sigmoid(-beta log(-gamma / zeta) - log_alpha), elementwise."""
        return _l0.OneParamPenaltyFn.apply("real_l0", _l0.check_param(self.log_alpha))

    def _penalty_reduced(self, reduction):
        total = _l0.OneParamPenaltySumFn.apply("real_l0", _l0.check_param(self.log_alpha))
        return total / self.log_alpha.numel() if reduction == "mean" else total

    def forward(self, input):
        # the branch follows the SHAPE of log_alpha, n == 1 first (ell_zero.py:92, :121-132)
        n, m = self.log_alpha.shape
        la = _l0.check_param(self.log_alpha)
        lead = input.shape[:-1]
        if n == 1:
            fn, shape = _l0.L0InputLinearFn, (*lead, 1, m)
        elif m == 1:
            fn, shape = _l0.L0OutputLinearFn, (*lead, n, 1)
        else:
            fn, shape = _l0.L0LinearFn, (n, m)
        u, seed, offset = _draw_uniform(shape, input.device) if self.training else (None, 0, 0)
        return fn.apply(input, self.weight, self.bias, la, u, seed, offset, self.training)

    def _gate_mask(self, hard, total=False):
        la = _l0.check_param(self.log_alpha)
        return _l0.gate_fwd(None, la, 1, la.numel(), _l0.HARD if hard else 0, out_dtype=self.weight.dtype,
                            total=total)

    def relevance(self, *, hard, **kwargs):
        """The eval gate (hard: gate > 0) expanded to the weight's shape; `threshold` is not used (ell_zero.py:156-165)."""
        with torch.no_grad():
            return self._gate_mask(hard).view(self.log_alpha.shape).expand_as(self.weight)

    def sparsity(self, *, hard, **kwargs):
        with torch.no_grad():
            _, kept = self._gate_mask(hard, total=True)
        n_relevant = float(kept.item()) * (self.weight.numel() // self.log_alpha.numel())
        return [(id(self.weight), self.weight.numel() - n_relevant)]


class LinearLASSO(torch.nn.Linear, BaseARD, SparsityStats):
    """Linear layer with the L1 penalty |W| (lasso.py)."""

    def forward(self, input):
        return ops.RealLinearFn.apply(input, self.weight, self.bias)

    @property
    def penalty(self):
        return _l0.OneParamPenaltyFn.apply("real_l1", _l0.check_param(self.weight))

    def _penalty_reduced(self, reduction):
        total = _l0.OneParamPenaltySumFn.apply("real_l1", _l0.check_param(self.weight))
        return total / self.weight.numel() if reduction == "mean" else total

    def relevance(self, *, threshold, **kwargs):
        """log(|w| + 1e-20) >= threshold, a bool tensor (lasso.py:11-14)."""
        with torch.no_grad():
            return _l0.l1_mask(_l0.check_param(self.weight), threshold)

    def sparsity(self, *, threshold, **kwargs):
        with torch.no_grad():
            _, kept = _l0.l1_mask(_l0.check_param(self.weight), threshold, count=True)
        return [(id(self.weight), self.weight.numel() - float(kept.item()))]
