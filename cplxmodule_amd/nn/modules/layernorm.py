"""CplxLayerNorm: complex layer normalisation on the fused per-row kernel (cplx.layer_norm)."""
import torch

from .base import CplxToCplx
from ... import cplx


class CplxLayerNorm(CplxToCplx):
    """Normalises a `Cplx` input over its last `len(normalized_shape)` dims: `kind="whiten"` whitens the row's 2 x 2
    covariance of (Re, Im), the convention of `CplxBatchNorm*d`; `"modulus"` divides by the row's RMS modulus.  With
    `elementwise_affine`, `weight` [2, 2, *normalized_shape] (initialised to I2) and `bias` [2, *normalized_shape] (0)
    apply out = W y + B per feature; both are float32 parameters for every activation dtype.  There are no running
    statistics: training and evaluation do not differ."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, kind="whiten"):
        super().__init__()
        ns = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
        if kind not in ("whiten", "modulus"):
            raise ValueError(f"unknown kind {kind!r}; one of ('whiten', 'modulus')")
        self.normalized_shape, self.eps, self.elementwise_affine, self.kind = ns, eps, elementwise_affine, kind
        if elementwise_affine:
            self.weight = torch.nn.Parameter(torch.empty(2, 2, *ns))
            self.bias = torch.nn.Parameter(torch.empty(2, *ns))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.elementwise_affine:
            with torch.no_grad():
                self.weight.copy_(torch.eye(2).reshape(2, 2, *(1,) * len(self.normalized_shape)))
                self.bias.zero_()

    def forward(self, input):
        return cplx.layer_norm(input, self.normalized_shape, self.weight, self.bias, self.eps, self.kind)

    def extra_repr(self):
        return (f"{self.normalized_shape}, eps={self.eps}, elementwise_affine={self.elementwise_affine}, "
                f"kind={self.kind!r}")
