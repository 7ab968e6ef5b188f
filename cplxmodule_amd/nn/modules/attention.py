"""CplxMultiheadAttention: complex multi-head attention on the fused flash kernel (cplx.scaled_dot_product_attention)."""
from .base import CplxToCplx
from .linear import CplxLinear
from ... import cplx


class CplxMultiheadAttention(CplxToCplx):
    """Batch-first multi-head attention of `Cplx` inputs [B, L, embed_dim]: four `CplxLinear` projections (`q_proj`,
    `k_proj`, `v_proj`, `out_proj`) around `cplx.scaled_dot_product_attention` with the scores `score` ("real":
    softmax(Re q k^H / sqrt(d)), "abs": softmax(|q k^H| / sqrt(d))).  The heads are split and merged by views only: the
    kernel reads the `[B, L, H, d]` projections in place as `[B, H, L, d]` and writes its result in the same memory order.
    Attention weights are never materialised and not returned."""

    def __init__(self, embed_dim, num_heads, bias=True, score="real"):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError(f"embed_dim = {embed_dim} is not divisible by num_heads = {num_heads}")
        if score not in ("real", "abs"):
            raise ValueError(f"unknown score {score!r}; one of ('real', 'abs')")
        self.embed_dim, self.num_heads, self.score = embed_dim, num_heads, score
        self.q_proj = CplxLinear(embed_dim, embed_dim, bias=bias)
        self.k_proj = CplxLinear(embed_dim, embed_dim, bias=bias)
        self.v_proj = CplxLinear(embed_dim, embed_dim, bias=bias)
        self.out_proj = CplxLinear(embed_dim, embed_dim, bias=bias)

    def _heads(self, x):
        shape = x.real.shape[:-1] + (self.num_heads, self.embed_dim // self.num_heads)
        return cplx.Cplx(x.real.view(shape).transpose(1, 2), x.imag.view(shape).transpose(1, 2))

    def forward(self, query, key=None, value=None, is_causal=False):
        key = query if key is None else key
        value = key if value is None else value
        q, k, v = self._heads(self.q_proj(query)), self._heads(self.k_proj(key)), self._heads(self.v_proj(value))
        o = cplx.scaled_dot_product_attention(q, k, v, is_causal=is_causal, score=self.score)
        shape = query.real.shape[:-1] + (self.embed_dim,)
        merged = cplx.Cplx(o.real.transpose(1, 2).reshape(shape), o.imag.transpose(1, 2).reshape(shape))
        return self.out_proj(merged)

    def extra_repr(self):
        return f"embed_dim={self.embed_dim}, num_heads={self.num_heads}, score={self.score!r}"
