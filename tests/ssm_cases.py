"""The plain statement of the primitive behind cplx.ssm_scan that tests/test_ssm_host.py and tests/test_gpu_ssm.py compare
against: the float64 loop of tests/scan_cases.py applied per state, then the read-out."""
import torch

from scan_cases import reference


def loop(a, b, c, x, dt=None, h0=None, reverse=False, conj=False, lag=False, dt_out=False):
    """a, b, c [..., N, T or 1], x and dt [..., T], h0 [..., N], float64 or complex128 on the CPU -> (y [..., T], the
    state after the last processed step [..., N], h [..., N, T]).  h_n = reference(A_n, b_n X, h0_n), y = sum_n c_n h_n
    with A = a or exp(dt a); under `lag` h0 enters step 0 unscaled, which the scan's loop spells as an input there."""
    A = a if dt is None else torch.exp(dt.unsqueeze(-2) * a)
    X = x if dt is None or dt_out else dt * x
    b, c = (b.conj(), c.conj()) if conj else (b, c)
    u = b * X.unsqueeze(-2)
    u = u.expand(torch.broadcast_shapes(u.shape, A.shape, c.shape)).clone()
    first, last = (-1, 0) if reverse else (0, -1)
    if lag and h0 is not None:
        u[..., first] += h0
        h0 = None
    h = reference(A, u, h0 if h0 is None else h0.expand(u.shape[:-1]), reverse, conj, lag)
    y = (c * h).sum(-2)
    return (dt * y if dt is not None and dt_out else y), h[..., last], h
