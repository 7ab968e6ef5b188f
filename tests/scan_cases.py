"""The plain statement of the recurrence behind cplx.linear_recurrence that tests/test_scan_host.py and
tests/test_gpu_scan.py compare against: a loop over t in float64 / complex128 torch on the CPU, vectorised over rows."""
import torch


def reference(a, x, h0=None, reverse=False, conj=False, lag=False):
    """h[p] = c[p] h[p - 1] + x[p] in processing order (reverse: from the last sample); c[p] is a at step p, conjugated
    under `conj`; under `lag` a at step p - 1, and nothing enters step 0.  a [..., T or 1], x [..., T], h0 [...]."""
    a = (a.conj() if conj else a).expand(x.shape)
    h = torch.zeros_like(x[..., 0]) if h0 is None else h0.expand(x.shape[:-1])
    steps = range(x.shape[-1])[::-1] if reverse else range(x.shape[-1])
    out, before = [], None
    for t in steps:
        h = (a[..., t] if not lag else a[..., before] if before is not None else 0) * h + x[..., t]
        out.append(h)
        before = t
    return torch.stack(out[::-1] if reverse else out, -1)


def z(pr, pi=None):
    """planes as the kernel received them -> float64 (both None imaginary) or complex128 on the CPU"""
    pr = pr.detach().double().cpu()
    return pr if pi is None else torch.complex(pr, pi.detach().double().cpu())
