"""The batch-run layer of the signal kernels (fft, rfft, fftconv, upfirdn, iir, filtfilt): pure host code, no launches,
importable without the library or a GPU.

A kernel transforms or filters along ONE dim and reads every other dim where it lies: those dims are sorted by the
result's stride and fused, jointly for every tensor of the call, into batch runs [size, stride per tensor ...] (`runs`).
A descriptor holds at most MAX_RUNS of them (csrc/runs.h decodes them).  Operands that need more are copied once,
differentiably, in an order each caller fixes (`fit`; `fit_like` for the one operand of a transform, `fit_wgrad` for a
weight gradient); `fill` writes the runs into a ctypes descriptor.
"""
import functools

import torch

from . import _lib
from ._lib import CplxAmdError

MAX_RUNS = 3
code = functools.partial(_lib.plane_code, "fft: planes must be float32, bfloat16 or float64")


def planes(x, name, fn):
    from .cplx import Cplx
    if isinstance(x, Cplx):
        pr, pi = x.real, x.imag
        if pr.dtype != pi.dtype:
            raise CplxAmdError(f"{fn}: the planes of `{name}` have different dtypes: {pr.dtype} and {pi.dtype}")
        return pr, pi
    if torch.is_tensor(x) and not x.is_complex():
        return x, None
    raise CplxAmdError(f"{fn}: `{name}` is a {type(x).__name__}{' of complex dtype' if torch.is_tensor(x) else ''}, "
                       "not a Cplx or a real torch.Tensor (wrap planes with Cplx(re, im); torch complex tensors are not taken)")


def runs(shape, strides, skip=-1):
    """the dims of `shape` other than `skip` as runs [size, stride per tensor ...], outermost first: sorted by the LAST
    tensor's strides (the result's) and fused where every tensor allows it"""
    skip %= len(shape)
    of = list(zip(*strides))                              # of[d]: the stride of dim d in every tensor
    dims = sorted((d for d in range(len(shape)) if d != skip and shape[d] != 1), key=lambda d: of[d][::-1], reverse=True)
    out = []
    for d in dims:
        if out and out[-1][1:] == [s * shape[d] for s in of[d]]:
            out[-1] = [out[-1][0] * shape[d], *of[d]]
        else:
            out.append([shape[d], *of[d]])
    return out


def dense(shape):
    strides, acc = [0] * len(shape), 1
    for d in reversed(range(len(shape))):
        strides[d] = acc
        acc *= max(shape[d], 1)
    return strides


def dense_like(t, dim, n):
    """(shape, strides) of the output for input plane t: t's shape with `n` along `dim`, dense, in t's memory order
    (what empty_like gives a dense t)"""
    shape, of = list(t.shape), t.stride()
    shape[dim] = n
    order = sorted(range(len(of)), key=lambda d: (-of[d], d))
    strides, acc = [0] * len(of), 1
    for d in reversed(order):
        strides[d] = acc
        acc *= max(shape[d], 1)
    return shape, strides


def share(pr, pi):
    """planes of one operand must share a layout"""
    if pi is not None and pr.stride() != pi.stride():
        return pr.contiguous(), pi.contiguous()
    return pr, pi


def _over(t, shape):
    """t broadcast over the batch dims of `shape` (all but the last; t keeps its own extent there and behind), as a view"""
    over = tuple(shape[:-1]) + tuple(t.shape[len(shape) - 1:])
    return t if t.shape == over else t.expand(over)


def fit(shape, operands, ys, order):
    """Fit a call along the last dim into MAX_RUNS runs.  `operands`: plane pairs (re, im or None), each broadcastable
    over the batch dims of `shape`; `ys`: the result's strides; `order`: tuples of operand indices, the operands that
    may be copied and in which order.  The planes of an operand are brought to one layout, then one tuple after the other
    is replaced by dense copies of its broadcast expansion (differentiable) until the runs fit -> (operands, runs); more
    than MAX_RUNS runs are left only by the broadcast pattern of what `order` does not name."""
    ops = [share(*p) for p in operands]
    for step in (*order, None):
        out = runs(shape, [_over(pr, shape).stride() for pr, _ in ops] + [ys])
        if step is None or len(out) <= MAX_RUNS:
            return ops, out
        for i in step:
            ops[i] = tuple(None if t is None else _over(t, shape).contiguous() for t in ops[i])


def fit_like(pr, pi, dim, n):
    """`fit` for a transform along `dim` of one operand (pi may be None) whose result has n entries there and is dense in
    the operand's memory order, so that its strides follow the operand's -> (pr, pi, runs, the result's strides)"""
    pr, pi = share(pr, pi)
    for last in (False, True):
        ys = dense_like(pr, dim, n)[1]
        out = runs(pr.shape, (pr.stride(), ys), dim)
        if last or len(out) <= MAX_RUNS:
            return pr, pi, out, ys
        pr, pi = pr.contiguous(), None if pi is None else pi.contiguous()


def fit_wgrad(a, c, k, fshape):
    """`fit` for a weight gradient: plane pairs a [*B, A] and c [*B, C] (copied together), results [*fshape, k] that
    the kernel sums over the rows fshape broadcasts over -> (a, c, runs, fshape to launch with): B itself when the
    broadcast pattern alone needs too many runs (per-row results, for the caller to `sum_to_size`)"""
    batch = tuple(a[0].shape[:-1])
    shape = batch + (k,)
    for f in (tuple(fshape), batch):
        ys = torch.empty(f + (k,), device="meta").expand(shape).stride()
        (a, c), out = fit(shape, [a, c], ys, [(0, 1)])
        if len(out) <= MAX_RUNS:
            break
    return a, c, out, f


def fill(desc, runs, fields, key=None):
    """write the runs into a descriptor: run r's size into desc.size[r] and its strides into the arrays named by
    `fields` (in the runs' column order), their number into desc.runs -> (rows, filters): the product of all sizes, and
    of the sizes of the runs whose stride in the array named `key` is not zero (1 without a key).  Whatever a run leaves
    out, or the descriptor has no run for, stays zero."""
    desc.runs = len(runs)
    arrays = [desc.size] + [getattr(desc, f) for f in fields]
    col = 0 if key is None else fields.index(key) + 1
    rows = filters = 1
    for r, run in enumerate(runs):
        for a, v in zip(arrays, run):
            a[r] = v
        rows *= run[0]
        if col and run[col] != 0:
            filters *= run[0]
    return rows, filters
