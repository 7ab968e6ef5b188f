"""Strided views into interleaved complex data (cplxmodule/utils/views.py:5-63)."""
import warnings

import torch


def fix_dim(dim, n_dim):
    """non-negative axis index, ValueError when out of range"""
    axis = dim + n_dim if dim < 0 else dim
    if not 0 <= axis < n_dim:
        raise ValueError(f"Dimension {dim} is out of range for {n_dim}.")
    return axis


def complex_view(x, dim=-1, squeeze=True):
    """(real, imag) views of a tensor holding re/im interleaved along `dim`: no copy, autograd
    flows into `x`.  A `dim` of size exactly 2 is dropped when `squeeze`; an odd size loses its
    last element (with a RuntimeWarning)."""
    dim = fix_dim(dim, x.dim())
    n = x.shape[dim]
    if n % 2:
        warnings.warn("Odd dimension size for the complex data unpacking: taking the least size "
                      "that fits.", RuntimeWarning)
    if n == 2 and squeeze:
        return x.select(dim, 0), x.select(dim, 1)
    even = x.narrow(dim, 0, n - n % 2)
    index = [slice(None)] * x.dim()
    index[dim] = slice(0, None, 2)
    real = even[tuple(index)]
    index[dim] = slice(1, None, 2)
    return real, even[tuple(index)]


def window_view(x, dim, size, stride, at=None):
    """Sliding-window view (cplxmodule/utils/views.py:66-121): like `x.unfold(dim, size, stride)`, but the window
    dimension of `size` goes to `at` (default: right after `dim`) instead of last.  A pure `as_strided` view: no copy,
    autograd flows into `x`.  ValueError for size <= 0, stride < 0, an out-of-range dim or a too short x."""
    if size <= 0:
        raise ValueError("`size` must be a positive integer.")
    if stride < 0:
        raise ValueError("`stride` must be a nonnegative integer.")
    dim = fix_dim(dim, x.dim())
    if x.shape[dim] < size:
        raise ValueError(f"`x` at dim {dim} is too short ({x.shape[dim]}) for this window size ({size}).")
    at = fix_dim(dim + 1 if at is None else at, x.dim() + 1)
    shape, strides = list(x.size()), list(x.stride())
    count = ((shape[dim] - size + 1) + stride - 1) // stride
    shape_view = shape[:dim] + [count] + shape[dim + 1:]
    shape_view.insert(at, size)
    strides_view = strides[:dim] + [strides[dim] * stride] + strides[dim + 1:]
    strides_view.insert(at, strides[dim])
    return torch.as_strided(x, shape_view, strides_view)
