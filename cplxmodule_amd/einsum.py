"""cplx.einsum for two complex operands: a host planner and one autograd Function over csrc/einsum.hip.

Reference: cplxmodule/cplx.py:1032-1059 (re = E(ar, br) - E(ai, bi), im = E(ar, bi) + E(ai, br): no conjugation).

The planner is pure Python on shapes and strides (no GPU, no tensors):

  1. the equation is validated by torch's own parser on meta tensors (its messages, its output shape), then read into
     one list of labels per operand; `...` becomes the labels '.0' (rightmost), '.1', ...;
  2. per operand, a repeated label is a diagonal (its strides add up) and an extent-1 dimension of a label that is
     larger in the other operand is a broadcast: the label is dropped from that operand (`squeeze`), which makes it a
     free or summed index of the other one -- `operand_views` does both with torch views, so that autograd undoes them
     for free, and a broadcast operand's gradient is summed inside the kernel, rounded once;
  3. every label is a mode of one group: batch (A, B, out), M (A, out), N (B, out), K (not in out).  A label that lives
     in ONE operand only and not in the output is a K mode with stride 0 in the other operand: it is summed inside the
     product's float32 accumulator instead of by a separate reduction (which would round a bf16 operand a second time);
  4. extent-1 modes are dropped and two neighbours of a group are fused when they are adjacent in every tensor that
     carries the group; an empty group is one mode of extent 1; more than 8 modes in a group is an error;
  5. the route: 'cgemm' (no batch, exactly one M, N and K mode, C row-major: ops.cgemm on the plan's strides),
     'kernel' (cplxamd_ceinsum), 'f64' (float64: permute / reshape copies + f64.matmul_batched) or 'empty' (an
     extent 0: torch's own zero-work result).

Mode order inside a group never depends on the strides (output order for batch / M / N, order of appearance for K), so
the summation order, and with it every bit of the result, is the same for every layout of the operands.
"""
import os
import string
from dataclasses import dataclass

import torch

from . import f64, ops
from ._lib import CplxAmdError

MAX_MODES = 8
_LETTERS = set(string.ascii_letters)


@dataclass(frozen=True)
class Mode:
    """`extent` indices with ELEMENT strides sa / sb / sc in A / B / C; `labels`: the subscripts fused into it."""
    extent: int
    sa: int
    sb: int
    sc: int
    labels: str = ""


@dataclass(frozen=True)
class Plan:
    batch: tuple
    m: tuple
    n: tuple
    k: tuple
    out_shape: tuple
    conj_a: bool
    conj_b: bool
    route: str

    @property
    def groups(self):
        return (self.batch, self.m, self.n, self.k)


# ---------------------------------------------------------------------------------------------------------------- #
#  equation -> labels                                                                                              #
# ---------------------------------------------------------------------------------------------------------------- #
def validate(equation, shapes):
    """torch.einsum's verdict on (equation, shapes): raises what it raises, returns the output shape."""
    metas = [torch.empty(tuple(s), device="meta") for s in shapes]
    return tuple(torch.einsum(equation, *metas).shape)


def _term_labels(term, ndim):
    letters = [c for c in term.replace("...", "") if c in _LETTERS]
    if "..." not in term:
        return letters
    head = [c for c in term.split("...")[0] if c in _LETTERS]
    nell = ndim - len(letters)
    return head + [f".{j}" for j in range(nell - 1, -1, -1)] + letters[len(head):]


def parse(equation, shapes):
    """-> ([labels of operand 0, labels of operand 1], labels of the output); call `validate` first."""
    eq = equation.replace(" ", "")
    lhs, arrow, rhs = eq.partition("->")
    terms = lhs.split(",")
    ins = [_term_labels(t, len(s)) for t, s in zip(terms, shapes)]
    nell = max(sum(1 for lab in labs if lab[0] == ".") for labs in ins)
    ell = [f".{j}" for j in range(nell - 1, -1, -1)]
    if arrow:
        if "..." in rhs:
            head, _, tail = rhs.partition("...")
            out = list(head) + ell + list(tail)
        else:
            out = list(rhs)
    else:
        flat = [lab for labs in ins for lab in labs if lab[0] != "."]
        out = ell + sorted(lab for lab in set(flat) if flat.count(lab) == 1)
    return ins, out


def label_extents(ins, shapes):
    ext = {}
    for labs, shape in zip(ins, shapes):
        for lab, e in zip(labs, shape):
            if ext.get(lab, 1) == 1:
                ext[lab] = int(e)
    return ext


def normalize(labels, shape, strides, ext):
    """One operand's (labels, shape, strides) -> {label: stride} with unique labels: a repeated label is a diagonal
    (strides add); an extent-1 dimension of a label that is larger in the other operand is a broadcast: the operand does
    not depend on that label, so the label is dropped from it."""
    out = {}
    for lab, e, s in zip(labels, shape, strides):
        if e == 1 and ext[lab] != 1:
            continue
        out[lab] = out.get(lab, 0) + int(s)
    return out


def operand_views(t, labels, ext):
    """`normalize` with torch views (autograd undoes them): -> (view, unique labels in the view's dimension order)."""
    labels = list(labels)
    for d in reversed(range(len(labels))):
        if t.shape[d] == 1 and ext[labels[d]] != 1:
            t = t.squeeze(d)
            del labels[d]
    for lab in dict.fromkeys(labels):
        while labels.count(lab) > 1:
            d1 = labels.index(lab)
            d2 = labels.index(lab, d1 + 1)
            t = torch.diagonal(t, 0, d1, d2).movedim(-1, d1)
            del labels[d2]
    return t, labels


def contiguous_strides(shape):
    st, acc = [], 1
    for e in reversed(shape):
        st.append(acc)
        acc *= max(int(e), 1)
    return tuple(reversed(st))


# ---------------------------------------------------------------------------------------------------------------- #
#  labels + strides -> plan                                                                                        #
# ---------------------------------------------------------------------------------------------------------------- #
def _fuse(modes, carried):
    """drop extent-1 modes; fuse (outer, inner) neighbours that are adjacent in every tensor of `carried`"""
    out = []
    for md in modes:
        if md.extent == 1:
            continue
        if out:
            o = out[-1]
            if all(getattr(o, s) == getattr(md, s) * md.extent for s in carried):
                out[-1] = Mode(o.extent * md.extent, md.sa, md.sb, md.sc, o.labels + md.labels)
                continue
        out.append(md)
    return tuple(out) if out else (Mode(1, 0, 0, 0, ""),)


def gemm_route_enabled():
    return os.environ.get("CPLXAMD_EINSUM_GEMM", "1") != "0"


def contraction_plan(x_strides, y_strides, out_labels, ext, dtype=torch.float32, conj=(False, False)):
    """x_strides / y_strides: {label: element stride} of the two operands (unique labels), `ext`: {label: extent}.
    C is contiguous in `out_labels` order."""
    out_shape = tuple(ext[lab] for lab in out_labels)
    c_strides = dict(zip(out_labels, contiguous_strides(out_shape)))
    groups = {"batch": [], "m": [], "n": [], "k": []}
    show = lambda lab: "." if lab[0] == "." else lab  # noqa: E731

    def mode(lab):
        return Mode(ext[lab], x_strides.get(lab, 0), y_strides.get(lab, 0), c_strides.get(lab, 0), show(lab))

    for lab in out_labels:
        in_x, in_y = lab in x_strides, lab in y_strides
        groups["batch" if in_x and in_y else "n" if in_y else "m"].append(mode(lab))
    for lab in list(x_strides) + [lab for lab in y_strides if lab not in x_strides]:
        if lab not in c_strides:
            groups["k"].append(mode(lab))
    fused = {"batch": _fuse(groups["batch"], ("sa", "sb", "sc")), "m": _fuse(groups["m"], ("sa", "sc")),
             "n": _fuse(groups["n"], ("sb", "sc")), "k": _fuse(groups["k"], ("sa", "sb"))}
    for name, g in fused.items():
        if len(g) > MAX_MODES:
            raise CplxAmdError(f"einsum: the {name} group has {len(g)} modes after fusion; the contraction kernel takes at "
                               f"most {MAX_MODES} per group (make the operands contiguous in fewer index runs)")
        p = 1
        for md in g:
            p *= md.extent
        if p >= 2 ** 31:
            raise CplxAmdError(f"einsum: the {name} group spans {p} indices; the contraction kernel takes 2^31 - 1")
    numel = 1
    for e in out_shape:
        numel *= e
    real = lambda g: [md for md in g if md.extent > 1]  # noqa: E731
    ktot = 1
    for md in fused["k"]:
        ktot *= md.extent
    if numel == 0 or ktot == 0:
        route = "empty"
    elif dtype == torch.float64:
        route = "f64"
    elif (gemm_route_enabled() and not real(fused["batch"]) and len(real(fused["m"])) == 1 and len(real(fused["n"])) == 1
          and len(real(fused["k"])) == 1 and fused["n"][0].sc == 1 and fused["m"][0].sc == fused["n"][0].extent
          and fused["m"][0].sa and fused["k"][0].sa and fused["n"][0].sb and fused["k"][0].sb):     # (a broadcast operand: the kernel)
        route = "cgemm"
    else:
        route = "kernel"
    return Plan(fused["batch"], fused["m"], fused["n"], fused["k"], out_shape, bool(conj[0]), bool(conj[1]), route)


def plan(equation, shapes, strides=None, dtype=torch.float32):
    """The plan of `cplx.einsum(equation, a, b)` from shapes and ELEMENT strides alone (None: contiguous operands)."""
    shapes = [tuple(int(e) for e in s) for s in shapes]
    if len(shapes) != 2:
        raise CplxAmdError("einsum.plan describes the product of two operands")
    validate(equation, shapes)
    if strides is None:
        strides = [contiguous_strides(s) for s in shapes]
    ins, out = parse(equation, shapes)
    ext = label_extents(ins, shapes)
    xs, ys = (normalize(labs, s, st, ext) for labs, s, st in zip(ins, shapes, strides))
    return contraction_plan(xs, ys, out, ext, dtype)


# ---------------------------------------------------------------------------------------------------------------- #
#  execution                                                                                                       #
# ---------------------------------------------------------------------------------------------------------------- #
def _same_layout(r, i):
    """one stride vector serves both planes of an operand; planes laid out differently are copied (rare: a Cplx built
    from two unrelated tensors)"""
    if r.stride() != i.stride():
        return r.contiguous(), i.contiguous()
    return r, i


def _contract(xr, xi, yr, yi, spec):
    """out[ol] = sum conj^cx(X)[xl] conj^cy(Y)[yl]; X, Y with unique labels, any strides; -> contiguous planes."""
    xl, yl, ol, ext, cx, cy = spec
    ext = dict(ext)
    xr, xi = _same_layout(xr, xi)
    yr, yi = _same_layout(yr, yi)
    p = contraction_plan(dict(zip(xl, xr.stride())), dict(zip(yl, yr.stride())), ol, ext, xr.dtype, (cx, cy))
    if p.route == "cgemm":
        m, n, k = p.m[0], p.n[0], p.k[0]
        cr, ci = ops.cgemm(xr, xi, (m.sa, k.sa), yr, yi, (n.sb, k.sb), m.extent, n.extent, k.extent,
                           conj_b=(cx != cy), out_dtype=xr.dtype)
        if cx:                       # conj(A) op(B) = conj(A conj(op(B)))
            ci = -ci
        return cr.view(p.out_shape), ci.view(p.out_shape)
    if p.route != "kernel":
        raise CplxAmdError(f"einsum: internal error, route '{p.route}' reached the kernel launcher")
    return ops.ceinsum(xr, xi, yr, yi, p)


class ContractFn(torch.autograd.Function):
    """One launch forward; backward = two more contractions of the same kind with the groups re-labelled and the
    conjugation flags set (dX in X's label order, dY in Y's), through this Function itself under create_graph."""

    @staticmethod
    def forward(ctx, xr, xi, yr, yi, spec):
        ctx.spec = spec
        ctx.save_for_backward(xr, xi, yr, yi)
        return _contract(xr.detach(), xi.detach(), yr.detach(), yi.detach(), spec)

    @staticmethod
    def backward(ctx, gr, gi):
        xr, xi, yr, yi = ctx.saved_tensors
        xl, yl, ol, ext, cx, cy = ctx.spec
        if torch.is_grad_enabled():
            run = ContractFn.apply
        else:
            run = lambda *a: _contract(*(t.detach() for t in a[:4]), a[4])  # noqa: E731
        dxr = dxi = dyr = dyi = None
        need = ctx.needs_input_grad
        if need[0] or need[1]:
            # cx = 0: dX = G conj(op(Y));  cx = 1: dX = conj(G) op(Y)
            dxr, dxi = run(gr, gi, yr, yi, (ol, yl, xl, ext, cx, cy if cx else not cy))
        if need[2] or need[3]:
            # cy = 0: dY = conj(op(X)) G;  cy = 1: dY = op(X) conj(G)
            dyr, dyi = run(xr, xi, gr, gi, (xl, ol, yl, ext, cx if cy else not cx, cy))
        return (dxr if need[0] else None, dxi if need[1] else None, dyr if need[2] else None,
                dyi if need[3] else None, None)


def _f64_product(xr, xi, xl, yr, yi, yl, ol, ext):
    """float64: the checking route of Cplx.__matmul__ -- permute / reshape copies to [Z, M, K] @ [Z, K, N]."""
    only_x = [lab for lab in xl if lab not in yl and lab not in ol]
    only_y = [lab for lab in yl if lab not in xl and lab not in ol]
    if only_x:
        dims = [xl.index(lab) for lab in only_x]
        xr, xi, xl = xr.sum(dims), xi.sum(dims), [lab for lab in xl if lab not in only_x]
    if only_y:
        dims = [yl.index(lab) for lab in only_y]
        yr, yi, yl = yr.sum(dims), yi.sum(dims), [lab for lab in yl if lab not in only_y]
    b = [lab for lab in ol if lab in xl and lab in yl]
    m = [lab for lab in ol if lab in xl and lab not in yl]
    n = [lab for lab in ol if lab in yl and lab not in xl]
    k = [lab for lab in xl if lab in yl and lab not in ol]
    size = lambda labs: [ext[lab] for lab in labs]  # noqa: E731
    prod = lambda labs: int(torch.Size(size(labs)).numel())  # noqa: E731
    Z, M, N, K = prod(b), prod(m), prod(n), prod(k)
    px = lambda t: t.permute([xl.index(lab) for lab in b + m + k]).reshape(Z, M, K)  # noqa: E731
    py = lambda t: t.permute([yl.index(lab) for lab in b + k + n]).reshape(Z, K, N)  # noqa: E731
    cr, ci = f64.matmul_batched(px(xr), px(xi), py(yr), py(yi))
    bmn = b + m + n
    back = [bmn.index(lab) for lab in ol]
    return cr.reshape(size(bmn)).permute(back), ci.reshape(size(bmn)).permute(back)


def einsum2(equation, ar, ai, br, bi):
    """Planes of cplx.einsum(equation, a, b); the operands were checked by the caller (HIP device, one dtype)."""
    shapes = [tuple(ar.shape), tuple(br.shape)]
    out_shape = validate(equation, shapes)
    ins, ol = parse(equation, shapes)
    ext = label_extents(ins, shapes)
    if tuple(ext[lab] for lab in ol) != out_shape:
        raise CplxAmdError(f"einsum: internal error, planned output shape differs from torch's for '{equation}'")
    if 0 in out_shape or 0 in ext.values():
        # nothing to multiply: torch's own (differentiable) empty / zero result
        return (torch.einsum(equation, ar, br) - torch.einsum(equation, ai, bi),
                torch.einsum(equation, ar, bi) + torch.einsum(equation, ai, br))
    (xr, xl), (xi, _) = operand_views(ar, ins[0], ext), operand_views(ai, ins[0], ext)
    (yr, yl), (yi, _) = operand_views(br, ins[1], ext), operand_views(bi, ins[1], ext)
    if ar.dtype == torch.float64:
        return _f64_product(xr, xi, xl, yr, yi, yl, ol, ext)
    spec = (tuple(xl), tuple(yl), tuple(ol), tuple(ext.items()), False, False)
    return ContractFn.apply(xr, xi, yr, yi, spec)
