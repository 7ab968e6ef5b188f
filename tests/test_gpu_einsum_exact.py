"""The contraction kernel behind cplx.einsum (csrc/einsum.hip), bit-exactly: integer-valued operands
(einsum_exact_cases.py) make every launch's result independent of the tile, the load path and the K staging, so both output
planes must EQUAL the int64 reference (float32) or its one round-to-nearest-even (bf16) over the whole tensor -- gradients
included -- and cplxamd_ceinsum must be the entry point that ran, on the load paths, swap state and tile the table names
(cplxamd_einsum_plan on the ACTUAL pointers): a case that falls to another path fails.  The operands are strided views into
NaN-filled buffers, the outputs are NaN before the launch, and the gaps of a padded C hold a canary that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import einsum_exact_cases as X
import gemm_exact_cases as G
from einsum_exact_cases import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENTRY = "cplxamd_ceinsum"
COMPUTE = G.COMPUTE | {ENTRY}


class Recorder:
    """A recording wrapper around `call` of ops.py: (entry point, returned success, arguments) per call."""

    def __init__(self, monkeypatch):
        from cplxmodule_amd import ops, _lib
        self.log = []

        def call(name, *a):
            try:
                _lib.call(name, *a)
            except Exception:
                self.log.append((name, False, a))
                raise
            self.log.append((name, True, a))

        def try_call(name, *a):
            ok = _lib.try_call(name, *a)
            self.log.append((name, bool(ok), a))
            return ok

        self.call = call
        monkeypatch.setattr(ops, "call", call)
        monkeypatch.setattr(ops, "try_call", try_call)

    def ran(self):
        """The compute entry points that ran and returned success, once per call."""
        return [n for n, ok, _ in self.log if ok and n in COMPUTE]

    def failed(self):
        return sorted({n for n, ok, _ in self.log if not ok})

    def dispatch(self, k=0):
        """cplxamd_einsum_plan on the pointers, descriptor and dtype of the k-th cplxamd_ceinsum call."""
        from cplxmodule_amd import ops
        a = [a for n, _, a in self.log if n == ENTRY][k]
        r = ops.einsum_dispatch(a[6]._obj, [p.value for p in a[:4]], a[9])
        return (r["mode_a"], r["mode_b"], r["swapped"], r["tile"])


@pytest.fixture
def nan_outputs():
    """torch.empty returns NaN while this holds: the planes ops.ceinsum allocates are NaN before the launch, so an element
    the kernel does not write cannot hold the right value by accident."""
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.utils.deterministic.fill_uninitialized_memory)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        assert bool(torch.empty(4096, device=DEV).isnan().all()) and bool(torch.empty(4096, dtype=torch.bfloat16, device=DEV).isnan().all())
        yield
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        torch.utils.deterministic.fill_uninitialized_memory = before[2]


def _operands(c, d):
    """-> ({ar, ai, br, bi: the view the case's storage describes, on the device}, {...: its NaN-filled buffer}), with the
    case's NaNs placed."""
    dt = X.TORCH_DTYPE[c["dtype"]]
    out, bufs = {}, {}
    for op, lay in (("a", c["la"]), ("b", c["lb"])):
        for p in "ri":
            bufs[op + p], out[op + p] = X.build_view(torch.from_numpy(d[op + p]).to(DEV), lay, dt, DEV)
    if c["poison"]:
        out["ar"][c["poison"]["a"]] = float("nan")
        out["bi"][c["poison"]["b"]] = float("nan")
    return out, bufs


def _leaves(c, v):
    """Gradient cases: the leaves (an expanded operand's leaf is its unexpanded base) and the operands made of them."""
    leaves, ops_ = {}, {}
    for k, t in v.items():
        lay = c["la"] if k[0] == "a" else c["lb"]
        base = t[tuple(slice(0, 1) if ax in lay["expand"] else slice(None) for ax in range(t.dim()))]
        leaves[k] = base.detach().requires_grad_(True)
        assert leaves[k].stride() == base.stride()
        ops_[k] = leaves[k].expand(t.shape) if lay["expand"] else leaves[k]
    return leaves, ops_


def _run_cabi(c, v, rec):
    """cplxamd_ceinsum directly, on the case's own descriptor: -> (C planes as views, their buffers)."""
    from cplxmodule_amd import ops, _lib
    p, a0, b0, _ = X.cabi_plan(c)
    dt = X.TORCH_DTYPE[c["dtype"]]
    shape = X.out_shape(c)
    bufs, views = [], []
    for _ in "ri":
        buf, view = X.build_view(torch.zeros(shape, device=DEV), c["cabi"]["c"], dt, DEV, fill=X.CANARY)
        view.fill_(float("nan"))
        bufs.append(buf)
        views.append(view)
    es = X.ESIZE[c["dtype"]]
    # the base pointers: the first element of the view, moved to the other end of every dimension whose stride is negated
    base = lambda t, lay_off, off: ctypes.c_void_p(t.data_ptr() + (off - lay_off) * es)  # noqa: E731
    pa = [base(v["a" + q], c["la"]["off"], a0) for q in "ri"]
    pb = [base(v["b" + q], c["lb"]["off"], b0) for q in "ri"]
    code = {"f32": _lib.F32, "bf16": _lib.BF16}[c["dtype"]]
    d = ops.einsum_desc(p)
    for g, modes in enumerate(p.groups):
        assert d.nmodes[g] == len(modes)                     # (an empty group stays empty: nmodes == 0)
    with torch.cuda.device(views[0].device):
        rec.call(ENTRY, pa[0], pa[1], pb[0], pb[1], _lib.ptr(views[0]), _lib.ptr(views[1]), ctypes.byref(d), int(c["conj"][0]),
                 int(c["conj"][1]), code, code, _lib.stream_ptr())
    return views, bufs


def _gaps(buf, view):
    """What of `buf` lies between the elements of `view` (a stride-0 dimension is marked once)."""
    mark = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    once = view[tuple(slice(0, 1) if st == 0 else slice(None) for st in view.stride())]
    mark.as_strided(once.shape, once.stride(), once.storage_offset()).fill_(True)
    assert int(mark.sum()) == once.numel() <= buf.numel()
    return buf[~mark]


def _gaps_hold_the_canary(buf, view):
    assert view.numel() < buf.numel()
    return int((_gaps(buf, view).float() != X.CANARY).sum())


def _routes_to_cgemm(c):
    return c["api"] != "cabi" and X.host_plan(c)[0].route == "cgemm"


@pytest.mark.parametrize("name", list(CASES))
def test_einsum_launch_is_exact(name, monkeypatch, nan_outputs):
    from cplxmodule_amd import Cplx, cplx
    from cplxmodule_amd import einsum as E
    c = CASES[name]
    monkeypatch.delenv("CPLXAMD_EINSUM_GEMM", raising=False)
    if c["grad"] or _routes_to_cgemm(c):
        monkeypatch.setenv("CPLXAMD_EINSUM_GEMM", "0")       # the GEMM family has its own exact suite; this one is the kernel's
    d = X.make_inputs(c)
    v, in_bufs = _operands(c, d)
    views = dict(v)
    rec = Recorder(monkeypatch)
    problems, grads, leaves = [], None, None
    if c["api"] == "cabi":
        got, bufs = _run_cabi(c, v, rec)
    elif c["api"] == "contract":
        xa, xb, xo = X.explicit_eq(c)
        spec = (tuple(xa), tuple(xb), tuple(xo), tuple(X.extents(c).items()), c["conj"][0], c["conj"][1])
        got = E._contract(v["ar"], v["ai"], v["br"], v["bi"], spec)
    else:
        if c["grad"]:
            leaves, v = _leaves(c, v)
        out = cplx.einsum(c["eq"], Cplx(v["ar"], v["ai"]), Cplx(v["br"], v["bi"]))
        got = (out.real, out.imag)
        if c["grad"]:
            g = [torch.from_numpy(d["g" + p]).to(DEV).double() for p in "ri"]
            loss = (out.real.double() * g[0]).sum() + (out.imag.double() * g[1]).sum()
            grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    torch.cuda.synchronize()

    want_ran = [ENTRY] * (3 if c["grad"] else 1)
    if rec.ran() != want_ran:
        problems.append(f"ran {rec.ran()}, expected {want_ran} (failed: {rec.failed()})")
    else:
        on_device = rec.dispatch(0)
        if on_device != c["want"]:
            problems.append(f"the launch took (mode_a, mode_b, swapped, tile) = {on_device}, the table says {c['want']}")

    ref = X.reference(c)
    mask = torch.from_numpy(X.nan_mask(c)).to(DEV) if c["poison"] else None
    for p, t in zip("ri", got):
        assert t.dtype == X.TORCH_DTYPE[c["dtype"]] and tuple(t.shape) == X.out_shape(c), (p, t.dtype, t.shape)
        gt = t.detach().float()
        want = X.expected_of(ref[p], c["dtype"]).to(DEV)
        bad = ~(gt == want)
        if mask is not None:                                 # NaN in exactly the poisoned row and column, exact elsewhere
            bad = torch.where(mask, ~gt.isnan(), bad)
            want = torch.where(mask, torch.full_like(want, float("nan")), want)
        msg = X.describe_mismatch(bad, gt, want, c, p)
        if msg:
            problems.append(msg)
    if c["api"] == "cabi":
        for p, buf, view in zip("ri", bufs, got):
            n = _gaps_hold_the_canary(buf, view)
            if n:
                problems.append(f"C{p}: {n} values in the gaps of the padded C were overwritten")
    if c["grad"]:
        gref = X.grad_reference(name)
        for k, gt in grads.items():
            assert gt.dtype == X.TORCH_DTYPE[c["dtype"]] and tuple(gt.shape) == gref[k].shape, (k, gt.dtype, gt.shape)
            want = X.expected_of(gref[k], c["dtype"]).to(DEV)           # bf16: ONE rounding of the exact gradient
            msg = X.describe_mismatch(~(gt.float() == want), gt.float(), want, c, k, what="d")
            if msg:
                problems.append(msg)
        if "diagonal" in name:
            off = ~torch.eye(c["sa"][0], dtype=torch.bool, device=DEV)
            assert not bool(grads["ar"][off].any()) and not bool(grads["ai"][off].any())
    # the operands were not written: what lies between their elements is still NaN, their elements are unchanged
    for k, t in views.items():
        if not bool(_gaps(in_bufs[k], t).isnan().all()):
            problems.append(f"operand {k}: the NaN filler between its elements was overwritten")
        src = torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV).float()
        same = t.detach().float() == src
        if c["poison"] and k in ("ar", "bi"):
            same[c["poison"]["a" if k == "ar" else "b"]] = True
        if not bool(same.all()):
            problems.append(f"operand {k} was modified")
    assert not problems, f"{name}\n" + "\n".join(problems)
