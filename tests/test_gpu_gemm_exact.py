"""Every GEMM kernel behind csrc/gemm.hip, bit-exactly: integer-valued operands (gemm_exact_cases.py) make every route's
result independent of the order of accumulation, so each output tensor must EQUAL the float64 reference (float32 outputs)
or its one round-to-nearest-even (bf16 outputs) over the whole tensor -- and the entry point a case was written for must
be the one that ran and returned success, on the kernel the table names: a case that falls through to another kernel
fails.  The one tolerance is the expf of the emul_exp epilogue (gemm_exact_cases.exp_check).  The x3.py drivers run on
integer operands, whose low pieces are zero: their views, offsets, stacking and scale undo are checked, the low pieces'
cross products are not."""
import pytest
import torch

import gemm_exact_cases as G
from gemm_exact_cases import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"


class Recorder:
    """Recording wrappers around `call` / `try_call` of ops.py and x3.py: (entry point, returned success) per call."""

    def __init__(self, monkeypatch):
        from cplxmodule_amd import ops, x3, _lib
        self.log = []

        def call(name, *a):
            try:
                _lib.call(name, *a)
            except Exception:
                self.log.append((name, False))
                raise
            self.log.append((name, True))

        def try_call(name, *a):
            ok = _lib.try_call(name, *a)
            self.log.append((name, bool(ok)))
            return ok

        self.call = call
        for mod in (ops, x3):
            monkeypatch.setattr(mod, "call", call)
        monkeypatch.setattr(ops, "try_call", try_call)

    def ran(self):
        """The GEMM entry points that ran and returned success."""
        return sorted({n for n, ok in self.log if ok and n in G.COMPUTE})

    def declined(self):
        return sorted({n for n, ok in self.log if not ok})


def _view(vals, rs, cs, dtype, off=0, bs=None):
    """`vals` (logical [R, C], or [batch, R, C] with batch stride bs) as a strided view into a fresh NaN-filled buffer that
    starts `off` elements behind a 16-byte aligned address: what lies between the elements must never be read."""
    shape = tuple(vals.shape)
    strides = ((bs,) if vals.dim() == 3 else ()) + (rs, cs)
    n = 1 + sum((e - 1) * s for e, s in zip(shape, strides))
    buf = torch.full((off + n,), float("nan"), dtype=dtype, device=vals.device)
    v = buf[off:].as_strided(shape, strides)
    v.copy_(vals.to(dtype))
    return v


def _strides(c):
    if c["strides"]:
        return c["strides"][:2], c["strides"][2:]
    a = (1, c["lda"] or c["M"]) if c["ta"] else (c["lda"] or c["K"], 1)
    b = (1, c["ldb"] or c["N"]) if c["tb"] else (c["ldb"] or c["K"], 1)
    return a, b


def _out_planes(c, d, planes):
    """C planes [M, ldc]: the old C where the case accumulates, NaN elsewhere (an element the kernel does not write cannot
    hold the right value by accident), the canary in the padding columns."""
    ldc = c["ldc"] or c["N"]
    out = []
    for p in planes:
        t = torch.full((c["M"], ldc), G.CANARY if ldc > c["N"] else float("nan"), dtype=G.TORCH_DTYPE[c["out"]], device=DEV)
        t[:, :c["N"]] = d["c0" + p].to(t.dtype) if "acc" in c["epi"] else float("nan")
        out.append(t)
    return out


def _f32(t):
    return None if t is None else t.to(torch.float32).contiguous()


def _run(c, d, rec):
    """-> {plane: the [M, ldc] tensor the case's entry point wrote}."""
    from cplxmodule_amd import ops, x3, _lib
    from cplxmodule_amd._lib import ptr, stream_ptr
    M, N, K, cplx = c["M"], c["N"], c["K"], c["cplx"]
    planes = ("r", "i") if cplx else ("r",)
    dt = G.TORCH_DTYPE[c["dtype"]]
    if c["api"] == "x3":
        At, Bt = [_f32(d["a" + p]) for p in planes], [_f32(d["b" + p]) for p in planes]
        sp = lambda ts, *a, **k: x3.split_planes(tuple(ts), *a, kind=c["mode"], **k)  # noqa: E731
        bias = tuple(_f32(d["bias" + p]) for p in planes) if "bias" in c["epi"] else None
        if c["lay"] == "NN":
            got = x3.gemm_nn(sp(At), sp(Bt, x3.SPLIT_B), M, N, K, bias=bias if cplx or bias is None else bias[0], conj_b=c["conj_b"])
        elif c["lay"] == "NT":
            Bk = [b.t().contiguous() for b in Bt]
            got = x3.gemm_nt(sp(At), sp(Bk, x3.SPLIT_B, stacked=True), M, N, K, conj_b=c["conj_b"])
        else:
            Ak, Bk = [a.t().contiguous() for a in At], [b.t().contiguous() for b in Bt]
            out = _out_planes(c, d, planes)
            got = x3.gemm_tt(sp(Ak), sp(Bk), M, N, K, conj_b=c["conj_b"], out=tuple(out) if cplx else out[0], accumulate=True,
                             beta=torch.tensor(c["beta"], device=DEV), emul=_f32(d["emul"]))
        return dict(zip(planes, got if cplx else (got,)))
    if c["api"] == "batched":
        bs_a, bs_b = M * K + 24, N * K + 40                  # batch strides larger than the matrices
        a = [_view(d["a" + p], K, 1, dt, bs=bs_a) for p in planes]
        b = [_view(d["b" + p], K, 1, dt, bs=bs_b) for p in planes]
        cr, ci = ops.cgemm_batched(a[0], a[1], (K, 1, bs_a), b[0], b[1], (K, 1, bs_b), c["batch"], M, N, K, conj_b=c["conj_b"])
        return dict(r=cr, i=ci)
    if c["api"] == "lrt":
        g = [d["a" + p].to(dt).contiguous() for p in planes]               # G [B, O]
        w = [d["b" + p].t().to(dt).contiguous() for p in planes]           # W [O, I]: K-major for this product
        x = [d["x" + p].to(dt).contiguous() for p in planes]
        ga = d["ga"].to(dt).contiguous()
        if cplx:
            return dict(zip(planes, ops._cplx_lrt_dx(g[0], g[1], w[0], w[1], x[0], x[1], ga)))
        return dict(r=ops._real_lrt_dx(g[0], w[0], x[0], ga))
    sa, sb = _strides(c)
    ea, eb = c["scales"] or (0, 0)
    a = [_view(d["a" + p] * 2.0 ** ea, sa[0], sa[1], dt, off=c["a_off"]) for p in planes]
    b = [_view(d["b" + p] * 2.0 ** eb, sb[0], sb[1], dt) for p in planes]
    scales = None
    if c["scales"]:
        scales = tuple(torch.tensor([2.0 ** e, 2.0 ** -e], dtype=torch.float32, device=DEV) for e in (ea, eb))
    bias = [_f32(d["bias" + p]) for p in planes] if "bias" in c["epi"] else None
    emul = _f32(d["lmul"]) if "emul_exp" in c["epi"] else _f32(d.get("emul"))
    acc = "acc" in c["epi"]
    beta = torch.tensor(c["beta"], device=DEV) if acc and c["beta"] is not None else None
    out = _out_planes(c, d, planes)
    if c["api"] == "ops":
        if cplx:
            ops.cgemm(a[0], a[1], sa, b[0], b[1], sb, M, N, K, bias=tuple(bias) if bias else None, conj_b=c["conj_b"],
                      out=tuple(out), accumulate=acc, algo=int("3m" in c["epi"]), beta=beta, emul=emul, scales=scales)
        else:
            ops.rgemm(a[0], sa, b[0], sb, M, N, K, bias=bias[0] if bias else None, emul=emul, out=out[0],
                      emul_exp="emul_exp" in c["epi"], accumulate=acc, beta=beta, scales=scales)
        return dict(zip(planes, out))
    # the C ABI directly (as ops.cgemm / ops.rgemm call it), with the case's own ldc
    assert c["api"] == "cabi" and c["dtype"] == "bf16"
    ws = ops._gemm_ws(M, N, K, cplx, a[0], out[0])
    wsn = 0 if ws is None else ws.numel()
    codes = (G.DTYPE_CODE[c["dtype"]], G.DTYPE_CODE[c["out"]])
    if emul is not None:                                     # (the multiplier has C's leading dimension: include/cplxamd.h)
        dense, emul = emul, torch.full(out[0].shape, float("nan"), dtype=torch.float32, device=DEV)
        emul[:, :N] = dense
    with torch.cuda.device(out[0].device):
        if cplx:
            rec.call("cplxamd_cgemm_fl", ptr(a[0]), ptr(a[1]), sa[0], sa[1], ptr(b[0]), ptr(b[1]), sb[0], sb[1],
                     ptr(bias[0] if bias else None), ptr(bias[1] if bias else None), ptr(emul), ptr(out[0]), ptr(out[1]),
                     out[0].stride(0), M, N, K, int(c["conj_b"]), *codes, int(acc), ptr(beta), 0, ptr(ws), wsn,
                     _lib.launch_flags(), stream_ptr())
        else:
            rec.call("cplxamd_rgemm_fl", ptr(a[0]), sa[0], sa[1], ptr(b[0]), sb[0], sb[1], ptr(bias[0] if bias else None), ptr(emul),
                     int("emul_exp" in c["epi"]), ptr(out[0]), out[0].stride(0), M, N, K, *codes, int(acc), ptr(beta), ptr(ws), wsn,
                     _lib.launch_flags(), stream_ptr())
    return dict(zip(planes, out))


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_route_is_exact(name, monkeypatch):
    from cplxmodule_amd import _lib
    c = CASES[name]
    if G.plan_checked(c):
        # the table is written for 256 compute units: on another device its kinds would be another table's
        on_device = _lib.load().cplxamd_gemm_plan(*G.plan_args(c, ncu=0))
        assert on_device == c["kind"], (f"{name}: on this device the dispatcher picks kind {on_device} "
                                        f"({G.KIND_NAME.get(on_device)}), the table says {c['kind']} ({G.KIND_NAME[c['kind']]})")
    d = G.make_inputs(c, DEV)
    ref = G.reference(c, d)
    rec = Recorder(monkeypatch)
    with _lib.launch_policy(c["flags"]):
        got = _run(c, d, rec)
        torch.cuda.synchronize()
    problems = []
    want_ran = [G.ENTRY[c["entry"]]]
    if rec.ran() != want_ran:
        problems.append(f"ran {rec.ran()}, expected {want_ran} (declined: {rec.declined()})")
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    N = c["N"]
    for p, t in got.items():
        assert t.dtype == G.TORCH_DTYPE[c["out"]], (p, t.dtype)
        g = t[..., :N].float()
        if "emul_exp" in c["epi"]:
            bad = G.exp_check(g, ref[p], d["lmul"])
            want = ref[p] * torch.exp(d["lmul"])
        else:
            if "lrt" in c["epi"]:
                want = G.expected_lrt(ref[p], d["x" + p], d["ga"])
            else:
                want = G.expected(ref[p], c["out"])
            bad = ~(g == want)
            if c["out"] == "bf16" and c["K"] >= 128:
                changed, ties = G.rounding_content(ref[p])
                if changed < 0.15 or ties < 16:
                    problems.append(f"C{p}: the case does not exercise the rounding ({changed:.1%} changed, {ties} ties)")
        msg = G.describe_mismatch(bad, g, want, c, p, d)
        if msg:
            problems.append(msg)
        if t.shape[-1] > N:
            pad = t[..., N:].float() != G.CANARY
            if bool(pad.any()):
                problems.append(f"C{p}: {int(pad.sum())} padding values behind column {N} were overwritten, first at "
                                f"{tuple(pad.nonzero()[0].tolist())}")
    assert not problems, f"{name}\n" + "\n".join(problems)
