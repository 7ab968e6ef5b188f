"""Inputs that aim the KL penalty kernels (csrc/kl.hip) at their own seams: one table for tests/test_kl_sweep_host.py
(which runs the self-checks below on the CPU) and tests/test_gpu_kl_sweep.py.

With t = 2 ln(|w| + 1e-12) - log_sigma2 and x = e^t, the kernels change formula at
  x = 1/64    slope of the packed cplx_vd path: cubic below, 1 - exp(-x) above
  x = 1/4     slope of the generic path (one_minus_exp_neg): series below, 1 - expf(-x) above
  x = 1       value: power series at and below, gamma + ln x + E1(x) (A&S 5.1.56) above
  x = 104     E1 dropped at and above
  t = 20      softplus linear above
  |w|^2 = 1e-8  a float4 lane of cplx_vd holding one weight below redoes its four elements by the generic formulas
Uniform random data never lands within a few float32 ulps of these, so the switch family is FOUND: `emulate` restates
the two float32 evaluation chains (packed: x = |w|^2 exp(-ls2); generic: t = 2 logf(|w| + 1e-12) - ls2, x = expf(t))
with correctly rounded elementary functions, candidates are drawn around each switch-point at four operand magnitudes,
and those whose emulated x / t / |w|^2 is within 4 ulps are kept.  The hardware's exp2 / log2 are 1 ulp, so a point
found at -4 ... +4 emulated ulps is within a few ulps on the device as well, on either side.

Families (each a dict of float32 arrays wr, wi, ls2, g; g = upstream gradient with positive, negative and exactly
zero entries; lengths are multiples of 4 so that every element is seen by the float4 body):
  switch  the points above                          range  |w| in [1e-4, 30] log-uniform, ls2 in [-30, 12]
  mixed   0 ... 4 tiny weights per aligned quad      edge   overflowing x, subnormal x, sub-1e-26 weights, zeros, -0.0
The real kinds read wr alone; `family(name, real=True)` is the same table searched with |w| = |wr|.

Pure numpy from fixed seeds; no torch, no GPU."""
import functools
import itertools

import numpy as np

F32 = np.float32
T_KINDS = ("real_vd", "real_ard", "cplx_vd", "cplx_ard", "cplx_vd_approx", "cplx_vd_scalefree", "cplx_vd_bogus")
ALL_KINDS = T_KINDS + ("real_l0", "real_l1")
FAMILIES = ("switch", "range", "mixed", "edge")

Q_TINY = F32(1e-8)
# switch-point -> (quantity, "first side" predicate as the kernel writes it)
SWITCHES = {
    "x=1/64(packed)": ("x_packed", F32(0.015625), lambda v, s: v < s),
    "x=1(packed)": ("x_packed", F32(1.0), lambda v, s: v <= s),
    "x=104(packed)": ("x_packed", F32(104.0), lambda v, s: v < s),
    "x=1/4(generic)": ("x_gen", F32(0.25), lambda v, s: v < s),
    "x=1(generic)": ("x_gen", F32(1.0), lambda v, s: v <= s),
    "x=104(generic)": ("x_gen", F32(104.0), lambda v, s: v < s),
    "t=20": ("t_gen", F32(20.0), lambda v, s: v > s),
    "q=1e-8": ("q", Q_TINY, lambda v, s: v >= s),
}
T_STARS = (np.log(1 / 64), np.log(1 / 4), 0.0, np.log(104.0), 20.0)
MAGNITUDES = (3e-4, 1e-2, 1.0, 30.0)
TINY_ABS = (0.0, 1e-38, 1e-30, 1e-20, 3e-7, 9.9e-5)   # 1e-38: a subnormal float32 whose square is 0


def _r32(a):
    return np.asarray(a, np.float64).astype(F32)


def ulps(v, s):
    """signed distance of positive float32 v from positive float32 s in units in the last place"""
    return np.asarray(v, F32).view(np.int32).astype(np.int64) - int(np.asarray(s, F32).view(np.int32))


def emulate(wr, wi, ls2):
    """The kernels' float32 chains with correctly rounded exp / log / sqrt.  wi None: a real kind."""
    wr, ls2 = np.asarray(wr, F32), np.asarray(ls2, F32)
    if wi is None:
        q = wr * wr
        theta = np.abs(wr)
    else:
        wi = np.asarray(wi, F32)
        q = _r32((wr * wr).astype(np.float64) + wi.astype(np.float64) ** 2)      # fmaf(wi, wi, rn(wr * wr))
        theta = np.sqrt(q)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        # exp_neg: hi + lo of -ls2 * log2(e)
        l2e, ln2 = F32(1.44269504089), F32(0.69314718056)
        yh = -ls2 * l2e
        yl = _r32((-ls2).astype(np.float64) * float(l2e) - yh.astype(np.float64))
        e = _r32(np.exp2(yh.astype(np.float64)))
        en = _r32(e.astype(np.float64) * (yl * ln2).astype(np.float64) + e.astype(np.float64))
        x_packed = q * en
        lg = _r32(np.log((theta + F32(1e-12)).astype(np.float64)))
        t_gen = -(ls2 - F32(2.0) * lg)
        x_gen = _r32(np.exp(t_gen.astype(np.float64)))
    return dict(q=q, x_packed=x_packed, t_gen=t_gen, x_gen=x_gen)


def _upstream(rs, n):
    g = rs.uniform(0.25, 2.0, n) * np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)
    g[rs.uniform(size=n) < 0.125] = 0.0
    g[:3] = (1.0, -1.0, 0.0)
    return g.astype(F32)


def _polar(rs, mag, real):
    n = mag.shape[0]
    if real:
        return (mag * np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)).astype(F32), np.zeros(n, F32)
    ph = rs.uniform(0, 2 * np.pi, n)
    return (mag * np.cos(ph)).astype(F32), (mag * np.sin(ph)).astype(F32)


def _pad4(d, filler):
    n = d["wr"].shape[0]
    k = (-n) % 4
    if k:
        for key in d:
            d[key] = np.concatenate([d[key], np.full(k, filler[key], F32)])
    return d


def _range(rs, n, real):
    mag = np.exp(rs.uniform(np.log(1e-4), np.log(30.0), n))
    wr, wi = _polar(rs, mag, real)
    if not real:                       # purely real and purely imaginary weights
        m = n // 16
        sg = np.where(rs.uniform(size=2 * m) < 0.5, -1.0, 1.0)
        wr[:m], wi[:m] = (sg[:m] * mag[:m]).astype(F32), 0.0
        wr[m:2 * m], wi[m:2 * m] = 0.0, (sg[m:] * mag[m:2 * m]).astype(F32)
    return dict(wr=wr, wi=wi, ls2=rs.uniform(-30, 12, n).astype(F32), g=_upstream(rs, n))


def _switch(rs, real, keep=24, draws=6000):
    """By search: per switch-point and operand magnitude, up to `keep` points on EACH side within 4 emulated ulps."""
    out = {k: [] for k in ("wr", "wi", "ls2")}
    hits = {}

    def take(name, wr, wi, ls2):
        qty, s, first = SWITCHES[name]
        em = emulate(wr, None if real else wi, ls2)
        d = ulps(em[qty], s)
        near = (np.abs(d) <= 4) & np.isfinite(em[qty]) & (em[qty] > 0)
        side = first(em[qty], s)
        for sd in (True, False):
            idx = np.flatnonzero(near & (side == sd))[:keep]
            hits[(name, sd)] = hits.get((name, sd), 0) + idx.size
            for key, arr in (("wr", wr), ("wi", wi), ("ls2", ls2)):
                out[key].append(arr[idx])

    for tstar, mag0 in itertools.product(T_STARS, MAGNITUDES):
        mag = mag0 * rs.uniform(0.9, 1.1, draws)
        wr, wi = _polar(rs, mag, real)
        th = np.abs(wr.astype(np.float64)) if real else np.hypot(wr.astype(np.float64), wi.astype(np.float64))
        ls0 = 2 * np.log(th + 1e-12) - tstar
        # a float32 step of ls2 moves x by |ls2| ulps: the neighbouring values of ls2 for every weight
        cand = np.stack([_r32(ls0 + j * np.maximum(np.abs(ls0), 0.5) * 2.0 ** -24) for j in range(-6, 7)])
        names = [k for k, (qty, s, _) in SWITCHES.items()
                 if qty != "q" and abs(np.log(float(s)) - tstar if qty != "t_gen" else float(s) - tstar) < 1e-6]
        order = rs.permutation(cand.size)       # (every candidate: the generic x is a function of the float32 t alone,
        for name in names:                      #  the nearest candidate per weight would always be the switch-point itself)
            take(name, np.broadcast_to(wr, cand.shape).ravel()[order], np.broadcast_to(wi, cand.shape).ravel()[order],
                 cand.ravel()[order])
    if not real:
        # (whole quads up to here, `keep` is a multiple of 4: the weights at and just above 1e-8 stay on the packed path)
        k = (-sum(a.size for a in out["wr"])) % 4
        for key, v in (("wr", 0.01), ("wi", 0.0), ("ls2", -3.0)):
            out[key].append(np.full(k, v, F32))
        mag = 1e-4 * (1 + rs.uniform(-1e-6, 1e-6, draws))
        wr, wi = _polar(rs, mag, False)
        take("q=1e-8", wr, wi, rs.uniform(-12, 4, draws).astype(F32))
    d = {k: np.concatenate(v) for k, v in out.items()}
    # the q = 1e-8 points sit last; the filler keeps a quad of theirs from being padded with a foreign weight
    d["g"] = _upstream(rs, d["wr"].shape[0])
    return _pad4(d, dict(wr=0.01, wi=0.0, ls2=-3.0, g=1.0)), hits


def tiny_weight(rs, k, real=False):
    """k-th tiny weight (cycling through TINY_ABS) as (wr, wi)"""
    a = TINY_ABS[k % len(TINY_ABS)]
    if real or a == 1e-38 or k % 3 == 0:
        return (F32(a), F32(0.0)) if (k // 3) % 2 == 0 or real else (F32(0.0), F32(a))
    ph = rs.uniform(0, 2 * np.pi)
    return F32(a * np.cos(ph)), F32(a * np.sin(ph))


def _mixed(rs, real, quads=1020):
    """Aligned quads with 0 ... 4 tiny weights in every arrangement; the rest from the range family."""
    d = _range(rs, 4 * quads, real)
    d["wr"][:], d["wi"][:] = _polar(rs, np.exp(rs.uniform(np.log(2e-4), np.log(30.0), 4 * quads)), real)
    layouts = [c for k in range(5) for c in itertools.combinations(range(4), k)]     # 16 subsets of the 4 positions
    tiny = np.zeros(4 * quads, bool)
    count = [0, 0, 0, 0]                 # every position cycles through the tiny magnitudes on its own
    for qd in range(quads):
        for pos in layouts[qd % len(layouts)]:
            d["wr"][4 * qd + pos], d["wi"][4 * qd + pos] = tiny_weight(rs, count[pos], real)
            tiny[4 * qd + pos] = True
            count[pos] += 1
    d["tiny"] = tiny
    return d


def _edge(real):
    rows = []    # (name, wr, wi, ls2)
    for t in (60, 80, 88, 89, 100, 120):
        rows.append((f"t={t},|w|=1", 1.0, 0.0, -float(t)))
        rows.append((f"t={t},|w|=30", 30.0 if real else 18.0, 0.0 if real else 24.0, 2 * np.log(30.0) - t))
    for a in (1.5e-4, 1e-2, 1.0, 30.0):
        rows.append((f"ls2=80,|w|={a:g}", a, 0.0, 80.0))
        rows.append((f"ls2=80,|w|={a:g},imag", 0.0 if not real else -a, a if not real else 0.0, 80.0))
    rows.append(("-0.0 imaginary part", 0.05, -0.0, -5.0))
    rows.append(("zero imaginary part", -0.05, 0.0, -5.0))
    while len(rows) % 4:                # the rows so far are healthy: their quads stay on the packed path
        rows.append(("filler", 0.3, -0.4, -2.0))
    for a in (1e-27, 1e-30, 1e-36):
        for ls in (-8.0, 0.0, 3.0):
            rows.append((f"|w|={a:g},ls2={ls:g}", a, 0.0, ls))
            rows.append((f"|w|={a:g},ls2={ls:g},both planes", -a * 0.6, a * 0.8, ls))
    rows += [("zero", 0.0, 0.0, -5.0), ("zero real part", 0.0, 0.05, -5.0), ("-0.0 real part", -0.0, 0.05, -5.0),
             ("-0.0 both", -0.0, -0.0, -5.0), ("-0.0, +0.0", -0.0, 0.0, 2.0), ("zero, ls2=-20", 0.0, 0.0, -20.0)]
    while len(rows) % 4:
        rows.append(("filler", 0.3, -0.4, -2.0))
    wr = np.array([r[1] for r in rows], F32)
    wi = np.array([r[2] for r in rows], F32)
    if real:
        wi = np.zeros_like(wi)
    n = len(rows)
    g = np.resize(np.array([1.0, -1.5, 0.0, 0.5, -1.0, 2.0, 0.75], F32), n)
    return dict(wr=wr, wi=wi, ls2=np.array([r[3] for r in rows], F32), g=g), [r[0] for r in rows]


@functools.lru_cache(maxsize=None)
def _build(name, real):
    rs = np.random.RandomState(dict(switch=101, range=102, mixed=103, edge=104)[name] + 1000 * real)
    if name == "switch":
        return _switch(rs, real)
    if name == "range":
        return _range(rs, 16384, real), None
    if name == "mixed":
        return _mixed(rs, real), None
    if name == "edge":
        return _edge(real)
    raise KeyError(name)


def family(name, real=False):
    """dict(wr, wi, ls2, g) of float32 arrays (read-only: shared between tests); wi is all zero for real=True."""
    d = _build(name, bool(real))[0]
    for v in d.values():
        v.setflags(write=False)
    return d


def switch_hits(real=False):
    """{(switch-point, first side?): number of points within 4 emulated ulps}"""
    return dict(_build("switch", bool(real))[1])


def edge_names(real=False):
    return list(_build("edge", bool(real))[1])


def is_real(kind):
    return kind.startswith("real")


# ---- float64 reference and the per-element bounds ------------------------------------------------------------------------
EPS32 = float(np.finfo(F32).eps)
L0_SHIFT = 0.66 * np.log(11.0)          # -beta log(-gamma / zeta), beta = 0.66, gamma = -0.1, zeta = 1.1


def reference(kind, d, g=None):
    """float64 value, slope f'(t) and gradients of sum(g * penalty) on the float32 inputs."""
    from oracle import cplx_oracle as orc
    f = np.float64
    wr, ls2 = d["wr"].astype(f), d["ls2"].astype(f)
    g = (d["g"] if g is None else np.broadcast_to(np.asarray(g), wr.shape)).astype(f)
    zero = np.zeros_like(wr)
    if kind == "real_l0":               # sigmoid(shift - log_alpha), the parameter is passed as log_sigma2
        s = orc.sigmoid(L0_SHIFT - ls2)
        return dict(value=s, slope=-s * (1 - s), dlog_sigma2=-s * (1 - s) * g, dwr=zero, cond=np.abs(ls2))
    if kind == "real_l1":
        return dict(value=np.abs(wr), slope=np.sign(wr), dlog_sigma2=zero, dwr=np.sign(wr) * g, cond=zero)
    wi = None if is_real(kind) else d["wi"].astype(f)
    t = -orc.log_alpha(ls2, wr, wi)
    out = dict(value=orc.penalty_exact(kind, ls2, wr, wi), slope=orc.penalty_dt(kind, t))
    if kind == "cplx_vd_bogus":         # its value is t itself (f' = 1); penalty_dt is the slope its GRADIENT uses
        out["slope"] = np.ones_like(t)
    out.update(orc.penalty_bwd(kind, g, ls2, wr, wi))
    q = wr * wr if wi is None else wr * wr + wi * wi
    out["cond"] = np.abs(ls2) + np.abs(np.log(q + 1e-24))
    out["theta"] = np.sqrt(q)
    return out


def bounds(ref, g):
    """The project's tolerances (tests/test_gpu_vd.py: 2e-6 on values, 2e-5 and 8 eps32 on gradients, the weight
    gradient's amplification 2 / (|w| + 1e-12)) plus the conditioning of the value: an error of a few eps32 in ls2 or
    ln |w|^2 moves f by f'(t) times that."""
    g = np.abs(np.asarray(g, np.float64))
    amp = np.maximum(2 / (ref.get("theta", np.ones_like(ref["value"])) + 1e-12), 1.0)
    b = dict(value=2e-6 * np.abs(ref["value"]) + 8 * EPS32 * np.abs(ref["slope"]) * ref["cond"] + 1e-37,
             dlog_sigma2=2e-5 * np.abs(ref["dlog_sigma2"]) + 8 * EPS32 * g,
             dwr=2e-5 * np.abs(ref["dwr"]) + 8 * EPS32 * g * amp)
    if "dwi" in ref:
        b["dwi"] = 2e-5 * np.abs(ref["dwi"]) + 8 * EPS32 * g * amp
    return b


def excluded(kind, name):
    """elements whose float64 reference is not finite (the only ones a test may skip)"""
    ref = reference(kind, family(name, is_real(kind)))
    bad = np.zeros(ref["value"].shape, bool)
    for k in ("value", "dlog_sigma2", "dwr", "dwi"):
        if k in ref:
            bad |= ~np.isfinite(ref[k])
    return bad


@functools.lru_cache(maxsize=None)
def bf16_midpoint_ls2():
    """float32 ls2 whose exp (correctly rounded to float32) lies within 2 float32 ulps of a bfloat16 rounding midpoint
    in [0.4, 2.7]: where a 1-ulp expf decides which way bf16(exp(ls2)) rounds.  By search over the neighbours of ln m."""
    hi = np.arange(int(F32(0.4).view(np.int32)) >> 16, (int(F32(2.7).view(np.int32)) >> 16) + 1, dtype=np.int64)
    mid = ((hi << 16) | 0x8000).astype(np.int32).view(F32)
    l0 = _r32(np.log(mid.astype(np.float64)))
    up, dn = [l0], [l0]
    for _ in range(3):
        up.append(np.nextafter(up[-1], F32(np.inf)).astype(F32))
        dn.append(np.nextafter(dn[-1], F32(-np.inf)).astype(F32))
    ls = np.concatenate(up + dn[1:])
    m = np.tile(mid, 7)
    e = _r32(np.exp(ls.astype(np.float64)))
    keep = np.abs(e.view(np.int32).astype(np.int64) - m.view(np.int32).astype(np.int64)) <= 2
    out = np.unique(ls[keep])
    out.setflags(write=False)
    return out


def self_check():
    """Both sides of every switch-point hit at least 8 times; every arrangement of tiny weights present; no element
    of any family has a non-finite reference (so none is ever skipped)."""
    for real in (False, True):
        hits = switch_hits(real)
        for name, (qty, _, _) in SWITCHES.items():
            if real and (qty in ("q", "x_packed")):
                continue
            for side in (True, False):
                assert hits.get((name, side), 0) >= 8, (real, name, side, hits.get((name, side), 0))
    m = family("mixed")
    tiny = m["tiny"].reshape(-1, 4)
    q = (m["wr"].astype(np.float64) ** 2 + m["wi"].astype(np.float64) ** 2).reshape(-1, 4)
    assert ((q < 1e-8) == tiny).all()
    seen = {tuple(r) for r in tiny}
    assert len(seen) == 16, len(seen)                      # every subset of the four positions
    mags = np.round(np.log10(np.sqrt(q) + 1e-45)).astype(int)
    for pos in range(4):                                   # every tiny magnitude at every position
        assert len(set(mags[tiny[:, pos], pos])) == len(TINY_ABS), (pos, set(mags[tiny[:, pos], pos]))
    for kind in T_KINDS:
        for name in FAMILIES:
            assert not excluded(kind, name).any(), (kind, name)
    return True
