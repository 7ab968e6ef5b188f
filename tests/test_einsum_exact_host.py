"""Host-side checks of the bit-exact einsum cases (einsum_exact_cases.py): every case gets the dispatch it was written for
(cplxamd_einsum_plan: the real host code of cplxamd_ceinsum, dry), the table covers every load path, tile, swap state and
conjugation, the int64 reference is what the descriptor handed to the kernel describes (the descriptor walker of
test_einsum_host.py), every view stays inside its own allocation, and the bf16 cases that are deep enough exercise the
rounding."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import einsum_exact_cases as X
from einsum_exact_cases import CASES
from test_einsum_host import offsets, run_plan

ALL = list(CASES)


def _code(dtype):
    from cplxmodule_amd import _lib
    return {"f32": _lib.F32, "bf16": _lib.BF16}[dtype]


def _dispatch(c):
    from cplxmodule_amd import ops
    p, a0, b0 = X.host_plan(c)
    r = ops.einsum_dispatch(ops.einsum_desc(p), X.declared_addresses(c, a0, b0), _code(c["dtype"]))
    return (r["mode_a"], r["mode_b"], r["swapped"], r["tile"]), r["grid"]


# ---- the table itself ------------------------------------------------------------------------------------------------------------
def test_case_names_are_unique():
    with pytest.raises(AssertionError):
        X.case(ALL[0], "ij,jk->ik", (2, 3), (3, 4), "f32", want=("KFAST", "KFAST", False, 64))
    assert all(c["name"] == n for n, c in CASES.items())
    assert all(("_f32" in n) == (c["dtype"] == "f32") and ("_bf16" in n) == (c["dtype"] == "bf16") for n, c in CASES.items())


@pytest.mark.parametrize("name", ALL)
def test_case_is_well_formed(name):
    """Integers within their limits that survive the cast to the case's dtype; 128 K < 2^24; at most ~10^8 multiply-adds."""
    c = CASES[name]
    assert X.well_formed(c)
    d = X.make_inputs(c)
    assert sorted(d) == sorted(["ar", "ai", "br", "bi"] + (["gr", "gi"] if c["grad"] else []))
    for k, v in d.items():
        assert v.dtype == np.int64 and np.abs(v).max() <= (3 if k[0] == "g" else 8), k
        t = torch.from_numpy(v)
        assert torch.equal(t.to(X.TORCH_DTYPE[c["dtype"]]).to(torch.int64), t), k
    assert d["ar"].shape == c["sa"] and d["bi"].shape == c["sb"]
    for op, lay in (("a", c["la"]), ("b", c["lb"])):
        for ax in lay["expand"]:
            assert (d[op + "r"] == d[op + "r"].take([0], axis=ax)).all()
    ref = X.reference(c)
    assert ref["r"].shape == ref["i"].shape == X.out_shape(c) and ref["r"].dtype == np.int64
    assert max(np.abs(ref["r"]).max(), np.abs(ref["i"]).max()) <= 128 * X.totals(c)[3]
    if c["name"] in X.F32_ONLY:
        assert c["dtype"] == "f32" and c["grad"] and (c["la"]["expand"] or c["lb"]["expand"])
    elif c["grad"]:
        assert not c["la"]["expand"] and not c["lb"]["expand"]           # (summed by autograd after the store: not ONE rounding)
    if c["poison"]:
        assert c["poison"]["a"][-1] == c["sa"][-1] - 1 and c["poison"]["a"][1] == c["sa"][1] - 1 and c["sa"][1] % c["want"][3]


def test_inputs_are_seeded_by_the_case_name():
    a, b = CASES["load_f32_t64_KVEC_KVEC"], CASES["load_f32_t64_KVEC_KFAST"]
    assert np.array_equal(X.make_inputs(a)["ar"], X.make_inputs(a)["ar"])
    assert a["sa"] == b["sa"] and not np.array_equal(X.make_inputs(a)["ar"], X.make_inputs(b)["ar"])


@pytest.mark.parametrize("name", ALL)
def test_case_gets_the_dispatch_it_names(name):
    """cplxamd_einsum_plan on the case's descriptor and declared alignment: the M / N swap, both load paths and the tile."""
    c = CASES[name]
    got, grid = _dispatch(c)
    assert got == c["want"], (got, c["want"])
    B, M, N, K = X.totals(c)
    t = c["want"][3]
    assert grid == B * -(-M // t) * -(-N // t)


def test_plan_returns_the_error_codes_of_the_launcher():
    from cplxmodule_amd import _lib, ops
    from cplxmodule_amd import einsum as E
    lib = _lib.load()
    ok = ctypes.c_void_p(256)
    out = (ctypes.c_int64 * 5)(*([-7] * 5))
    d = ops.einsum_desc(E.plan("bmk,bkn->bmn", [(2, 3, 4), (2, 4, 5)]))
    plan = lambda d, dt=_lib.F32: lib.cplxamd_einsum_plan(ctypes.byref(d), 256, 256, 256, 256, dt, out)  # noqa: E731
    run = lambda d, dt=_lib.F32: lib.cplxamd_ceinsum(ok, ok, ok, ok, ok, ok, ctypes.byref(d), 0, 0, dt, dt, None)  # noqa: E731
    assert lib.cplxamd_einsum_plan(None, 0, 0, 0, 0, _lib.F32, out) == -1
    assert lib.cplxamd_einsum_plan(ctypes.byref(d), 0, 0, 0, 0, _lib.F32, None) == -1
    for dt in (_lib.F16, _lib.F64):
        assert plan(d, dt) == run(d, dt) == -3
    for grp, field, idx, val in ((1, "nmodes", None, 9), (1, "nmodes", None, -1), (1, "stride_c", 0, 0), (3, "extent", 0, -4)):
        arr = getattr(d, field)
        old = arr[grp] if idx is None else arr[grp][idx]
        if idx is None:
            arr[grp] = val
        else:
            arr[grp][idx] = val
        assert plan(d) == run(d) == -1, (grp, field)
        if idx is None:
            arr[grp] = old
        else:
            arr[grp][idx] = old
    assert list(out) == [-7] * 5                                    # nothing is written on an error
    d.extent[2][0] = 0                                              # an empty result: success, a grid of 0
    assert plan(d) == run(d) == 0 and out[4] == 0
    d.extent[2][0] = 5
    assert plan(d) == 0 and list(out) == [1, 2, 0, 64, 2]           # A k-contiguous (KVEC), B [b, k, n] (ROWS), two 64-tiles
    assert lib.cplxamd_einsum_plan(ctypes.byref(d), 260, 256, 256, 256, _lib.F32, out) == 0 and out[0] == 0      # A misaligned
    assert lib.cplxamd_einsum_plan(ctypes.byref(d), 256 + 16, 256, 256, 256 + 32, _lib.F32, out) == 0 and out[0] == 1
    d.nmodes[0] = 2
    d.extent[0][0], d.extent[0][1] = 2 ** 16, 2 ** 16
    d.stride_c[0][0] = d.stride_c[0][1] = 1
    assert plan(d) == run(d) == -3                                  # a group beyond 31 bits
    d.extent[0][0], d.extent[0][1] = 2 ** 15, 2 ** 15               # 2^30 batch entries x 2 tiles... of M = 3: a grid of 2^30
    assert plan(d) == 0 and out[4] == 2 ** 30
    d.extent[1][0] = 200                                            # two tiles of 128 per entry: the grid beyond 31 bits
    assert plan(d) == -3


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_dispatch_has_a_case():
    have = {(c["dtype"],) + c["want"] for c in CASES.values()}
    for dt in X.DTYPES:
        for tile, ma, mb, sw in itertools.product((64, 128), X.MODES[dt], X.MODES[dt], (False, True)):
            assert (dt, ma, mb, sw, tile) in have, (dt, ma, mb, sw, tile)
        # every conjugation pair in both swap states, on both tiles
        conj = {(c["conj"], c["want"][2], c["want"][3]) for c in CASES.values() if c["dtype"] == dt and c["api"] != "einsum"}
        for ca, cb, sw, tile in itertools.product((False, True), (False, True), (False, True), (64, 128)):
            assert ((ca, cb), sw, tile) in conj, (dt, ca, cb, sw, tile)
        mine = [c for c in CASES.values() if c["dtype"] == dt]
        # the K sets of the stage seams, on the scalar and on the vector paths
        for md in X.MODES[dt]:
            ks = {X.totals(c)[3] for c in mine if c["kseam"] and c["want"][:2] == (md, md) and c["want"][3] == 64}
            assert ks == set(X.KSEAM_VEC[dt] if md == "KVEC" else X.KSEAM[dt]), (dt, md, ks)
        assert {X.totals(c)[3] // X.BK[dt] + 1 for c in mine if c["kseam"] and c["want"][3] == 128} >= {2, 4}
        # the M / N seams
        mn = {(c["want"][3],) + X.totals(c)[1:3] for c in mine if c["family"] == "mnseam"}
        assert mn == {(64, m, n) for m in X.MN64 for n in X.MN64} | {(128, m, n) for m in X.MN128 for n in X.MN128}
        # the C ABI: a padded C, negated strides in A and in B (rows and K), empty groups, odd bases
        cabi = [c for c in mine if c["api"] == "cabi"]
        assert any(any(c["cabi"]["c"]["pad"] or ()) for c in cabi) and any(c["cabi"]["c"]["step"] for c in cabi)
        assert {c["cabi"].get("rev_a") for c in cabi} >= {"m", "k"} and {c["cabi"].get("rev_b") for c in cabi} >= {"n", "k"}
        empty = set()
        for c in cabi:
            p = X.cabi_plan(c)[0]
            empty |= {g for g, modes in zip("bmnk", p.groups) if not modes}
            assert X.geometry(X.out_shape(c), c["cabi"]["c"])[2] > int(np.prod(X.out_shape(c))), c["name"]     # every C is padded
        assert empty == set("bmnk")
        assert any(c["la"]["off"] % 2 and c["lb"]["off"] % 2 and c["cabi"]["c"]["off"] % 2 for c in cabi)
        # a group of exactly 8 modes, for M, N and K, and groups of several modes in every position
        eight = {g for c in mine for g, modes in zip("bmnk", X.host_plan(c)[0].groups) if len(modes) == 8}
        assert eight == set("mnk"), eight
        assert any(len(X.host_plan(c)[0].batch) == 2 and 0 in [md.sb for md in X.host_plan(c)[0].batch] for c in mine)
        # gradients, one per feature; containment on the vector paths and both tiles
        assert sum(c["grad"] for c in mine) == (8 if dt == "f32" else 7)
        nan = {c["want"] for c in mine if c["poison"]}
        assert nan == {(md, md, False, t) for md in (("KVEC", "ROWVEC") if dt == "bf16" else ("KVEC",)) for t in (64, 128)}
        # the planner's features and the three output orders
        eqs = {c["eq"] for c in mine}
        assert eqs >= {"ijk,jl->il", "iij,jk->ik", "...ik,...kj->...ij", "ij,ij->ij", "i,j->ij", "i,i->", "ij,j->i", "bmk,bkn->mnb"}
        assert any(c["eq"] == "i,i->" and c["sa"] == (1000,) for c in mine)
    assert {c["api"] for c in CASES.values()} == {"einsum", "contract", "cabi"}


def test_both_swap_states_occur_with_each_load_mode_in_each_role():
    for dt in X.DTYPES:
        for md in X.MODES[dt]:
            for tile in (64, 128):
                for sw in (False, True):
                    assert any(c["dtype"] == dt and c["want"][0] == md and c["want"][2:] == (sw, tile) for c in CASES.values())
                    assert any(c["dtype"] == dt and c["want"][1] == md and c["want"][2:] == (sw, tile) for c in CASES.values())


# ---- the reference is what the descriptor describes ------------------------------------------------------------------------------
def _flat(c, d, op):
    """The complex buffer of operand `op` as the kernel's base pointer sees it (NaN between the elements)."""
    shape, lay = (c["sa"], c["la"]) if op == "a" else (c["sb"], c["lb"])
    bufs = [X.build_view(torch.from_numpy(d[op + p]).double(), lay, torch.float64)[0].numpy() for p in "ri"]
    return bufs[0] + 1j * bufs[1]


@pytest.mark.parametrize("name", ALL)
def test_reference_equals_the_walk_of_the_descriptor(name):
    """run_plan (test_einsum_host.py) on the plan handed to the kernel, over the NaN-filled buffers, equals the int64
    reference of the logical operands; every offset the kernel forms -- 16-byte loads included -- lies inside the operand's
    own buffer, and C's offsets are exactly the elements of the output view."""
    from cplxmodule_amd import einsum as E
    c = CASES[name]
    d = X.make_inputs(c)
    p, a0, b0 = X.host_plan(c)
    for g in p.groups:
        assert len(g) <= E.MAX_MODES
    a_flat, b_flat = _flat(c, d, "a"), _flat(c, d, "b")
    # bounds: the smallest and the largest element offset of each operand
    for flat, base, attr in ((a_flat, a0, "sa"), (b_flat, b0, "sb")):
        groups = [g for g, k in zip(p.groups, "bmnk") if not (attr == "sa" and k == "n") and not (attr == "sb" and k == "m")]
        lo = base + sum(min(0, (md.extent - 1) * getattr(md, attr)) for g in groups for md in g)
        hi = base + sum(max(0, (md.extent - 1) * getattr(md, attr)) for g in groups for md in g)
        assert 0 <= lo and hi < flat.size, (attr, lo, hi, flat.size)
    shape = X.out_shape(c)
    if c["api"] == "cabi":
        stc, c0, cn = X.cabi_plan(c)[3]
        idx = c0 + (offsets(p.batch, "sc")[:, None, None] + offsets(p.m, "sc")[None, :, None] + offsets(p.n, "sc")[None, None, :])
        view = torch.arange(cn).as_strided(shape, stc, c0)
        assert sorted(idx.ravel().tolist()) == sorted(view.reshape(-1).tolist()) and 0 <= idx.min() and idx.max() < cn
        dense = dict(zip(X.explicit_eq(c)[2], E.contiguous_strides(shape)))
        redo = lambda g: tuple(E.Mode(md.extent, md.sa, md.sb, dense.get(md.labels, 0), md.labels) for md in g)  # noqa: E731
        p = E.Plan(redo(p.batch), redo(p.m), redo(p.n), p.k, shape, p.conj_a, p.conj_b, p.route)
    assert p.out_shape == shape and (p.conj_a, p.conj_b) == c["conj"]
    got = run_plan(p, a_flat, b_flat, a0, b0)
    ref = X.reference(c)
    assert not np.isnan(got).any()
    assert np.array_equal(got.real, ref["r"]) and np.array_equal(got.imag, ref["i"])


def test_vector_loads_stay_inside_the_rows_they_start_in():
    """What makes a 16-byte load safe: a KVEC operand's innermost K extent is a multiple of the vector and a ROWVEC operand's
    innermost row extent a multiple of 8, so no load of `vec` elements starts inside the view and ends outside it."""
    for c in CASES.values():
        p = X.host_plan(c)[0]
        ma, mb, sw, _ = c["want"]
        for md, rows, attr in ((mb if sw else ma, p.m, "sa"), (ma if sw else mb, p.n, "sb")):
            if md == "KVEC":
                assert getattr(p.k[-1], attr) == 1 and p.k[-1].extent % X.VEC[c["dtype"]] == 0, c["name"]
            if md == "ROWVEC":
                assert getattr(rows[-1], attr) == 1 and rows[-1].extent % 8 == 0, c["name"]


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["grad"]])
def test_gradient_reference_equals_float64_autograd(name):
    """The int64 gradient formulas against torch's float64 autograd of the four-product formula (exact on integers)."""
    c = CASES[name]
    d = X.make_inputs(c)
    ts = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("ar", "ai", "br", "bi")}
    re = torch.einsum(c["eq"], ts["ar"], ts["br"]) - torch.einsum(c["eq"], ts["ai"], ts["bi"])
    im = torch.einsum(c["eq"], ts["ar"], ts["bi"]) + torch.einsum(c["eq"], ts["ai"], ts["br"])
    loss = (re * torch.from_numpy(d["gr"]).double()).sum() + (im * torch.from_numpy(d["gi"]).double()).sum()
    grads = dict(zip(ts, torch.autograd.grad(loss, list(ts.values()))))
    want = X.grad_reference(name)
    for k, g in grads.items():
        for op, lay in (("a", c["la"]), ("b", c["lb"])):
            if k[0] == op:
                for ax in lay["expand"]:
                    g = g.sum(ax, keepdim=True)
        assert np.array_equal(g.numpy(), want[k].astype(np.float64)), k
    if "diagonal" in name:                  # exactly zero off the diagonal
        off = ~np.eye(c["sa"][0], dtype=bool)
        assert not want["ar"][off].any() and not want["ai"][off].any() and want["ar"].any()


def test_nan_mask_is_one_row_and_one_column():
    c = CASES["nan_bf16_t64_ROWVEC"]
    m = X.nan_mask(c)
    (ba, ra, _), (bb, rb, _) = c["poison"]["a"], c["poison"]["b"]
    want = np.zeros_like(m)
    want[ba, ra, :] = True
    want[bb, :, rb] = True
    assert np.array_equal(m, want) and m.sum() == c["sb"][1] + c["sa"][1]


# ---- expected values ----------------------------------------------------------------------------------------------------------------
def test_expected_refuses_what_float32_cannot_hold_and_rounds_once():
    assert torch.equal(X.expected_of(np.array([1, -5, 2 ** 24, 3 * 2 ** 30]), "f32").double(),
                       torch.tensor([1.0, -5.0, 2.0 ** 24, 3.0 * 2.0 ** 30], dtype=torch.float64))
    for dt in X.DTYPES:
        with pytest.raises(ValueError):
            X.expected_of(np.array([1, 2 ** 24 + 1]), dt)
    # bf16 keeps 8 significant bits: between 256 and 512 it holds the even integers, 257 and 259 are ties
    v = np.array([255, 257, 259, 258, -257, -259, 513, 515, 514, 518])
    assert X.expected_of(v, "bf16").tolist() == [255.0, 256.0, 260.0, 258.0, -256.0, -260.0, 512.0, 516.0, 512.0, 520.0]
    assert X.expected_of(v, "bf16").dtype == torch.float32


# ---- do the bf16 results exercise the rounding? ----------------------------------------------------------------------------------
# bf16 holds the integers below 256; with operands in [-8, 8] a complex sum of K = 128 products has a standard deviation
# of 384, and three tenths of such sums change under one rounding, many of them exact ties (test_gemm_exact_host.py).  The
# cases below K = 128 test addressing, not the rounding, and are listed here by family (their number per family is pinned);
# every load path, tile and swap state has a deep case ('deep_*').  The gradient cases are shallow in their FORWARD only: their
# backward contractions are deep, which test_bf16_gradient_case_exercises_the_rounding asserts plane by plane.  The scalar dot has two output values in all: it cannot hold 16 ties, so its seed is chosen
# such that BOTH of its values are exact ties that round AWAY from zero (neither truncation nor round-half-down gives them), and
# that is what is asserted of it.
_SHALLOW_FAMILIES = ("load", "kseam", "mnseam", "conj", "cabi", "nan", "order", "grad")
TOO_SHALLOW = (
    {n for n in CASES if "_bf16" in n and n.split("_")[0] in _SHALLOW_FAMILIES}
    | {f"modes_bf16_{w}" for w in ("mn_k3x7", "mn_k5x9", "mn_k5x9_t128", "two_batch_stride0", "eight_m", "eight_n")}
    | {f"feat_bf16_{w}" for w in ("summed_only_label", "diagonal", "ellipsis_broadcast", "hadamard", "outer", "matvec")}
)
SCALAR = {"feat_bf16_dot_k1000"}
_BF16 = [n for n, c in CASES.items() if c["dtype"] == "bf16"]


SHALLOW_COUNT = {"cabi": 10, "conj": 16, "feat": 6, "grad": 7, "kseam": 31, "load": 72, "mnseam": 25, "modes": 6, "nan": 4, "order": 2}


def test_shallow_cases_are_the_listed_ones():
    assert {n for n in _BF16 if X.totals(CASES[n])[3] < 128} == TOO_SHALLOW
    # pinned: a new shallow case does not join the set silently
    count = {}
    for n in TOO_SHALLOW:
        count[n.split("_")[0]] = count.get(n.split("_")[0], 0) + 1
    assert count == SHALLOW_COUNT and len(TOO_SHALLOW) == 179
    deep = [CASES[n] for n in _BF16 if n not in TOO_SHALLOW and n not in SCALAR]
    assert len(deep) == 17
    for md in X.MODES["bf16"]:
        for tile in (64, 128):
            for sw in (False, True):
                assert any(c["want"] == (md, md, sw, tile) for c in deep), (md, tile, sw)


@pytest.mark.parametrize("name", [n for n in _BF16 if n not in TOO_SHALLOW])
def test_bf16_case_exercises_the_rounding(name):
    """At least 15 % of the expected values change under the rounding and at least 16 are exact ties: a condition on the
    INPUTS, so that no case silently tests nothing."""
    c = CASES[name]
    for p, v in X.reference(c).items():
        changed, ties = X.rounding_content(torch.from_numpy(np.atleast_1d(v).astype(np.float64)))
        if name in SCALAR:
            away = abs(float(X.expected_of(np.atleast_1d(v), "bf16")[0])) > abs(int(v))
            assert v.size == 1 and changed == 1.0 and ties == 1 and away, (p, int(v), changed, ties)
        else:
            assert changed >= 0.15 and ties >= 16, (p, changed, ties)


_BF16_GRAD = [n for n in _BF16 if CASES[n]["grad"]]


def test_every_bf16_gradient_feature_has_a_deep_case():
    assert sorted(n[len("grad_bf16_"):] for n in _BF16_GRAD) == ["bmm", "diagonal", "ellipsis_broadcast", "heads", "out_perm",
                                                                 "summed_only_label", "two_k_modes"]
    assert {CASES[n]["want"][2] for n in _BF16_GRAD} == {False, True}          # both swap states of the forward


@pytest.mark.parametrize("name", _BF16_GRAD)
def test_bf16_gradient_case_exercises_the_rounding(name):
    """The forward of a gradient case is shallow (TOO_SHALLOW), its BACKWARD contractions are not: they reduce over N (dA,
    and over what A is broadcast along) and over M (dB), ~600 terms here.  At least 15 % of every gradient plane changes
    under the ONE rounding it is held to and at least 16 values are exact ties, so a truncating or twice-rounding backward
    launch cannot pass.  (The gradient of a diagonal operand is zero off the diagonal: its diagonal is what is measured.)"""
    c = CASES[name]
    sub_a = X.explicit_eq(c)[0]
    for k, v in X.grad_reference(name).items():
        if k[0] == "a" and len(set(sub_a)) < len(sub_a):
            v = np.einsum(f"{sub_a}->{''.join(dict.fromkeys(sub_a))}", v)
        changed, ties = X.rounding_content(torch.from_numpy(np.ascontiguousarray(v).astype(np.float64)))
        assert changed >= 0.15 and ties >= 16, (k, changed, ties)


# ---- the seams the reports name ------------------------------------------------------------------------------------------------------
def test_describe_mismatch_names_the_seam():
    c = CASES["deep_bf16_t64_KVEC"]                        # [2, 72, 40] on 64-tiles, K = 136: stages of 32, the last k >= 128
    ref = X.reference(c)
    want = X.expected_of(ref["i"], "bf16")
    assert X.describe_mismatch(~(want == want), want, want, c, "i") == ""
    assert X.describe_mismatch(~(-0.0 * want == 0.0 * want), want, want, c, "i") == ""          # by value
    # a bumped border element, a NaN in the last row of the ragged tile
    got = want.clone()
    got[1, 63, 7] += 4
    got[0, 71, 39] = float("nan")
    got[1, 64, 5] -= 4
    msg = X.describe_mismatch(~(got == want), got, want, c, "i")
    assert msg.startswith("Ci: 3 of 5760 values differ") and "(1, 63, 7)" in msg and "tile border" in msg
    assert "last row and column of a ragged tile" in msg and "got nan" in msg and "batch 1, 64 x 64 tile 1,0" in msg
    assert "lacks" not in msg and "TRUNCATED" not in msg and "flipped" not in msg
    # a lost last K stage
    d = X.make_inputs(c)
    short = {k: v.copy() for k, v in d.items()}
    short["ar"][..., 128:] = 0
    short["ai"][..., 128:] = 0
    got = X.expected_of(X.products(c["eq"], short)["i"], "bf16")
    msg = X.describe_mismatch(~(got == want), got, want, c, "i")
    assert "the result lacks exactly the last K stage (k >= 128)" in msg and "TRUNCATED" not in msg
    # truncation instead of round-to-nearest-even
    got = X._truncated(X.expected_of(ref["i"], "f32"))
    bad = ~(got == want)
    assert 0.1 < float(bad.float().mean()) < 0.5
    msg = X.describe_mismatch(bad, got, want, c, "i")
    assert "TRUNCATED to bf16" in msg and "lacks" not in msg and "flipped" not in msg
    # a flipped conjugation
    for which, conj in (("A", (True, False)), ("B", (False, True))):
        for plane in "ri":
            want = X.expected_of(ref[plane], "bf16")
            got = X.expected_of(X.reference(c, conj=conj)[plane], "bf16")
            msg = X.describe_mismatch(~(got == want), got, want, c, plane)
            assert f"conjugation flag of {which} flipped" in msg, (which, plane)
    # a swapped case names the swap; a multi-mode case its flat tile; a gradient plane just the values
    c = CASES["modes_f32_mn_k3x7"]                          # M = 5 x 13, N = 3 x 23: (4, 12, 2, 22) is row 64, column 68
    want = X.expected_of(X.reference(c)["r"], "f32")
    got = want.clone()
    got[4, 12, 2, 22] += 1
    msg = X.describe_mismatch(~(got == want), got, want, c)
    assert "last row and column of a ragged tile" in msg and "64 x 64 tile 1,1" in msg and "tile border" in msg
    c = CASES["load_f32_t128_KVEC_ROWS_swap"]
    want = X.expected_of(X.reference(c)["r"], "f32")
    got = want.clone()
    got[200, 3, 70] += 1
    assert "batch 200, 128 x 128 tile 0,0 (operands swapped)" in X.describe_mismatch(~(got == want), got, want, c)
    msg = X.describe_mismatch(torch.tensor([False, True]), torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0]), c, "ar", what="d")
    assert msg == "dar: 1 of 2 values differ (shape (2,))\n  (1,): got 2.0, want 3.0"
