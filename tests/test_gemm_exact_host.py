"""Host-side checks of the bit-exact GEMM cases (gemm_exact_cases.py): every case selects the kernel it was written for,
stays exactly representable, and -- where its sums are large enough -- actually exercises the bf16 rounding."""
import numpy as np
import pytest
import torch

import gemm_exact_cases as G
from gemm_exact_cases import CASES

NUMPY_MAX_MACS = 3e7          # the int64 numpy product takes a fraction of a second below this


def test_case_names_are_unique():
    with pytest.raises(AssertionError):
        G.case(next(iter(CASES)), True, 8, 8, 32)
    assert all(c["name"] == n for n, c in CASES.items())


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if G.plan_checked(c)])
def test_case_takes_the_kernel_it_names(name):
    """The dispatch of csrc/gemm.hip as a pure function (cplxamd_gemm_plan), at the 256 compute units the table assumes."""
    from cplxmodule_amd import _lib
    c = CASES[name]
    got = _lib.load().cplxamd_gemm_plan(*G.plan_args(c))
    assert got == c["kind"], (G.KIND_NAME.get(got, got), G.KIND_NAME[c["kind"]])


def test_cases_outside_the_plan_say_why():
    for n, c in CASES.items():
        if not G.plan_checked(c):
            assert (c["dtype"] != "bf16" or c["api"] in ("batched", "x3") or "3m" in c["epi"] or c["strides"] or c["a_off"]), n
        if c["kind"] is not None:
            assert c["dtype"] == "bf16" and c["kind"] in G.KIND_NAME, n


def test_every_kernel_kind_and_entry_point_has_a_case():
    assert {c["kind"] for c in CASES.values() if G.plan_checked(c)} == set(range(7))
    assert {c["entry"] for c in CASES.values()} == set(G.ENTRY)
    # ... on both sides of every switch the table is built around
    have = {(c["entry"], c["lay"], c["out"]) for c in CASES.values()}
    for e in ("cgemm", "rgemm"):
        assert {(e, lay, o) for lay in ("NN", "NT", "TN", "TT") for o in ("bf16", "f32")} <= have
    assert {c["beta"] for c in CASES.values() if "acc" in c["epi"]} == {None, 0.5, -2.0}
    assert {c["mode"] for c in CASES.values() if c["api"] == "x3"} == {"x3", "x2"}
    assert {c["lay"] for c in CASES.values() if c["api"] == "x3"} == {"NN", "NT", "TT"}
    assert {c["K"] for c in CASES.values() if c["kind"] == 2} == {384, 416, 448}         # the ring remainders 0, 1, 2
    assert any(c["ldc"] == c["N"] + 8 for c in CASES.values()) and any(c["ldc"] == c["N"] + 1 for c in CASES.values())


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_well_formed(name):
    c = CASES[name]
    assert 2 * c["K"] * 64 + 8 < 2 ** 24 and G.magnitude_bound(c) < 2 ** 24
    if c["beta"] is not None:
        assert "acc" in c["epi"] and c["beta"] in (0.5, -2.0)
    if c["epi"] & {"acc", "emul", "emul_exp"}:
        assert c["out"] == "f32"
    if "emul_exp" in c["epi"]:
        assert not c["cplx"] and not c["epi"] & {"acc", "emul"}       # exp_check's bound is on acc * exp(m) alone
    if "lrt" in c["epi"]:
        assert c["lay"] == "NT" and c["out"] == "bf16" and c["epi"] == {"lrt"} and c["conj_b"] == c["cplx"]
    if c["dtype"] == "f16":
        assert c["out"] == "f32" and (c["scales"] is None or all(abs(e) <= 4 for e in c["scales"]))
    if c["ldc"] is not None:
        assert c["api"] == "cabi" and c["ldc"] > c["N"]
    if c["ta"] and c["dtype"] != "f32" and not c["strides"] and c["kind"] != 0:
        assert c["M"] % 8 == 0                                        # what the K-major reads of the fast kernels take
    if c["tb"] and c["dtype"] != "f32" and not c["strides"] and c["kind"] != 0:
        assert c["N"] % 8 == 0


_SMALL = [n for n, c in CASES.items() if G.macs(c) <= NUMPY_MAX_MACS]


@pytest.mark.parametrize("name", _SMALL)
def test_reference_equals_numpy_int64(name):
    """The float64 torch reference against integer arithmetic; every operand is what the docstring says it is and survives
    the cast to the case's input type."""
    c = CASES[name]
    d = G.make_inputs(c)
    for k, v in d.items():
        lim = {"a": 8, "b": 8, "x": 8, "g": 3, "c": 64, "e": 8, "l": 2}[k[0]] if not k.startswith("bias") else 8
        assert float(v.abs().max()) <= lim, k
        if k[0] in "abxg" and not k.startswith("bias"):
            assert bool((v == v.round()).all()) and bool((v.to(G.TORCH_DTYPE[c["dtype"]]).double() == v).all()), k
    i64 = lambda k: d[k].numpy().astype(np.int64)  # noqa: E731
    mm = lambda a, b: np.matmul(i64(a), np.swapaxes(i64(b), -1, -2))  # noqa: E731
    if c["cplx"]:
        s = -1 if c["conj_b"] else 1
        want = {"r": mm("ar", "br") - s * mm("ai", "bi"), "i": s * mm("ar", "bi") + mm("ai", "br")}
    else:
        want = {"r": mm("ar", "br")}
    got = G.products(c, d)
    assert sorted(got) == sorted(want)
    for p in want:
        assert got[p].dtype == torch.float64 and np.array_equal(got[p].numpy(), want[p].astype(np.float64)), p
        assert np.abs(want[p]).max() <= 2 * c["K"] * 64
    ref = G.reference(c, d)
    for p in ref:
        if "bias" in c["epi"] and not c["epi"] & {"emul", "acc"}:
            assert np.array_equal(ref[p].numpy(), want[p] + d["bias" + p].numpy())
        G.expected(ref[p], "f32")                                     # (raises unless float32 holds it)
    if "emul" in c["epi"]:
        j = np.log2(d["emul"].numpy())
        assert np.array_equal(j, np.round(j)) and np.abs(j).max() <= 3
    if "emul_exp" in c["epi"]:
        zeros = float((d["lmul"] == 0).double().mean())
        assert 0.45 < zeros < 0.6 and bool((d["lmul"].float().double() == d["lmul"]).all())


def test_inputs_are_seeded_by_the_case_name():
    a, b = CASES["k1_c_full_k128"], CASES["k1_c_ragged_plain_bf16"]
    assert torch.equal(G.make_inputs(a)["ar"], G.make_inputs(a)["ar"])
    assert not torch.equal(G.make_inputs(a)["ar"][:, :128], G.make_inputs(b)["ar"][:256])


def test_expected_refuses_what_float32_cannot_hold():
    ok = torch.tensor([1.0, -0.5, 2.0 ** 24, 3.0 * 2.0 ** 30], dtype=torch.float64)
    assert torch.equal(G.expected(ok, "f32").double(), ok)
    for v in (2.0 ** 24 + 1, 0.1, 2.0 ** 23 + 0.5):
        with pytest.raises(ValueError):
            G.expected(torch.tensor([1.0, v], dtype=torch.float64), "f32")
        with pytest.raises(ValueError):
            G.expected(torch.tensor([1.0, v], dtype=torch.float64), "bf16")


def test_expected_rounds_once_to_nearest_even():
    # bf16 keeps 8 significant bits: between 256 and 512 it holds the even integers, 257 and 259 are ties
    v = torch.tensor([255.0, 257.0, 259.0, 258.0, 257.5, 256.5, -257.0, -259.0, 513.0, 515.0, 127.5, 128.5], dtype=torch.float64)
    want = torch.tensor([255.0, 256.0, 260.0, 258.0, 258.0, 256.0, -256.0, -260.0, 512.0, 516.0, 127.5, 128.0])
    assert torch.equal(G.expected(v, "bf16"), want)
    assert G.rounding_content(v) == (9 / 12, 5)


def test_expected_lrt_is_the_documented_double_rounding():
    acc = torch.tensor([257.0, 259.0, 100.0, 1000.0], dtype=torch.float64)
    x, ga = torch.tensor([1.0, -1.0, 8.0, 3.0], dtype=torch.float64), torch.tensor([1.0, 1.0, -3.0, 1.0], dtype=torch.float64)
    # bf16(257) = 256, + 2 = 258 -- one rounding of 259 would give 260;  bf16(259) = 260, - 2 = 258 (257 -> 256 in one);
    # 100 - 48 = 52;  bf16(1000) = 1000, + 6 = 1006 -> 1008
    assert torch.equal(G.expected_lrt(acc, x, ga), torch.tensor([258.0, 258.0, 52.0, 1008.0]))
    assert not torch.equal(G.expected_lrt(acc, x, ga), G.expected(acc + 2 * x * ga, "bf16"))


def test_exp_check_is_exact_on_zeros_and_four_ulps_elsewhere():
    base = torch.tensor([3.0, 3.0, 3.0, 3.0, 3.0, 0.0, 0.0, -100.5], dtype=torch.float64)
    lm = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, -2.0], dtype=torch.float64)
    v = 3.0 * np.exp(1.0)                                      # 8.15..: one float32 ulp is 2^-20
    f = np.float32
    got = torch.tensor([3.0, np.nextafter(f(3), f(4)), f(v), f(v) + f(3 * 2.0 ** -20), f(v) + f(6 * 2.0 ** -20), 0.0, 1e-30,
                        f(-100.5 * np.exp(-2.0))], dtype=torch.float32)
    assert G.exp_check(got, base, lm).tolist() == [False, True, False, False, True, False, True, False]
    assert G.EXP_ULPS == 4


# ---- do the bf16 results exercise the rounding? ------------------------------------------------------------------------------
# A stored bf16 value tests the rounding only if one rounding changes it; an exact tie also tells round-half-even from
# round-half-up.  bf16 holds the integers below 256, so sums must be larger than that: with operands in [-8, 8] (E x^2 = 24)
# a product has variance 576 and a sum of K = 128 of them a standard deviation of 271 (real; complex 384) -- a fifth (three
# tenths) of the values change.  Below K = 128 the sums are too small for that, and those cases -- the ring prologue's fills,
# the layouts, the generic kernel's odd K -- are listed here by name; each kernel they run has larger cases.
_T = ("c", "r")
TOO_SHALLOW = (
    {f"k1_{t}_full_k{k}" for t in _T for k in (32, 64, 96)} | {f"k1_{t}_sliver_bf16" for t in _T}
    | {f"k1_r_{lay}_bf16" for lay in ("NN", "NT", "TN", "TT")}
    | {f"k1_c_{lay}_bf16{cj}" for lay in ("NN", "NT", "TN", "TT") for cj in ("", "_conj")}
    | {f"gen_{t}_bf16_{w}" for t in _T for w in ("misaligned", "k40")}
    | {n for n in CASES if n.startswith("gauss_264x136x96_") and "_bf16" in n}
)
_BF16_OUT = [n for n, c in CASES.items() if c["out"] == "bf16"]


def test_shallow_cases_are_the_listed_ones():
    assert {n for n in _BF16_OUT if CASES[n]["K"] < 128} == TOO_SHALLOW
    assert sum(n.startswith("gauss_264x136x96_") for n in TOO_SHALLOW) == 6


@pytest.mark.parametrize("name", [n for n in _BF16_OUT if n not in TOO_SHALLOW])
def test_bf16_case_exercises_the_rounding(name):
    """At least 15 % of the expected values change under the rounding and at least 16 are exact ties (the weakest measured
    kind of case, real at K = 128, has 19 %): a condition on the INPUTS, so that no case silently tests nothing."""
    c = CASES[name]
    ref = G.reference(c, G.make_inputs(c))
    for p, v in ref.items():
        changed, ties = G.rounding_content(v)
        assert changed >= 0.15 and ties >= 16, (p, changed, ties)


# ---- the seams the reports name ----------------------------------------------------------------------------------------------
def test_workgroup_order_and_split_plan_mirror_the_kernels():
    wg = G.workgroup_of_tile(17, 16)                      # 4352 x 2048 complex, 4352 x 4096 real
    assert sorted(wg.values()) == list(range(272))
    assert sum(v >= G.NCU for v in wg.values()) == 16     # 16 workgroups run a second tile
    assert G.split_plan(CASES["slab_c_TT_even_k4096"]) == (4, 1024)
    assert G.split_plan(CASES["slab_c_TT_uneven_k4288"]) == (4, 1088)                # 3 x 1088 + 1024
    assert G.split_plan(CASES["slab_c_TT_ragged_chunk_k4160"]) == (4, 1056)          # 3 x 1056 + 992
    assert G.split_plan(CASES["slab_c_TT_over_threshold_k2080"]) == (2, 1056)
    assert G.split_plan(CASES["slab_r_TT_k4096"]) == (4, 1024)


def test_describe_mismatch_names_the_seam():
    c = CASES["k1_c_ragged_plain_bf16"]                   # 257 x 136 on 256 x 128 tiles
    d = G.make_inputs(c)
    want = G.expected(G.reference(c, d)["i"], "bf16")
    assert G.describe_mismatch(~(want == want), want, want, c, "i") == ""
    assert G.describe_mismatch(~(-0.0 * want == 0.0 * want), want, want, c, "i") == ""        # by value
    got = want.clone()
    got[256, 7] += 1
    got[3, 135] = float("nan")
    got[255, 128] += 2
    msg = G.describe_mismatch(~(got == want), got, want, c, "i")
    assert msg.startswith("Ci: 3 of ") and "(256, 7)" in msg and "last row of a ragged tile" in msg
    assert "last column of a ragged tile" in msg and "got nan" in msg and "256 x 128 tile 0,1" in msg and "tile border" in msg
    c = CASES["k2_r_NN_k384"]
    bad = torch.zeros(c["M"], c["N"], dtype=torch.bool)
    wg = G.workgroup_of_tile(17, 16)
    tm, tn = next(t for t, v in wg.items() if v >= G.NCU)
    bad[tm * 256 + 5, tn * 256 + 9] = True
    z = torch.zeros(c["M"], c["N"])
    assert "SECOND-round tile" in G.describe_mismatch(bad, z, z, c)
    tm, tn = next(t for t, v in wg.items() if v == 3)
    bad[:] = False
    bad[tm * 256 + 5, tn * 256 + 9] = True
    assert "workgroup 3's first tile" in G.describe_mismatch(bad, z, z, c)
    # a slab case that lost one split
    c = CASES["slab_c_TT_uneven_k4288_bias_emul_acc"]
    d = G.make_inputs(c)
    ref = G.reference(c, d)["r"]
    short = dict(d, ar=d["ar"].clone())
    short["ar"][:, 2 * 1088:3 * 1088] = 0
    short["ai"] = d["ai"].clone()
    short["ai"][:, 2 * 1088:3 * 1088] = 0
    got = G.reference(c, short)["r"]
    msg = G.describe_mismatch(~(got == ref), got, ref, c, "r", d)
    assert "4 K splits of 1088 (last 1024)" in msg and "lacks exactly split 2 of 4 (k in [2176, 3264))" in msg
