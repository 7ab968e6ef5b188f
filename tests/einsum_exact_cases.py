"""Case table, operand builder and exact reference of the bit-exact einsum tests (test_einsum_exact_host.py,
test_gpu_einsum_exact.py).

The operands of csrc/einsum.hip are integers in [-8, 8] here and the upstream gradients integers in [-3, 3], so every product
and every partial sum is an integer far below 2^24 (`well_formed` asserts 128 K < 2^24 per case): exactly representable in
float32 whatever the tile, the load path, the K stage or the MFMA instruction.  Every launch must therefore give

    float32 outputs   exactly the int64 reference (numpy.einsum on the LOGICAL operands, four real products),
    bf16 outputs      exactly torch.tensor(ref, dtype=float32).bfloat16(): ONE round-to-nearest-even of a known value,

over the whole tensor, gradients included.  The reference never sees the planner, a stride or a descriptor.

A case names its equation and the logical shapes of both operands, its dtype, the STORAGE of each operand (`L`: a
permutation of the dimensions, a step and a padding per dimension, an element offset behind a 16-byte aligned address,
stride-0 dimensions; the view is cut out of a NaN-filled buffer, so a read between the elements poisons the result), the API
it goes through ('einsum' cplx.einsum | 'contract' einsum._contract with a conjugation spec | 'cabi' cplxamd_ceinsum
directly on a descriptor with ONE mode per subscript, a padded C whose gaps hold a canary, negated strides) and the dispatch
it was written for: `want` = (mode_a, mode_b, swapped, tile) as cplxamd_einsum_plan reports them, i.e. AFTER the swap.

Constants the shapes are built around (read from csrc/einsum.hip): BK = 16 (float32) / 32 (bf16) per K stage, the k-offset
tables double-buffered by stage parity; KVEC needs the innermost K extent % 4 (float32) / % 8 (bf16), ROWVEC (bf16) the
innermost row extent % 8; the 128 x 128 tile is taken when B ceil(M / 128) ceil(N / 128) >= 256 and max(M, N) > 64.
"""
import functools
import zlib

import numpy as np
import torch

from gemm_exact_cases import expected, rounding_content  # noqa: F401  (shared with the GEMM table)

TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
ESIZE = {"f32": 4, "bf16": 2}
BK = {"f32": 16, "bf16": 32}
VEC = {"f32": 4, "bf16": 8}
MODES = {"f32": ("KFAST", "KVEC", "ROWS"), "bf16": ("KFAST", "KVEC", "ROWS", "ROWVEC")}
CANARY = -77.0                                  # (exact in bf16) what the gaps of a padded C hold
DTYPES = ("f32", "bf16")

CASES = {}


def L(order=None, step=None, pad=None, off=0, expand=()):
    """Storage of a logical tensor: `order` = its dimensions from the outermost to the innermost in memory (None: as
    written), `step[d]` = the view takes every step-th element of dimension d, `pad[d]` = elements of dimension d allocated
    behind the view's, `off` = elements between a 16-byte aligned address and the first one, `expand` = dimensions of
    stride 0 (the values do not depend on them)."""
    return dict(order=order, step=step, pad=pad, off=off, expand=tuple(expand))


def case(name, eq, sa, sb, dtype, la=None, lb=None, api="einsum", conj=(False, False), want=None, family="", cabi=None,
         grad=False, poison=None, seed=0, kseam=None):
    """eq, sa, sb: the equation and the logical shapes of A and B.   la / lb: their storage (`L`).   conj: (conj_a, conj_b)
    ('contract' and 'cabi').   want: (mode_a, mode_b, swapped, tile).   cabi: dict(c=L(...) storage of C, rev_a / rev_b =
    subscripts whose stride is negated in A / B (the base pointer moves to the other end: the kernel reads the operand
    REVERSED along them, and so does the reference)).   grad: also all four gradient planes, through autograd.   poison:
    dict(a=index, b=index) of ONE NaN per operand.   kseam: the K-stage family this case belongs to ('scalar' | 'kvec')."""
    assert name not in CASES, name
    assert dtype in DTYPES and api in ("einsum", "contract", "cabi") and len(want) == 4
    assert (cabi is not None) == (api == "cabi") and (api != "einsum" or conj == (False, False))
    CASES[name] = dict(name=name, eq=eq.replace(" ", ""), sa=tuple(sa), sb=tuple(sb), dtype=dtype, la=la or L(), lb=lb or L(),
                       api=api, conj=tuple(bool(x) for x in conj), want=tuple(want), family=family, cabi=cabi, grad=grad,
                       poison=poison, seed=seed, kseam=kseam)


# ---------------------------------------------------------------------------------------------------------------------------------
#  the table
# ---------------------------------------------------------------------------------------------------------------------------------
T64 = dict(b=2, m=72, n=40)                      # 2 x 1 tiles of 64, both ragged
T128 = dict(b=256, m=72, n=8)                    # 256 x 1 x 1 tiles of 128: the cheapest shape that takes the wide tile
KRAG = {"f32": 20, "bf16": 40}                   # two K stages, the second one a tail; a multiple of the vector
KDEEP = 136                                      # bf16: sums large enough for the rounding to matter (five stages, a tail)


def op_lay(mode, dtype, off=None):
    """Storage of a logical [b, rows, k] operand that takes load path `mode` (the extents allowing)."""
    if mode == "KVEC":
        return L()
    if mode == "KFAST":
        return L(off=1 if off is None else off)
    if mode == "ROWS":
        return L(order=(0, 2, 1), off=(0 if dtype == "f32" else 1) if off is None else off)
    assert mode == "ROWVEC" and dtype == "bf16"
    return L(order=(0, 2, 1))


def bmm(name, dtype, shape, K, ma, mb, tile, swapped=False, **kw):
    """[b, m, k] x [b, n, k] -> [b, m, n] (swapped: [b, n, m], C's unit stride in M) on the load paths ma / mb of A / B."""
    b, m, n = shape["b"], shape["m"], shape["n"]
    la, lb = kw.pop("la", None) or op_lay(ma, dtype), kw.pop("lb", None) or op_lay(mb, dtype)
    case(name, "bmk,bnk->bnm" if swapped else "bmk,bnk->bmn", (b, m, K), (b, n, K), dtype, la, lb,
         want=(mb, ma, True, tile) if swapped else (ma, mb, False, tile), **kw)


_SW = {False: "", True: "_swap"}

# ---- 1. the load-path matrix: every (mode_a, mode_b) on both tiles and in both swap states, ragged M, N and K ------------------
for _dt in DTYPES:
    for _tile, _shape in ((64, T64), (128, T128)):
        for _ma in MODES[_dt]:
            for _mb in MODES[_dt]:
                for _sw in (False, True):
                    bmm(f"load_{_dt}_t{_tile}_{_ma}_{_mb}{_SW[_sw]}", _dt, _shape, KRAG[_dt], _ma, _mb, _tile, _sw, family="load")
    # KFAST the other ways: a K extent that is no multiple of the vector; the gather (no unit stride at all: every other element)
    bmm(f"load_{_dt}_t64_kfast_odd_extent", _dt, T64, KRAG[_dt] + 1, "KFAST", "KFAST", 64, la=L(), lb=L(), family="load")
    bmm(f"load_{_dt}_t64_gather", _dt, T64, KRAG[_dt], "KFAST", "KFAST", 64, la=L(step=(1, 1, 2)), lb=L(step=(1, 2, 2)), family="load")
    bmm(f"load_{_dt}_t128_gather", _dt, T128, KRAG[_dt], "KFAST", "KFAST", 128, la=L(step=(1, 1, 2)), lb=L(step=(1, 2, 2)),
        family="load")
    # one case that fills all 2 x 2 sub-tiles of every wave of the wide tile: 64 x 2 x 2 tiles
    _full = dict(b=64, m=136, n=136)
    for _md in ("KVEC", MODES[_dt][-1]):
        for _sw in (False, True):
            bmm(f"load_{_dt}_t128_full_{_md}{_SW[_sw]}", _dt, _full, KRAG[_dt], _md, _md, 128, _sw, family="load")
# bf16 ROWS the other way: aligned storage whose row extent is no multiple of 8
bmm("load_bf16_t64_rows_odd_extent", "bf16", dict(b=2, m=71, n=37), 40, "ROWS", "ROWS", 64, la=L(order=(0, 2, 1)),
    lb=L(order=(0, 2, 1)), family="load")
# deep K: what makes the bf16 store's rounding visible, per load path, tile and swap state
for _tile, _shape in ((64, T64), (128, T128)):
    for _md in MODES["bf16"]:
        for _sw in (False, True):
            bmm(f"deep_bf16_t{_tile}_{_md}{_SW[_sw]}", "bf16", _shape, KDEEP, _md, _md, _tile, _sw, family="deep")
bmm("deep_f32_t64_KVEC", "f32", T64, KDEEP, "KVEC", "KVEC", 64, family="deep")
bmm("deep_f32_t128_ROWS_swap", "f32", T128, KDEEP, "ROWS", "ROWS", 128, True, family="deep")

# ---- 2. K-stage seams: one, two, three and four stages, both parities of the k-offset tables reused -----------------------------
KSEAM = {"f32": (1, 15, 16, 17, 32, 33, 49), "bf16": (1, 31, 32, 33, 64, 65, 97)}
KSEAM_VEC = {"f32": (4, 20, 36), "bf16": (8, 40, 72)}
_KS = dict(b=2, m=40, n=24)
for _dt in DTYPES:
    for _K in KSEAM[_dt]:
        # (an aligned K extent would take KVEC; an extent-1 K mode is dropped, and contiguous rows would take the row path)
        _lay = L(step=(1, 2, 1)) if _K == 1 else L(off=1 if _K % VEC[_dt] == 0 else 0)
        bmm(f"kseam_{_dt}_KFAST_k{_K}", _dt, _KS, _K, "KFAST", "KFAST", 64, la=_lay, lb=_lay, family="kseam", kseam="scalar")
        for _md in MODES[_dt][2:]:
            bmm(f"kseam_{_dt}_{_md}_k{_K}", _dt, _KS, _K, _md, _md, 64, family="kseam", kseam="scalar")
    for _K in (KSEAM[_dt][3], KSEAM[_dt][-1]):                 # two and four stages on the wide tile
        bmm(f"kseam_{_dt}_t128_KFAST_k{_K}", _dt, T128, _K, "KFAST", "KFAST", 128, la=L(), lb=L(), family="kseam", kseam="scalar")
        bmm(f"kseam_{_dt}_t128_{MODES[_dt][-1]}_k{_K}", _dt, T128, _K, MODES[_dt][-1], MODES[_dt][-1], 128, family="kseam",
            kseam="scalar")
    for _K in KSEAM_VEC[_dt]:
        bmm(f"kseam_{_dt}_KVEC_k{_K}", _dt, _KS, _K, "KVEC", "KVEC", 64, family="kseam", kseam="kvec")
        bmm(f"kseam_{_dt}_t128_KVEC_k{_K}", _dt, T128, _K, "KVEC", "KVEC", 128, family="kseam", kseam="kvec")

# ---- 3. M / N tile seams ------------------------------------------------------------------------------------------------------------
MN64, MN128 = (1, 63, 64, 65), (127, 128, 129)
for _dt in DTYPES:
    for _m in MN64:
        for _n in MN64:
            # (N = 1: the N group is empty, C's unit stride lies in M and the operands are swapped)
            bmm(f"mnseam_{_dt}_t64_{_m}x{_n}", _dt, dict(b=2, m=_m, n=_n), BK[_dt] + 1, "KFAST", "KFAST", 64, la=L(), lb=L(),
                family="mnseam")
            if _n == 1 and _m > 1:
                CASES[f"mnseam_{_dt}_t64_{_m}x{_n}"]["want"] = ("KFAST", "KFAST", True, 64)
    for _m in MN128:
        for _n in MN128:
            _b = 256 // (-(-_m // 128) * -(-_n // 128))
            bmm(f"mnseam_{_dt}_t128_{_m}x{_n}", _dt, dict(b=_b, m=_m, n=_n), 3, "KFAST", "KFAST", 128, la=L(), lb=L(), family="mnseam")

# ---- 4. several modes per group (sliced storage: nothing fuses) -------------------------------------------------------------------
for _dt in DTYPES:
    # M = 5 x 13 and N = 3 x 23 cross a tile border in mid-digit; K = 3 x 7 / 5 x 9 cross a stage border in mid-digit
    for _j, _l in ((3, 7), (5, 9)):
        case(f"modes_{_dt}_mn_k{_j}x{_l}", "abjl,cdjl->abcd", (5, 13, _j, _l), (3, 23, _j, _l), _dt, L(pad=(0, 2, 1, 3)),
             L(pad=(0, 1, 0, 2)), want=("KFAST", "KFAST", False, 64), family="modes")
    case(f"modes_{_dt}_mn_k5x9_t128", "zabjl,zcdjl->zabcd", (256, 5, 13, 5, 9), (256, 3, 23, 5, 9), _dt, L(pad=(0, 0, 2, 1, 3)),
         L(pad=(0, 0, 1, 0, 2)), want=("KFAST", "KFAST", False, 128), family="modes")
    # two batch modes, B does not depend on the second one (stride 0)
    case(f"modes_{_dt}_two_batch_stride0", "xymk,xynk->xymn", (3, 4, 33, KRAG[_dt]), (3, 4, 17, KRAG[_dt]), _dt, L(pad=(0, 1, 0, 0)),
         L(expand=(1,)), want=("KVEC", "KVEC", False, 64), family="modes")
    # exactly 8 modes in a group: 2^8 indices from [:2] slices of extent-4 dimensions
    _e8, _p8 = (2,) * 8, (2,) * 8
    case(f"modes_{_dt}_eight_m", "abcdefghk,nk->abcdefghn", _e8 + (VEC[_dt],), (5, VEC[_dt]), _dt, L(pad=_p8 + (0,)), L(),
         want=("KVEC", "KVEC", False, 64), family="modes")
    case(f"modes_{_dt}_eight_n", "mk,abcdefghk->mabcdefgh", (5, VEC[_dt]), _e8 + (VEC[_dt],), _dt, L(), L(pad=_p8 + (0,)),
         want=("KVEC", "KVEC", False, 64), family="modes")
    case(f"modes_{_dt}_eight_k", "mabcdefgh,nabcdefgh->mn", (33,) + _e8, (17,) + _e8, _dt, L(pad=(0,) + _p8), L(),
         want=("KFAST", "KFAST", False, 64), family="modes")

# ---- 5. planner features with an exact answer ------------------------------------------------------------------------------------
for _dt in DTYPES:
    case(f"feat_{_dt}_summed_only_label", "ijk,jl->il", (6, 8, 5), (8, 9), _dt, want=("KFAST", "ROWS", False, 64), family="feat")
    case(f"feat_{_dt}_diagonal", "iij,jk->ik", (8, 8, 12), (12, 5), _dt,
         want=("KVEC" if _dt == "f32" else "KFAST", "ROWS", False, 64), family="feat")
    case(f"feat_{_dt}_ellipsis_broadcast", "...ik,...kj->...ij", (2, 1, 9, 31), (3, 31, 5), _dt,
         want=("KFAST", "ROWS", False, 64), family="feat")
    case(f"feat_{_dt}_hadamard", "ij,ij->ij", (13, 29), (13, 29), _dt, want=("KFAST", "KFAST", False, 64), family="feat")
    case(f"feat_{_dt}_outer", "i,j->ij", (70,), (45,), _dt, want=("ROWS", "ROWS", False, 64), family="feat")
    case(f"feat_{_dt}_dot_k1000", "i,i->", (1000,), (1000,), _dt, want=("KVEC", "KVEC", False, 64), family="feat",
         seed={"f32": 0, "bf16": 63}[_dt])           # (bf16: BOTH values, -702 and 622, are ties that round AWAY from zero)
    case(f"feat_{_dt}_matvec", "ij,j->i", (70, 33), (33,), _dt, want=("KFAST", "KFAST", True, 64), family="feat")

# ---- 6. output orders: C's unit stride in N and in M is family 1; in a batch mode the store is strided ---------------------------
for _dt in DTYPES:
    case(f"order_{_dt}_unit_stride_in_batch", "bmk,bkn->mnb", (5, 70, KRAG[_dt]), (5, KRAG[_dt], 33), _dt,
         want=("KVEC", "ROWS", False, 64), family="order")
    case(f"order_{_dt}_unit_stride_in_batch_t128", "bmk,bkn->mnb", (256, 70, KRAG[_dt]), (256, KRAG[_dt], 8), _dt,
         want=("KVEC", "ROWVEC" if _dt == "bf16" else "ROWS", False, 128), family="order")

# ---- 7. conjugation: all four flag pairs, both tiles, with and without the swap (which exchanges the flags) -------------------------
for _dt in DTYPES:
    for _tile, _shape in ((64, T64), (128, T128)):
        for _ca in (False, True):
            for _cb in (False, True):
                for _sw in (False, True):
                    # (A on KVEC and B on the row path: the operands' roles are told apart by their load paths too)
                    _mb = MODES[_dt][-1]
                    bmm(f"conj_{_dt}_t{_tile}_{int(_ca)}{int(_cb)}{_SW[_sw]}", _dt, _shape, KRAG[_dt] + VEC[_dt], "KVEC", _mb, _tile,
                        _sw, api="contract", conj=(_ca, _cb), family="conj")

# ---- 8. the C ABI directly: a padded C with canary gaps, negated strides, nmodes == 0, odd base addresses -----------------------
for _dt in DTYPES:
    _K = KRAG[_dt]
    _row = MODES[_dt][-1]
    case(f"cabi_{_dt}_padded_c", "bmk,bnk->bmn", (2, 72, _K), (2, 40, _K), _dt, L(), op_lay(_row, _dt), api="cabi",
         conj=(False, True), cabi=dict(c=L(pad=(0, 2, 3))), want=("KVEC", _row, False, 64), family="cabi")
    case(f"cabi_{_dt}_padded_c_swap_t128", "bmk,bnk->bnm", (256, 72, _K), (256, 8, _K), _dt, L(), op_lay(_row, _dt), api="cabi",
         conj=(True, False), cabi=dict(c=L(pad=(0, 1, 5))), want=(_row, "KVEC", True, 128), family="cabi")
    case(f"cabi_{_dt}_padded_c_strided_store", "bmk,bnk->bmn", (2, 72, _K), (2, 40, _K), _dt, L(off=1), L(off=1), api="cabi",
         cabi=dict(c=L(step=(1, 1, 2), pad=(1, 0, 1))), want=("KFAST", "KFAST", False, 64), family="cabi")
    # negative strides: A's rows in reversed order (K stays contiguous), B's K in reversed order
    case(f"cabi_{_dt}_reversed_rows_of_a", "bmk,bnk->bmn", (2, 72, _K), (2, 40, _K), _dt, L(), L(), api="cabi",
         cabi=dict(c=L(pad=(0, 0, 1)), rev_a="m"), want=("KVEC", "KVEC", False, 64), family="cabi")
    case(f"cabi_{_dt}_reversed_k_of_b", "bmk,bnk->bmn", (2, 72, _K + 1), (2, 40, _K + 1), _dt, L(), L(), api="cabi",
         conj=(True, True), cabi=dict(c=L(pad=(0, 0, 1)), rev_b="k"), want=("KFAST", "KFAST", False, 64), family="cabi")
    case(f"cabi_{_dt}_reversed_rows_of_b_rowpath_t128", "bmk,bnk->bmn", (256, 72, _K), (256, 8, _K), _dt, L(),
         L(order=(0, 2, 1)), api="cabi", cabi=dict(c=L(pad=(0, 0, 8)), rev_b="n", rev_a="k"), want=("KFAST", "KFAST", False, 128),
         family="cabi")
    # nmodes == 0 stands for one mode of extent 1: no batch; no M and no N; no K (zeros are written... here: an outer product)
    case(f"cabi_{_dt}_no_batch_group", "mk,nk->mn", (70, _K), (33, _K), _dt, api="cabi", cabi=dict(c=L(pad=(0, 3))),
         want=("KVEC", "KVEC", False, 64), family="cabi")
    case(f"cabi_{_dt}_no_m_no_n_group", "bk,bk->b", (37, _K), (37, _K), _dt, api="cabi", conj=(False, True),
         cabi=dict(c=L(step=(2,))), want=("KVEC", "KVEC", False, 64), family="cabi")
    case(f"cabi_{_dt}_no_k_group", "bm,bn->bmn", (3, 70), (3, 33), _dt, api="cabi", conj=(True, False), cabi=dict(c=L(pad=(0, 0, 2))),
         want=("ROWS", "ROWS", False, 64), family="cabi")
    # odd base addresses of A, B and C
    case(f"cabi_{_dt}_odd_bases", "bmk,bnk->bmn", (2, 72, _K), (2, 40, _K), _dt, L(off=3), L(order=(0, 2, 1), off=1), api="cabi",
         cabi=dict(c=L(off=1, pad=(0, 0, 1))), want=("KFAST", "ROWS", False, 64), family="cabi")

# ---- 9. gradients through cplx.einsum + autograd: one case per feature -------------------------------------------------------------
# The BACKWARD contractions reduce over other extents than the forward: dA over N (and what A is broadcast along), dB over M.
# With |g| <= 3 a complex sum of T terms has a standard deviation of sqrt(192 T): those extents are ~600 here, so that a fifth
# of every bf16 gradient plane changes under the ONE rounding it is held to (asserted on the host, plane by plane).
for _dt in DTYPES:
    _g = dict(grad=True, family="grad")
    case(f"grad_{_dt}_bmm", "bmk,bkn->bmn", (2, 601, 21), (2, 21, 597), _dt, want=("KFAST", "ROWS", False, 64), **_g)
    case(f"grad_{_dt}_heads", "bhqd,bhkd->bhqk", (1, 2, 601, 16), (1, 2, 597, 16), _dt, want=("KVEC", "KVEC", False, 64), **_g)
    case(f"grad_{_dt}_out_perm", "bmk,bkn->nbm", (2, 601, 21), (2, 21, 597), _dt, want=("ROWS", "KFAST", True, 64), **_g)
    case(f"grad_{_dt}_two_k_modes", "mjk,jkn->mn", (601, 5, 9), (5, 9, 597), _dt, L(pad=(0, 0, 2)), L(),
         want=("KFAST", "ROWS", False, 64), **_g)
    case(f"grad_{_dt}_summed_only_label", "ijk,jl->il", (120, 8, 5), (8, 597), _dt, want=("KFAST", "ROWS", False, 64), **_g)
    case(f"grad_{_dt}_diagonal", "iij,jk->ik", (601, 601, 12), (12, 597), _dt,
         want=("KVEC" if _dt == "f32" else "KFAST", "ROWS", False, 64), **_g)
    case(f"grad_{_dt}_ellipsis_broadcast", "...ik,...kj->...ij", (2, 1, 300, 31), (9, 31, 67), _dt,
         want=("KFAST", "ROWS", False, 64), **_g)
# an operand expanded with .expand(): autograd sums its gradient AFTER the store (a second rounding in bf16), so this one is
# exact in float32 only
case("grad_f32_expanded_operand", "bmk,kn->bmn", (4, 37, 20), (20, 29), "f32", L(expand=(0,)), L(), want=("KVEC", "ROWS", False, 64),
     grad=True, family="grad")
F32_ONLY = {"grad_f32_expanded_operand"}

# ---- 10. non-finite containment: one NaN in A at the last K element of a tail row, one in B ---------------------------------------
for _dt in DTYPES:
    for _tile, _shape in ((64, T64), (128, T128)):
        for _md in ("KVEC", "ROWVEC") if _dt == "bf16" else ("KVEC",):
            _K = KRAG[_dt]
            bmm(f"nan_{_dt}_t{_tile}_{_md}", _dt, _shape, _K, _md, _md, _tile, family="nan",
                poison=dict(a=(1, _shape["m"] - 1, _K - 1), b=(0, 3, BK[_dt] - 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
#  equation -> subscripts, groups (independent of the planner)
# ---------------------------------------------------------------------------------------------------------------------------------
def explicit_eq(c):
    """The equation in letters only: '...' becomes the letters Z, Y, ... (right-aligned, as every einsum reads it)."""
    lhs, rhs = c["eq"].split("->")
    ta, tb = lhs.split(",")
    ell = "ZYXW"

    def term(t, rank):
        if "..." not in t:
            return t
        n = rank - len(t.replace("...", ""))
        return t.replace("...", ell[:n][::-1])

    xa, xb = term(ta, len(c["sa"])), term(tb, len(c["sb"]))
    n = max(sum(ch in ell for ch in xa), sum(ch in ell for ch in xb))
    return xa, xb, rhs.replace("...", ell[:n][::-1])


def extents(c):
    xa, xb, _ = explicit_eq(c)
    ext = {}
    for labs, shape in ((xa, c["sa"]), (xb, c["sb"])):
        for lab, e in zip(labs, shape):
            ext[lab] = max(ext.get(lab, 1), e)
    return ext


def out_shape(c):
    ext = extents(c)
    return tuple(ext[lab] for lab in explicit_eq(c)[2])


def groups(c):
    """-> dict(b, m, n, k): the subscripts of each index group (an operand that is broadcast along a subscript does not carry
    it), batch / M / N in output order, K in order of appearance."""
    xa, xb, xo = explicit_eq(c)
    ext = extents(c)
    in_a = {lab for lab, e in zip(xa, c["sa"]) if e == ext[lab]} | {lab for lab in xa if ext[lab] == 1}
    in_b = {lab for lab, e in zip(xb, c["sb"]) if e == ext[lab]} | {lab for lab in xb if ext[lab] == 1}
    g = dict(b=[], m=[], n=[], k=[])
    for lab in xo:
        g["b" if lab in in_a and lab in in_b else "m" if lab in in_a else "n"].append(lab)
    for lab in list(dict.fromkeys(xa)) + [lab for lab in dict.fromkeys(xb) if lab not in xa]:
        if lab not in xo:
            g["k"].append(lab)
    return g


def totals(c):
    """(B, M, N, K): the products of the groups' extents."""
    ext, g = extents(c), groups(c)
    return tuple(int(np.prod([ext[lab] for lab in g[k]], dtype=np.int64)) for k in "bmnk")


def macs(c):
    B, M, N, K = totals(c)
    return B * M * N * K


def well_formed(c):
    B, M, N, K = totals(c)
    assert 128 * K < 2 ** 24, c["name"]            # |sum| <= 2 K 64: every partial sum is exact in float32
    assert macs(c) <= 1.2e8, c["name"]
    tile = 128 if B * -(-M // 128) * -(-N // 128) >= 256 and max(M, N) > 64 else 64
    assert tile == c["want"][3], c["name"]
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
#  storage
# ---------------------------------------------------------------------------------------------------------------------------------
def geometry(shape, lay):
    """(element strides of the logical dimensions, element offset, elements of the buffer) of a tensor stored as `lay` says."""
    nd = len(shape)
    order = tuple(lay["order"] or range(nd))
    step = tuple(lay["step"] or (1,) * nd)
    pad = tuple(lay["pad"] or (0,) * nd)
    assert sorted(order) == list(range(nd)) and len(step) == len(pad) == nd
    alloc = [1 if d in lay["expand"] else shape[d] * step[d] + pad[d] for d in range(nd)]
    strides, acc = [0] * nd, 1
    for d in reversed(order):
        strides[d] = 0 if d in lay["expand"] else acc * step[d]
        acc *= alloc[d]
    return tuple(strides), lay["off"], lay["off"] + acc


def build_view(vals, lay, dtype, device="cpu", fill=float("nan")):
    """`vals` (a logical tensor; constant along the expanded dimensions) as a view into a fresh buffer filled with `fill`, cut
    out as `lay` says: -> (buffer, view).  The buffer starts at a 16-byte aligned address; what lies between the elements of
    the view must never be read (NaN) or written (the canary)."""
    strides, off, numel = geometry(tuple(vals.shape), lay)
    buf = torch.full((numel,), fill, dtype=dtype, device=device)
    view = buf.as_strided(tuple(vals.shape), strides, off)
    idx = tuple(slice(0, 1) if d in lay["expand"] else slice(None) for d in range(vals.dim()))
    view[idx].copy_(vals[idx].to(dtype))
    return buf, view


# ---------------------------------------------------------------------------------------------------------------------------------
#  operands and the int64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """int64 numpy operands seeded by the case name: ar, ai [sa], br, bi [sb] in [-8, 8] (constant along the dimensions the
    storage expands), and for a gradient case gr, gi [out shape] in [-3, 3]."""
    rs = np.random.RandomState((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7fffffff)
    d = {}
    for op, shape, lay in (("a", c["sa"], c["la"]), ("b", c["sb"], c["lb"])):
        gen = tuple(1 if i in lay["expand"] else e for i, e in enumerate(shape))
        for p in "ri":
            d[op + p] = np.ascontiguousarray(np.broadcast_to(rs.randint(-8, 9, size=gen), shape)).astype(np.int64)
    if c["grad"]:
        for p in "ri":
            d["g" + p] = rs.randint(-3, 4, size=out_shape(c)).astype(np.int64)
    return d


def _flipped(c, d):
    """The operands as the kernel reads them: reversed along the subscripts whose stride a C-ABI case negates."""
    out = dict(d)
    if c["cabi"]:
        xa, xb, _ = explicit_eq(c)
        for op, labs, rev in (("a", xa, c["cabi"].get("rev_a", "")), ("b", xb, c["cabi"].get("rev_b", ""))):
            for lab in rev:
                for p in "ri":
                    out[op + p] = np.flip(out[op + p], labs.index(lab))
    return out


def products(eq, d, conj=(False, False)):
    """re, im of sum conj^ca(A) conj^cb(B) in int64: the four real products."""
    E = lambda x, y: np.einsum(eq, x, y)  # noqa: E731
    sa, sb = (-1 if conj[0] else 1), (-1 if conj[1] else 1)
    ai, bi = sa * d["ai"], sb * d["bi"]
    return {"r": E(d["ar"], d["br"]) - E(ai, bi), "i": E(d["ar"], bi) + E(ai, d["br"])}


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = CASES[name]
    return products(c["eq"], _flipped(c, make_inputs(c)), c["conj"])


def reference(c, conj=None, d=None):
    """{plane: int64 array [out shape]}.  (conj, d: what describe_mismatch's hypotheses vary.)"""
    if conj is None and d is None:
        return _reference(c["name"])
    return products(c["eq"], _flipped(c, d or make_inputs(c)), c["conj"] if conj is None else conj)


def _d_operand(sub_x, shape_x, sub_y, sub_o, ext, y, g):
    """d/dX of sum(g * einsum('x,y->o', X, y)) in int64, X with subscripts sub_x (repeated: a diagonal) and `shape_x` (an
    extent 1 where the subscript is larger elsewhere: a broadcast)."""
    ux = "".join(dict.fromkeys(sub_x))
    have = "".join(lab for lab in ux if lab in sub_o or lab in sub_y)
    dx = np.einsum(f"{sub_o},{sub_y}->{have}", g, y)
    dx = dx.reshape([ext[lab] if lab in have else 1 for lab in ux])
    dx = np.broadcast_to(dx, [ext[lab] for lab in ux])                    # a subscript of X alone: summed away in the forward
    own = {}
    for lab, e in zip(sub_x, shape_x):
        own[lab] = e
    for ax, lab in enumerate(ux):
        if own[lab] == 1 and ext[lab] != 1:                               # broadcast in the forward: summed in the backward
            dx = dx.sum(axis=ax, keepdims=True)
    out = np.zeros(shape_x, dtype=np.int64)
    np.einsum(f"{sub_x}->{ux}", out)[...] = dx                            # (a writeable view of the diagonal)
    return out


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """{ar, ai, br, bi: int64 gradient of sum(re * gr + im * gi)} for a gradient case."""
    c = CASES[name]
    d = make_inputs(c)
    xa, xb, xo = explicit_eq(c)
    ext = extents(c)
    dx = lambda g, y: _d_operand(xa, c["sa"], xb, xo, ext, y, g)  # noqa: E731
    dy = lambda x, g: _d_operand(xb, c["sb"], xa, xo, ext, x, g)  # noqa: E731
    out = {"ar": dx(d["gr"], d["br"]) + dx(d["gi"], d["bi"]), "ai": dx(d["gi"], d["br"]) - dx(d["gr"], d["bi"]),
           "br": dy(d["ar"], d["gr"]) + dy(d["ai"], d["gi"]), "bi": dy(d["ar"], d["gi"]) - dy(d["ai"], d["gr"])}
    for op, lay in (("a", c["la"]), ("b", c["lb"])):                      # an expanded operand: autograd sums over the expansion
        for ax in lay["expand"]:
            for p in "ri":
                out[op + p] = out[op + p].sum(axis=ax, keepdims=True)
    return out


def expected_of(ref, dtype):
    """The float32 tensor a kernel must return for the int64 array `ref` (gemm_exact_cases.expected: refuses what float32
    cannot hold, ONE round-to-nearest-even for bf16)."""
    return expected(torch.from_numpy(np.ascontiguousarray(ref).astype(np.float64)), dtype)


def nan_mask(c):
    """Where the result of a poisoned case must be NaN: every output element whose sum contains a poisoned operand element."""
    za, zb = np.zeros(c["sa"], dtype=np.int64), np.zeros(c["sb"], dtype=np.int64)
    za[c["poison"]["a"]] = 1
    zb[c["poison"]["b"]] = 1
    return (np.einsum(c["eq"], za, np.ones_like(zb)) + np.einsum(c["eq"], np.ones_like(za), zb)) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
#  descriptors (the C-ABI cases build theirs here, ONE mode per subscript, without the planner)
# ---------------------------------------------------------------------------------------------------------------------------------
def cabi_plan(c):
    """-> (einsum.Plan with one Mode per subscript and EMPTY groups where the equation has none, element offsets of the base
    pointers of A and B, geometry of C): the descriptor of a C-ABI case.  A negated stride moves the base pointer to the
    other end of that dimension."""
    from cplxmodule_amd import einsum as E
    assert c["api"] == "cabi"
    xa, xb, xo = explicit_eq(c)
    ext, g = extents(c), groups(c)
    sta, a0, _ = geometry(c["sa"], c["la"])
    stb, b0, _ = geometry(c["sb"], c["lb"])
    stc, c0, cn = geometry(out_shape(c), c["cabi"]["c"])
    sa, sb, sc = dict(zip(xa, sta)), dict(zip(xb, stb)), dict(zip(xo, stc))
    for lab in c["cabi"].get("rev_a", ""):
        a0 += (ext[lab] - 1) * sa[lab]
        sa[lab] = -sa[lab]
    for lab in c["cabi"].get("rev_b", ""):
        b0 += (ext[lab] - 1) * sb[lab]
        sb[lab] = -sb[lab]
    mode = lambda lab: E.Mode(ext[lab], sa.get(lab, 0), sb.get(lab, 0), sc.get(lab, 0), lab)  # noqa: E731
    p = E.Plan(*(tuple(mode(lab) for lab in g[k]) for k in "bmnk"), out_shape(c), c["conj"][0], c["conj"][1], "kernel")
    return p, a0, b0, (stc, c0, cn)


def host_plan(c):
    """-> (einsum.Plan handed to the kernel, element offsets of A's and B's base pointers) for every API."""
    from cplxmodule_amd import einsum as E
    if c["api"] == "cabi":
        p, a0, b0, _ = cabi_plan(c)
        return p, a0, b0
    sta, a0, _ = geometry(c["sa"], c["la"])
    stb, b0, _ = geometry(c["sb"], c["lb"])
    dt = TORCH_DTYPE[c["dtype"]]
    if c["api"] == "einsum":
        ins, out = E.parse(c["eq"], [c["sa"], c["sb"]])
        ext = E.label_extents(ins, [c["sa"], c["sb"]])
        xs, ys = E.normalize(ins[0], c["sa"], sta, ext), E.normalize(ins[1], c["sb"], stb, ext)
        return E.contraction_plan(xs, ys, out, ext, dt), a0, b0
    xa, xb, xo = explicit_eq(c)
    return E.contraction_plan(dict(zip(xa, sta)), dict(zip(xb, stb)), tuple(xo), extents(c), dt, c["conj"]), a0, b0


def declared_addresses(c, a0, b0):
    """Addresses with the alignment the case's storage declares (a 16-byte aligned buffer + the element offset)."""
    es = ESIZE[c["dtype"]]
    return (4096 + a0 * es, 8192 + a0 * es, 12288 + b0 * es, 16384 + b0 * es)


# ---------------------------------------------------------------------------------------------------------------------------------
#  mismatch reports that name the seam
# ---------------------------------------------------------------------------------------------------------------------------------
def _flat_mn(c, idx):
    """(b, m, n): the flat batch / M / N index of output coordinate `idx`."""
    xo, ext, g = explicit_eq(c)[2], extents(c), groups(c)
    out = []
    for k in "bmn":
        f = 0
        for lab in g[k]:
            f = f * ext[lab] + idx[xo.index(lab)]
        out.append(f)
    return tuple(out)


def _seams(c, idx):
    B, M, N, K = totals(c)
    t = c["want"][3]
    b, m, n = _flat_mn(c, idx)
    out = []
    last = [w for w, hit in (("row", M % t and m == M - 1), ("column", N % t and n == N - 1)) if hit]
    if last:
        out.append("last " + " and ".join(last) + " of a ragged tile")
    if m % t in (0, t - 1) or n % t in (0, t - 1):
        out.append("tile border")
    out.append(f"batch {b}, {t} x {t} tile {m // t},{n // t}" + (" (operands swapped)" if c["want"][2] else ""))
    return ", ".join(out)


def _without_last_stage(c):
    """The reference that lacks the last K stage, and the flat k it starts at (None: one stage only, or no plain K order)."""
    xa, xb, xo = explicit_eq(c)
    g, ext = groups(c), extents(c)
    K = totals(c)[3]
    cut = (K - 1) // BK[c["dtype"]] * BK[c["dtype"]]
    if cut == 0 or len(set(xa)) != len(xa) or len(set(xb)) != len(xb) or c["cabi"] and (c["cabi"].get("rev_a") or c["cabi"].get("rev_b")):
        return None, cut
    keep = (np.arange(K) < cut).reshape([ext[lab] for lab in g["k"]])
    d = dict(make_inputs(c))
    for op, labs in (("a", xa), ("b", xb)):
        if all(lab in labs for lab in g["k"]):
            shape = [ext[lab] if lab in g["k"] else 1 for lab in labs]
            perm = [g["k"].index(lab) for lab in labs if lab in g["k"]]
            mask = np.transpose(keep, perm).reshape(shape)
            for p in "ri":
                d[op + p] = d[op + p] * mask
            return reference(c, d=d), cut
    return None, cut


def _truncated(want_exact):
    """bf16 by truncation (the low 16 bits dropped) instead of round-to-nearest-even."""
    bits = want_exact.to(torch.float32).contiguous().view(torch.int32)
    return (bits & ~0xffff).view(torch.float32)


def hypotheses(c, plane):
    """[(sentence, float32 tensor the kernel would have returned)]: a lost last K stage, a truncating bf16 store, one
    conjugation flag flipped."""
    out = []
    short, cut = _without_last_stage(c)
    if short is not None:
        out.append((f"the result lacks exactly the last K stage (k >= {cut})", expected_of(short[plane], c["dtype"])))
    if c["dtype"] == "bf16":
        out.append(("the values are the reference TRUNCATED to bf16, not rounded to nearest even",
                    _truncated(expected_of(reference(c)[plane], "f32"))))
    for which, conj in (("A", (not c["conj"][0], c["conj"][1])), ("B", (c["conj"][0], not c["conj"][1]))):
        out.append((f"the result is that of the conjugation flag of {which} flipped",
                    expected_of(reference(c, conj=conj)[plane], c["dtype"])))
    return out


def describe_mismatch(bad, got, want, c, plane="r", limit=6, what="C"):
    """'' if `bad` (a bool tensor of the output's shape) is False everywhere, else a sentence: how many values differ, the
    first few (index, got, want) with the tile and the seam each lies on, and which host-side hypothesis explains ALL the
    differences (a lost last K stage, truncation, a flipped conjugation), if one does."""
    count = int(bad.sum())
    if count == 0:
        return ""
    lines = [f"{what}{plane}: {count} of {bad.numel()} values differ (shape {tuple(bad.shape)})"]
    for idx in bad.nonzero()[:limit].cpu().tolist():
        g, w = float(got[tuple(idx)]), float(want[tuple(idx)])
        where = ""
        if what == "C":
            try:
                where = f"  [{_seams(c, idx)}]"
            except Exception:       # noqa: BLE001  (the report must not hide the mismatch it reports)
                pass
        lines.append(f"  {tuple(idx)}: got {g!r}, want {w!r}{where}")
    if what == "C" and not c["poison"]:
        try:
            gc, bc = got.cpu(), bad.cpu()
            for sentence, alt in hypotheses(c, plane):
                if bool((gc[bc] == alt[bc]).all()):
                    lines.append("  " + sentence)
        except Exception:           # noqa: BLE001
            pass
    return "\n".join(lines)
