"""Case table, operand generator and exact reference of the bit-exact GEMM tests (test_gemm_exact_host.py,
test_gpu_gemm_exact.py).

The operands are small integers -- activations, weights and gradients in [-8, 8], biases in {k/2 : |k| <= 16}, an old C
of integers in [-64, 64], multipliers 2^j with |j| <= 3, beta in {1, 0.5, -2} -- so every product and every partial sum is
an integer (or a dyadic fraction) far below 2^24: exactly representable in float32 whatever the order of accumulation, the
tile shape, the split-K schedule or the MFMA instruction.  Every route through csrc/gemm.hip must therefore give

    float32 outputs   exactly the float64 reference  C = ((A op(B)^T + bias) * emul) + beta * C_old,
    bf16 outputs      exactly torch.tensor(ref, dtype=float32).bfloat16(): ONE round-to-nearest-even of a known value,

over the whole tensor.  The range [-8, 8] (the convolution cases use [-3, 3]) is what makes a bf16 output test its
rounding: at K = 128 a fifth of the real and three tenths of the complex sums change under one rounding, thousands of them
exact ties (test_gemm_exact_host.py asserts this of every case).

Two epilogues are not a single rounding of the reference, and `expected_lrt` / `exp_check` below say what they are instead:
the fused LRT input gradient rounds twice by its documented arithmetic (csrc/gemm.h), and `emul_exp` multiplies by expf,
which is not exact -- the ONE tolerance of these tests (EXP_ULPS).

The split-product drivers of x3.py run on integer float32 operands: an integer in [-8, 8] IS its first piece and the other
pieces are zero, so this checks the piece views, the K-concatenation offsets, the stacking and the scale undo -- NOT the
cross products of the low pieces, which are all zero here (tests/test_gpu_x3.py bounds those).

A case names the C entry point it must run (`entry`: a key of ENTRY) and, for bf16 operands, the kernel the dispatcher
must pick at 256 CUs (`kind`: the code cplxamd_gemm_plan reports).  The operands are laid out as the kernels see them:
C[m, n] = sum_k A[m, k] op(B[n, k]) with A[m, k] at a[m * a_rs + k * a_cs], B[n, k] at b[n * b_rs + k * b_cs]; layout "N"
is K-contiguous (cs == 1), "T" is K-major (rs == 1).

Tile constants the shapes are built around (read from the kernels): the bf16 / half families work on 256 x 128 (complex)
and 256 x 256 (real) output tiles and 32-wide K tiles through a 3-stage ring; the one-wave-per-SIMD family takes whole
tiles and K % 64 == 0, K >= 128; split-K asks for fewer than 192 tiles, K >= 2048 and gives every split at least 32 K
tiles; the persistent forms want more tiles than CUs and K >= 384 (8-wave).
"""
import zlib

import torch

from cplxmodule_amd import _lib

ENTRY = {
    "cgemm": "cplxamd_cgemm_fl", "rgemm": "cplxamd_rgemm_fl", "clrt": "cplxamd_cgemm_lrt_dx_fl",
    "rlrt": "cplxamd_rgemm_lrt_dx_fl", "batched": "cplxamd_cgemm_batched", "csc": "cplxamd_cgemm_sc_fl",
    "rsc": "cplxamd_rgemm_sc_fl",
}
COMPUTE = frozenset(ENTRY.values())           # everything else ops.py / x3.py call around a GEMM is data movement
KIND_NAME = {0: "generic", 1: "eight-wave one-tile", 2: "eight-wave persistent", 3: "one-wave-per-SIMD", 4: "split-K slabs",
             5: "split-K slabs (one-wave-per-SIMD)", 6: "one-wave-per-SIMD persistent"}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
DTYPE_CODE = {"f32": _lib.F32, "bf16": _lib.BF16, "f16": _lib.F16}

NCU = 256                                      # the table is written for 256 compute units
BK = 32
EXP_ULPS = 4                                   # emul_exp: float32 ulps of acc * exp(m) -- the only tolerance here
CANARY = -77.0                                 # (exact in bf16) what the padding columns of a padded C hold

SHARED, EXCLUSIVE, FAMILY = _lib.LAUNCH_SHARED, _lib.LAUNCH_EXCLUSIVE, _lib.LAUNCH_FAMILY
K1, K2, K3, K6 = FAMILY(0) | SHARED, FAMILY(0) | EXCLUSIVE, FAMILY(0xff) | SHARED, FAMILY(0xff) | EXCLUSIVE

CASES = {}


def case(name, cplx, M, N, K, lay="NN", conj_b=False, dtype="bf16", out=None, epi=(), beta=None, flags=0, lda=None,
         ldb=None, ldc=None, entry=None, kind=None, api="ops", plan=True, strides=None, a_off=0, batch=1, scales=None,
         mode=None, seed=0):
    """lay: layouts of A and B, 'N' K-contiguous | 'T' K-major.   out: output dtype (None: as the input).
    epi: any of 'bias', 'acc' (C = result + beta * C_old; beta None = 1), 'emul', 'emul_exp', 'lrt' (the fused LRT input
    gradient), '3m' (Gauss, algo = 1).   flags: _lib.launch_policy of the call.   lda / ldb / ldc: leading dimensions
    (None: dense).   api: 'ops' ops.cgemm / ops.rgemm | 'cabi' the C entry point directly (a padded C with canary columns) |
    'lrt' ops._cplx_lrt_dx / ops._real_lrt_dx | 'batched' ops.cgemm_batched | 'x3' the split-product drivers of x3.py
    (`mode` 'x3' | 'x2'; `lay` picks gemm_nn / gemm_nt / gemm_tt).   kind: what cplxamd_gemm_plan must report (bf16
    operands; None: not a bf16 4M launch); plan = False: the plan cannot see why the fast path declines (a misaligned
    pointer), the case is exempt from the dispatch check.   strides: (a_rs, a_cs, b_rs, b_cs) of the generic kernel's
    arbitrary views.   a_off: elements the A planes start into their 16-byte aligned buffers.   batch: batch entries
    ('batched').   scales: (ea, eb), the half operands carry 2^ea, 2^eb and the kernel undoes them."""
    assert name not in CASES, name
    epi = frozenset((epi,) if isinstance(epi, str) else epi)
    assert epi <= {"bias", "acc", "emul", "emul_exp", "lrt", "3m"} and len(lay) == 2 and set(lay) <= set("NT")
    if entry is None:
        entry = ("clrt" if cplx else "rlrt") if "lrt" in epi else ("csc" if cplx else "rsc") if dtype == "f16" else \
            ("cgemm" if cplx else "rgemm")
    CASES[name] = dict(name=name, cplx=cplx, M=M, N=N, K=K, ta=lay[0] == "T", tb=lay[1] == "T", lay=lay, conj_b=conj_b,
                       dtype=dtype, out=out or dtype, epi=epi, beta=beta, flags=flags, lda=lda, ldb=ldb, ldc=ldc, entry=entry,
                       kind=kind, api=api, plan=plan, strides=strides, a_off=a_off, batch=batch, scales=scales, mode=mode,
                       seed=seed)


_CR = {True: "c", False: "r"}
FULL = {True: (256, 128), False: (256, 256)}             # one whole tile
RAGGED = {True: (257, 136), False: (260, 264)}           # four tiles, the last row / column of tiles ragged ("N" rows only)
RAGGED8 = {True: (264, 136), False: (264, 264)}          # the same with M % 8 == N % 8 == 0: what the "T" layouts take
BETAS = (None, 0.5, -2.0)
_btag = lambda b: "1" if b is None else str(b).replace("-", "m").replace(".", "p")  # noqa: E731

# ---- 1. the eight-wave one-tile kernel (kind 1) ---------------------------------------------------------------------------------
for _c in (True, False):
    _t = _CR[_c]
    _one = dict(cplx=_c, flags=K1, kind=1)
    for _K in (32, 64, 96, 128):            # 1, 2, 3, 4 K tiles: the 3-stage ring's prologue at every fill
        case(f"k1_{_t}_full_k{_K}", M=FULL[_c][0], N=FULL[_c][1], K=_K, **_one)
        case(f"k1_{_t}_ragged_bias_f32_k{_K}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=_K, out="f32", epi="bias", **_one)
    for _o in ("bf16", "f32"):
        case(f"k1_{_t}_sliver_{_o}", M=1, N=8, K=64, out=_o, epi="bias", **_one)
        for _lay in ("NN", "NT", "TN", "TT"):
            for _cj in ((False, True) if _c else (False,)):
                case(f"k1_{_t}_{_lay}_{_o}" + ("_conj" if _cj else ""), M=RAGGED8[_c][0], N=RAGGED8[_c][1], K=96, lay=_lay,
                     conj_b=_cj, out=_o, **_one)
        case(f"k1_{_t}_ragged_bias_{_o}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out=_o, epi="bias", conj_b=_c, **_one)
        case(f"k1_{_t}_ragged_plain_{_o}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out=_o, **_one)
        # row-padded operands
        case(f"k1_{_t}_padded_NN_{_o}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out=_o, lda=136, ldb=136, **_one)
        case(f"k1_{_t}_padded_TT_{_o}", M=RAGGED8[_c][0], N=RAGGED8[_c][1], K=128, lay="TT", out=_o, lda=RAGGED8[_c][0] + 8,
             ldb=RAGGED8[_c][1] + 8, **_one)
        # the C ABI directly: a padded C; ldc = N + 8 keeps the LDS-staged store path, ldc = N + 1 takes the direct one
        for _shape, _tag in ((FULL, "full"), (RAGGED, "ragged")):
            for _pad in (8, 1):
                case(f"k1_{_t}_{_tag}_ldc_plus{_pad}_{_o}", M=_shape[_c][0], N=_shape[_c][1], K=128, out=_o, epi="bias",
                     ldc=_shape[_c][1] + _pad, api="cabi", **_one)
    for _b in BETAS:
        case(f"k1_{_t}_ragged_acc_beta{_btag(_b)}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out="f32", epi="acc", beta=_b, **_one)
        case(f"k1_{_t}_TT_acc_beta{_btag(_b)}", M=264, N=136, K=96, lay="TT", conj_b=_c, out="f32", epi="acc", beta=_b, **_one)
    case(f"k1_{_t}_ragged_emul", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out="f32", epi="emul", **_one)
    case(f"k1_{_t}_ragged_bias_emul_acc", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out="f32", epi=("bias", "emul", "acc"),
         beta=0.5, **_one)
    case(f"k1_{_t}_ldc_plus8_emul_acc", M=RAGGED[_c][0], N=RAGGED[_c][1], K=128, out="f32", epi=("emul", "acc"), beta=-2.0,
         ldc=RAGGED[_c][1] + 8, api="cabi", **_one)
case("k1_r_ragged_emul_exp", False, 260, 264, 128, out="f32", epi="emul_exp", flags=K1, kind=1)
case("k1_r_TT_bias_emul_exp", False, 264, 136, 96, lay="TT", out="f32", epi=("bias", "emul_exp"), flags=K1, kind=1)

# ---- 2. the eight-wave persistent kernel (kind 2): 272 tiles on 256 workgroups, 16 of which run a second tile ----------------
# K = 384, 416, 448: 12, 13, 14 K tiles, the ring remainders R = 0, 1, 2 (one instantiation each)
PERSIST = {True: (4352, 2048), False: (4352, 4096)}
for _K in (384, 416, 448):
    _pc = dict(cplx=True, M=4352, N=2048, K=_K, flags=K2, kind=2)
    _pr = dict(cplx=False, M=4352, N=4096, K=_K, flags=K2, kind=2)
    case(f"k2_c_NN_k{_K}", **_pc)
    case(f"k2_c_NT_conj_k{_K}", lay="NT", conj_b=True, **_pc)
    case(f"k2_c_lrt_k{_K}", lay="NT", conj_b=True, epi="lrt", api="lrt", **_pc)
    case(f"k2_r_NN_k{_K}", **_pr)
    case(f"k2_r_NN_f32_k{_K}", out="f32", **_pr)
    case(f"k2_r_NT_k{_K}", lay="NT", **_pr)
    case(f"k2_r_lrt_k{_K}", lay="NT", epi="lrt", api="lrt", **_pr)
case("k2_c_NN_bias_k416", True, 4352, 2048, 416, epi="bias", flags=K2, kind=2)
case("k2_c_NT_conj_bias_k448", True, 4352, 2048, 448, lay="NT", conj_b=True, epi="bias", flags=K2, kind=2)
case("k2_r_NN_bias_k384", False, 4352, 4096, 384, epi="bias", flags=K2, kind=2)
case("k2_r_NT_bias_k416", False, 4352, 4096, 416, lay="NT", epi="bias", flags=K2, kind=2)
case("k2_r_NN_f32_bias_k448", False, 4352, 4096, 448, out="f32", epi="bias", flags=K2, kind=2)
# the boundary: exactly one tile per workgroup is the one-tile kernel, and so is a K loop of 11 tiles
case("k2_c_exactly_256_tiles_is_one_tile", True, 4096, 2048, 384, flags=K2, kind=1)
case("k2_c_11_k_tiles_is_one_tile", True, 4352, 2048, 352, flags=K2, kind=1)

# ---- 3. the one-wave-per-SIMD kernel (kind 3) -----------------------------------------------------------------------------------
W4 = {True: (512, 256), False: (512, 512)}
for _c in (True, False):
    _t = _CR[_c]
    for _K in (128, 192, 256):
        _w = dict(cplx=_c, M=W4[_c][0], N=W4[_c][1], K=_K, flags=K3, kind=3)
        case(f"k3_{_t}_NN_k{_K}", **_w)
        case(f"k3_{_t}_NT_k{_K}", lay="NT", conj_b=_c, **_w)
        case(f"k3_{_t}_lrt_k{_K}", lay="NT", conj_b=_c, epi="lrt", api="lrt", **_w)
        case(f"k3_{_t}_TT_acc_k{_K}", lay="TT", conj_b=_c, out="f32", epi="acc", beta=BETAS[_K // 64 % 3], **_w)
        case(f"k3_{_t}_TT_emul_k{_K}", lay="TT", conj_b=_c, out="f32", epi="emul", **_w)
        case(f"k3_{_t}_NN_bias_f32_k{_K}", out="f32", epi="bias", **_w)
    case(f"k3_{_t}_NN_bias_k192", cplx=_c, M=W4[_c][0], N=W4[_c][1], K=192, epi="bias", flags=K3, kind=3)
    case(f"k3_{_t}_TT_bias_emul_acc_k128", cplx=_c, M=W4[_c][0], N=W4[_c][1], K=128, lay="TT", conj_b=_c, out="f32",
         epi=("bias", "emul", "acc"), beta=0.5, flags=K3, kind=3)
    case(f"k3_{_t}_TN_is_one_tile", cplx=_c, M=W4[_c][0], N=W4[_c][1], K=128, lay="TN", flags=K3, kind=1)
for _K in (128, 192, 256):
    case(f"k3_r_TT_emul_exp_k{_K}", False, 512, 512, _K, lay="TT", out="f32", epi="emul_exp", flags=K3, kind=3)
# the default family's K-depth rule
case("k3_c_default_family_NN_k1024", True, 256, 128, 1024, flags=0, kind=3)
case("k3_c_default_family_NT_k1024_is_one_tile", True, 256, 128, 1024, lay="NT", conj_b=True, flags=0, kind=1)

# ---- 4. the one-wave-per-SIMD persistent kernel (kind 6; real, bf16 out, plain epilogue) ----------------------------------------
case("k6_r_NN_k128", False, 4352, 4096, 128, flags=K6, kind=6)
case("k6_r_NN_k192", False, 4352, 4096, 192, flags=K6, kind=6)
case("k6_r_NT_k4096", False, 4352, 4096, 4096, lay="NT", flags=K6, kind=6)

# ---- 5. split-K slabs (float32 out; the slab-reduce kernel carries the epilogue) --------------------------------------------------
_ALL = ("bias", "emul", "acc")
for _n, _kw in {
    "c_TT_even_k4096": dict(cplx=True, M=256, N=128, K=4096, lay="TT", conj_b=True, flags=FAMILY(0xff), kind=5),      # 4 x 1024
    "c_TT_uneven_k4288": dict(cplx=True, M=256, N=128, K=4288, lay="TT", conj_b=True, flags=FAMILY(0xff), kind=5),    # 3 x 1088 + 1024
    "c_TT_default_family_k4096": dict(cplx=True, M=256, N=128, K=4096, lay="TT", conj_b=True, flags=0, kind=4),
    "c_TT_over_threshold_k2080": dict(cplx=True, M=256, N=128, K=2080, lay="TT", conj_b=True, flags=FAMILY(0xff), kind=4),
    "c_TT_ragged_chunk_k4160": dict(cplx=True, M=256, N=128, K=4160, lay="TT", conj_b=True, flags=FAMILY(0xff), kind=4),  # 3 x 1056 + 992
    "r_TT_k4096": dict(cplx=False, M=256, N=256, K=4096, lay="TT", flags=0, kind=4),
    "c_NN_k4096": dict(cplx=True, M=256, N=128, K=4096, flags=FAMILY(0xff), kind=5),
    "c_NN_ragged_tiles_k4096": dict(cplx=True, M=257, N=136, K=4096, flags=0, kind=4),
}.items():
    case(f"slab_{_n}", out="f32", **_kw)
    case(f"slab_{_n}_bias_emul_acc", out="f32", epi=_ALL, beta=0.5 if _kw["K"] % 128 else -2.0, **_kw)
case("slab_r_TT_k4096_emul_exp", False, 256, 256, 4096, lay="TT", out="f32", epi="emul_exp", flags=0, kind=4)

# ---- 6. Gauss 3M (algo = 1): sums of integers in [-8, 8] are exact in bf16, so the three-product combine is exact too -----------
for _M, _N, _K in ((256, 128, 128), (264, 136, 96)):
    for _li, _lay in enumerate(("NN", "NT", "TT")):
        for _cj in (False, True):
            for _o in ("bf16", "f32"):
                _bias = (_li + _cj + (_o == "f32")) % 2 == 0           # (half of the combinations, every factor on both sides)
                case(f"gauss_{_M}x{_N}x{_K}_{_lay}_{_o}" + ("_conj" if _cj else "") + ("_bias" if _bias else ""), True, _M, _N, _K,
                     lay=_lay, conj_b=_cj, out=_o, epi=("3m", "bias") if _bias else "3m", flags=K1)

# ---- 7. the generic kernel (kind 0) --------------------------------------------------------------------------------------------
for _c in (True, False):
    _t = _CR[_c]
    case(f"gen_{_t}_f32_100x50x40", _c, 100, 50, 40, dtype="f32", epi="bias")
    case(f"gen_{_t}_f32_k1", _c, 100, 50, 1, dtype="f32", epi="bias", conj_b=_c)
    # A[m, k] at 3 k + 123 m, B[n, k] at 7 n + 351 k: neither unit nor a multiple of 8 anywhere
    case(f"gen_{_t}_f32_strided", _c, 100, 50, 40, dtype="f32", epi=("bias", "emul", "acc"), beta=0.5, strides=(123, 3, 7, 351))
    case(f"gen_{_t}_bf16_misaligned", _c, 257, 136, 64, epi="bias", a_off=1, kind=0, plan=False)
    case(f"gen_{_t}_bf16_k40", _c, 257, 136, 40, epi="bias", kind=0)
    case(f"gen_{_t}_bf16_k40_f32_acc", _c, 136, 72, 40, out="f32", lay="TT" if _c else "NT", epi=("emul", "acc"), beta=-2.0, kind=0)
    case(f"gen_{_t}_bf16_k160_rounding", _c, 100, 50, 160, strides=(161, 1, 161, 1), epi="bias")
# the generic kernel's own split-K (the shapes of test_cgemm_f32_generic_split_k: a K that is no multiple of its 16-wide K
# tile, splits whose range is empty)
for _M, _N, _K in ((256, 10, 1568), (10, 1568, 256), (64, 64, 1000), (70, 130, 4100), (3, 5, 777)):
    case(f"gen_c_f32_split_{_M}x{_N}x{_K}", True, _M, _N, _K, dtype="f32", epi="bias", conj_b=_K % 2 == 0)
case("gen_c_f32_split_NT_64x64x1000", True, 64, 64, 1000, lay="NT", dtype="f32", conj_b=True)
case("gen_r_f32_split_emul_70x130x4100", False, 70, 130, 4100, dtype="f32", epi=("emul", "acc"), beta=0.5)
for _cj in (False, True):
    _cn = "_conj" if _cj else ""
    case(f"batched_f32{_cn}", True, 37, 29, 40, dtype="f32", conj_b=_cj, entry="batched", api="batched", batch=3)
    case(f"batched_bf16{_cn}", True, 70, 130, 160, conj_b=_cj, entry="batched", api="batched", batch=3)

# ---- 8. the IEEE-half kernels (float32 out), without and with the operands' power-of-two scales -------------------------------
_SC = {None: "", (3, -2): "_scaled_3_m2", (-4, 4): "_scaled_m4_4", (4, 4): "_scaled_4_4"}
for _c in (True, False):
    _t = _CR[_c]
    for _i, _sc in enumerate(_SC):
        _K = (128, 192)[_i % 2]
        _h = dict(cplx=_c, dtype="f16", out="f32", scales=_sc)
        _tag = _SC[_sc]
        case(f"h_{_t}_full_k{_K}{_tag}", M=FULL[_c][0], N=FULL[_c][1], K=_K, flags=K1, **_h)
        case(f"h_{_t}_ragged_bias_k{_K}{_tag}", M=RAGGED[_c][0], N=RAGGED[_c][1], K=_K, epi="bias", conj_b=_c, flags=K1, **_h)
        case(f"h_{_t}_ragged_TT_bias_emul_acc_k{_K}{_tag}", M=RAGGED8[_c][0], N=RAGGED8[_c][1], K=_K, lay="TT", conj_b=_c, epi=_ALL,
             beta=0.5, flags=K1, **_h)
        case(f"h_{_t}_NT_acc_k{_K}{_tag}", M=RAGGED8[_c][0], N=RAGGED8[_c][1], K=_K, lay="NT", conj_b=_c, epi="acc", beta=-2.0, flags=K1,
             **_h)
        case(f"h_{_t}_w4_NN_bias_k{_K}{_tag}", M=W4[_c][0], N=W4[_c][1], K=_K, epi="bias", flags=K3, **_h)
        case(f"h_{_t}_w4_NT_emul_k{_K}{_tag}", M=W4[_c][0], N=W4[_c][1], K=_K, lay="NT", conj_b=_c, epi="emul", flags=K3, **_h)
        case(f"h_{_t}_w4_TT_bias_emul_acc_k{_K}{_tag}", M=W4[_c][0], N=W4[_c][1], K=_K, lay="TT", conj_b=_c, epi=_ALL, beta=None,
             flags=K3, **_h)
    case(f"h_{_t}_sliver", cplx=_c, M=1, N=8, K=128, dtype="f16", out="f32", epi="bias", flags=K1, scales=(2, 1))
case("h_r_TT_emul_exp_k128", False, 264, 264, 128, lay="TT", dtype="f16", out="f32", epi="emul_exp", flags=K1, scales=(1, 2))
case("h_r_w4_TT_emul_exp_k192", False, 512, 512, 192, lay="TT", dtype="f16", out="f32", epi="emul_exp", flags=K3)

# ---- 9. the split-product drivers of x3.py on integer float32 operands --------------------------------------------------------
# An integer in [-8, 8] IS its first piece (the others are zero), so the drivers' results are exact too.  This checks the
# piece views, the K-concatenation offsets, the stacking and the scale undo -- NOT the cross products of the low pieces,
# which are all zero here (tests/test_gpu_x3.py bounds those).
for _mode, _e in (("x3", ("cgemm", "rgemm")), ("x2", ("csc", "rsc"))):
    for _c in (True, False):
        _t = _CR[_c]
        _x = dict(cplx=_c, M=256, N=128, K=128, dtype="f32", api="x3", mode=_mode, entry=_e[0 if _c else 1])
        case(f"{_mode}_{_t}_gemm_nn_bias", epi="bias", **_x)
        case(f"{_mode}_{_t}_gemm_nt", lay="NT", conj_b=_c, **_x)
        case(f"{_mode}_{_t}_gemm_tt_emul_acc", lay="TT", conj_b=_c, epi=("emul", "acc"), beta=0.5, **_x)


# ---------------------------------------------------------------------------------------------------------------------------------
def tile_of(c):
    """(BM, BN) of the output tiles the case's kernel works on."""
    if c["kind"] == 0 or c["dtype"] == "f32" or c["api"] == "batched":
        bm = 64 if ((c["M"] + 127) // 128) * ((c["N"] + 127) // 128) <= 32 else 128
        return bm, bm
    return 256, (128 if c["cplx"] and "3m" not in c["epi"] else 256)


def split_plan(c):
    """(number of splits, K per split) of a split-K case of the bf16 families (kinds 4, 5; plan_splits of gemm_bf16_impl.h)."""
    bm, bn = tile_of(c)
    tiles = -(-c["M"] // bm) * -(-c["N"] // bn)
    s = min(256 // tiles, c["K"] // (32 * BK), 16)
    return s, -(-(c["K"] // BK) // s) * BK


def workgroup_of_tile(tiles_m, tiles_n, group_m=4):
    """{(tile row, tile column): virtual block} -- the XCD-contiguous grouped order every bf16 / half kernel walks its tiles in
    (gemm_bf16_impl.h, gemm_bf16_persist.h, gemm_bf16_w4.hip).  The persistent forms give workgroup j the blocks j, j + 256, ..."""
    ntiles = tiles_m * tiles_n
    q, r = ntiles >> 3, ntiles & 7
    out = {}
    for v in range(ntiles):
        xcd, idx = v & 7, v >> 3
        lin = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
        grp, in_grp = divmod(lin, group_m * tiles_n)
        first_m = grp * group_m
        gm = min(tiles_m - first_m, group_m)
        out[(first_m + in_grp % gm, in_grp // gm)] = v
    assert len(out) == ntiles
    return out


def plan_args(c, ncu=NCU):
    """Arguments of cplxamd_gemm_plan for a case: its `epi` knows the layers' three epilogues only -- 0 plain (a bias does not
    change the 8-wave kernels' dispatch), 1 the fused LRT term, 2 the float32 accumulate / multiplier."""
    epi = 1 if "lrt" in c["epi"] else 2 if c["epi"] & {"acc", "emul", "emul_exp"} else 0
    return (int(c["cplx"]), c["M"], c["N"], c["K"], int(c["ta"]), int(c["tb"]), DTYPE_CODE[c["out"]], epi, c["flags"], ncu)


def plan_checked(c):
    """Cases whose kernel cplxamd_gemm_plan can name: bf16 operands on the 4M entry points."""
    return c["dtype"] == "bf16" and c["api"] in ("ops", "cabi", "lrt") and "3m" not in c["epi"] and c["plan"] and not c["strides"]


def magnitude_bound(c):
    """|A op(B)^T| <= 2 K 64 (complex: two products per term), + 8 for the bias."""
    return 2 * c["K"] * 64 + 8


def macs(c):
    return (4 if c["cplx"] else 1) * c["batch"] * c["M"] * c["N"] * c["K"]


def _gen(c, device):
    g = torch.Generator(device=device)
    g.manual_seed((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7fffffff)
    return g


def make_inputs(c, device="cpu"):
    """float64 operands on `device`, integer-valued (biases half-integers), seeded by the case name: A [M, K], B [N, K]
    (logical, whatever the storage layout; a leading batch dimension for 'batched'), per plane 'r' / 'i' (real cases: 'r'
    only), and what the epilogue reads: bias [N], C0 [M, N] in [-64, 64], emul [M, N] = 2^j, lmul [M, N] (the
    log-multiplier of emul_exp: exact zeros where a seeded mask says so, eighths in [-2, 2] elsewhere), x and ga [M, N]
    (the LRT term: x in [-8, 8], ga in [-3, 3])."""
    g = _gen(c, device)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).double()  # noqa: E731
    M, N, K = c["M"], c["N"], c["K"]
    lead = (c["batch"],) if c["api"] == "batched" else ()
    d = {}
    for p in ("r", "i") if c["cplx"] else ("r",):
        d["a" + p], d["b" + p] = ints(-8, 8, *lead, M, K), ints(-8, 8, *lead, N, K)
        if "bias" in c["epi"]:
            d["bias" + p] = ints(-16, 16, N) / 2
        if "acc" in c["epi"]:
            d["c0" + p] = ints(-64, 64, M, N)
        if "lrt" in c["epi"]:
            d["x" + p] = ints(-8, 8, M, N)
    if "lrt" in c["epi"]:
        d["ga"] = ints(-3, 3, M, N)
    if "emul" in c["epi"]:
        d["emul"] = 2.0 ** ints(-3, 3, M, N)
    if "emul_exp" in c["epi"]:
        zero = ints(0, 1, M, N) == 0
        d["lmul"] = torch.where(zero, torch.zeros((), dtype=torch.float64, device=device), ints(-16, 16, M, N) / 8)
    return d


def products(c, d):
    """The exact float64 A op(B)^T per plane.  A complex product is written out as its four real ones; an integer-valued
    float64 product is exact in any order, so torch.matmul is an exact reference on every device."""
    mm = lambda a, b: torch.matmul(a, b.transpose(-1, -2))  # noqa: E731
    if not c["cplx"]:
        return {"r": mm(d["ar"], d["br"])}
    s = -1.0 if c["conj_b"] else 1.0
    return {"r": mm(d["ar"], d["br"]) - s * mm(d["ai"], d["bi"]), "i": s * mm(d["ar"], d["bi"]) + mm(d["ai"], d["br"])}


def reference(c, d):
    """-> {plane: float64 [M, N]}: C = ((A op(B)^T + bias) * emul) + beta * C_old.  With 'emul_exp' the multiplier is left
    out (it is not exact: exp_check); with 'lrt' this is the accumulator the documented arithmetic starts from
    (expected_lrt)."""
    ref = products(c, d)
    beta = 1.0 if c["beta"] is None else c["beta"]
    for p in ref:
        if "bias" in c["epi"]:
            ref[p] = ref[p] + d["bias" + p]
        if "emul" in c["epi"]:                      # (one real multiplier, on both planes of a complex result)
            ref[p] = ref[p] * d["emul"]
        if "acc" in c["epi"]:
            ref[p] = ref[p] + beta * d["c0" + p]
    return ref


def expected(ref, dtype):
    """What a kernel must return for the exact value `ref` (a float64 tensor), as float32: the value itself for a float32
    output, its ONE round-to-nearest-even for a bf16 output.  Refuses a value float32 cannot hold."""
    t = ref.to(torch.float32)
    if not bool((t.double() == ref).all()):
        raise ValueError("the reference is not exactly representable in float32")
    return t.bfloat16().float() if dtype == "bf16" else t


def expected_lrt(acc, x, ga):
    """The fused LRT input gradient, by the kernel's documented arithmetic (csrc/gemm.h: 'round(acc) to bf16 first, then
    fmaf(2 x, ga, that) rounded to bf16') -- TWO roundings, the same as the GEMM followed by cplxamd_lrt_dx_accum:
        bf16(float32(bf16(acc)) + 2 x ga).
    The inner sum is exact in float32 (a bf16 value below 2^24 plus an integer of at most 48), which `expected` asserts."""
    return expected(expected(acc, "bf16").double() + 2.0 * x * ga, "bf16")


def exp_check(got, base, lmul):
    """The emul_exp epilogue, C = base * expf(lmul) with base = A op(B)^T (+ bias): -> a bool tensor, True where `got` (float32)
    is WRONG.  Where lmul == 0 the result must equal base exactly (expf(0) == 1).  Elsewhere it must lie within EXP_ULPS
    float32 ulps of base * exp(lmul) formed in float64 -- one ulp for the product's rounding plus the library expf's error."""
    want = base * torch.exp(lmul)
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want).exponent - 24)        # |want| in [2^(e-1), 2^e): ulp 2^(e-24)
    close = torch.where(want == 0, got == 0, (got.double() - want).abs() <= EXP_ULPS * ulp)
    return ~torch.where(lmul == 0, got.double() == base, close)


def rounding_content(ref):
    """(fraction of values one bf16 rounding changes, number of exact ties among them) of a float64 tensor."""
    bits = ref.to(torch.float32).contiguous().view(torch.int32)
    low = bits & 0xffff
    return float((low != 0).double().mean()), int((low == 0x8000).sum())


# ---- mismatch reports that name the seam ----------------------------------------------------------------------------------------
def _seams(c, m, n):
    """Words for one mismatching coordinate (m, n) of the output."""
    M, N = c["M"], c["N"]
    bm, bn = tile_of(c)
    out = []
    if (M % bm and m == M - 1) or (N % bn and n == N - 1):
        out.append("last " + " and ".join(w for w, hit in (("row", M % bm and m == M - 1), ("column", N % bn and n == N - 1)) if hit)
                   + " of a ragged tile")
    if m % bm in (0, bm - 1) or n % bn in (0, bn - 1):
        out.append("tile border")
    tm, tn = m // bm, n // bn
    out.append(f"{bm} x {bn} tile {tm},{tn}")
    if c["kind"] in (2, 6):
        v = workgroup_of_tile(M // bm, N // bn)[(tm, tn)]
        out.append(f"workgroup {v % NCU}'s " + ("SECOND-round tile" if v >= NCU else "first tile"))
    return ", ".join(out)


def _missing_split(c, d, plane, m, n, diff):
    """Name the K split whose partial sum equals what a slab case's output lacks at (m, n), if one does."""
    if c["kind"] not in (4, 5) or c["epi"] & {"emul_exp"}:
        return ""
    s, chunk = split_plan(c)
    if "emul" in c["epi"]:
        diff = diff / float(d["emul"][m, n])
    row = {k: d["a" + k][m] for k in "ri" if "a" + k in d}
    col = {k: d["b" + k][n] for k in "ri" if "b" + k in d}
    sg = -1.0 if c["conj_b"] else 1.0
    if not c["cplx"]:
        terms = row["r"] * col["r"]
    elif plane == "r":
        terms = row["r"] * col["r"] - sg * row["i"] * col["i"]
    else:
        terms = sg * row["r"] * col["i"] + row["i"] * col["r"]
    parts = [float(terms[i * chunk:(i + 1) * chunk].sum()) for i in range(s)]
    hit = [i for i, p in enumerate(parts) if p == diff and p != 0]
    return f", lacks exactly split {hit[0]} of {s} (k in [{hit[0] * chunk}, {min(c['K'], (hit[0] + 1) * chunk)}))" if hit else ""


def describe_mismatch(bad, got, want, c, plane="r", d=None, limit=6):
    """'' if `bad` (a bool tensor [M, N], or [batch, M, N]) is False everywhere, else the count and the first few coordinates
    with the seam each lies on: last row / column of a ragged tile, border of the kernel's tile, the workgroup's second-round
    tile of the persistent forms, the K split of a slab case.  Only the mismatching coordinates leave the device."""
    count = int(bad.sum())
    if count == 0:
        return ""
    lines = [f"C{plane}: {count} of {bad.numel()} values differ (shape {tuple(bad.shape)})"]
    if c["kind"] in (4, 5):
        s, chunk = split_plan(c)
        lines[0] += f"; {s} K splits of {chunk} (last {c['K'] - (s - 1) * chunk})"
    for idx in bad.nonzero()[:limit].cpu().tolist():
        m, n = idx[-2:]
        g, w = float(got[tuple(idx)]), float(want[tuple(idx)])
        where = _seams(c, m, n)
        if d is not None and len(idx) == 2:
            try:
                where += _missing_split(c, d, plane, m, n, w - g)
            except Exception:       # noqa: BLE001  (the report must not hide the mismatch it reports)
                pass
        lines.append(f"  {tuple(idx)}: got {g!r}, want {w!r}  [{where}]")
    return "\n".join(lines)
