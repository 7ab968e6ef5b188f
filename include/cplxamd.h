/* cplxamd.h -- C ABI of libcplxamd.so: the MI355X (gfx950) kernels behind the
 * cplxmodule hot path (complex linear / conv / batch-norm forward+backward and the
 * variational-dropout local-reparameterization + KL path).
 *
 * Conventions
 *  - plain device pointers, sizes and element strides; no torch / C++ types.
 *  - complex tensors are two planar arrays (re, im): the reference's `Cplx` layout,
 *    /root/reference/cplxmodule/cplx.py:10-52.
 *  - every entry point is asynchronous on `stream` (a hipStream_t passed as void*),
 *    never allocates, never synchronises, and returns 0 on success, a hipError_t
 *    (> 0) for a failed launch, or a negative CPLXAMD_E* code for a bad argument.
 *  - scratch memory is supplied by the caller; sizes come from the *_ws_bytes() helpers.
 *
 * Each entry point cites the reference function (file:line under /root/reference) whose
 * arithmetic it replaces.
 */
#ifndef CPLXAMD_H
#define CPLXAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPLXAMD_ABI_VERSION 25

/* element types of activations / outputs */
enum { CPLXAMD_F32 = 0, CPLXAMD_BF16 = 1,
       CPLXAMD_F16 = 2 /* IEEE half: operand type of cplxamd_cgemm_sc_fl / cplxamd_rgemm_sc_fl only */,
       CPLXAMD_F64 = 3 /* float64: the Welch spectra (cplxamd_welch_*) and the initialiser kernels (cplxamd_init_*) only */ };

/* complex product algorithm of cplxamd_cgemm */
enum {
  CPLXAMD_ALGO_4M = 0,   /* four real products in one K loop     (cplx.py:634-648 linear_naive) */
  CPLXAMD_ALGO_3M = 1    /* Gauss: three real MFMA GEMMs + combine (cplx.py:651-672 linear_3m)   */
};

/* KL penalty kinds */
enum {
  CPLXAMD_KL_REAL_VD = 0,  /* cplxmodule/nn/relevance/real/vd.py:54-76     */
  CPLXAMD_KL_REAL_ARD = 1, /* cplxmodule/nn/relevance/real/ard.py:10-39    */
  CPLXAMD_KL_CPLX_VD = 2,  /* cplxmodule/nn/relevance/complex/vd.py:95-99  */
  CPLXAMD_KL_CPLX_ARD = 3, /* cplxmodule/nn/relevance/complex/ard.py:9-39  */
  /* SURVEY 8(f) row 4, cplxmodule/nn/relevance/extensions/complex.py: */
  CPLXAMD_KL_CPLX_VD_APPROX = 4,    /* :113-117 softplus-sigmoid approximation          */
  CPLXAMD_KL_CPLX_VD_SCALEFREE = 5, /* :43-46   log|w| - log_sigma2 - Ei(-1/alpha) / 2  */
  CPLXAMD_KL_CPLX_VD_BOGUS = 6,     /* :142-160 value -log_alpha (Ei dropped), exact slope  */
  /* ABI 25, cplxmodule/nn/relevance/extensions/real/: penalties of ONE parameter p, passed as both wr and log_sigma2;
   * only the gradient pointer named here is written (pass NULL for the other) */
  CPLXAMD_KL_REAL_L0 = 7,   /* ell_zero.py:73-88  sigmoid(beta log(zeta / -gamma) - log_alpha), p = log_alpha,
                                                   gradient -> g_log_sigma2                                  */
  CPLXAMD_KL_REAL_L1 = 8    /* lasso.py:7-9       |w| (torch.abs's gradient sign(w), 0 at 0), p = w, -> g_wr  */
};

/* error codes (negative; positive values are hipError_t) */
enum {
  CPLXAMD_OK = 0,
  CPLXAMD_EINVAL = -1,   /* bad enum / null pointer / negative size */
  CPLXAMD_EALIGN = -2,   /* pointer or leading dimension not aligned as required */
  CPLXAMD_ESHAPE = -3,   /* shape not supported by this entry point */
  CPLXAMD_EWS = -4       /* workspace too small */
};

/* Per-call launch policy (ABI 19): the `flags` argument of the `*_fl` entry points.  The library keeps NO mutable state
 * that a launch depends on (SURVEY 8(b) "Threading": re-entrant, no globals except read-only tuning tables): two threads /
 * streams / models in one process choose their launch forms independently, call by call.  GEMM results do not depend on
 * the flags (every form of a GEMM launch produces the same bits; tests/test_gpu_r04.py, test_gpu_gemm_persist.py,
 * test_gpu_r05.py), nor do the convolutions' forward / data-gradient results; the convolution WEIGHT gradients and the
 * conv -> batch-norm moments are sums of per-workgroup float32 partials whose number follows the flags (SHARED: twice as
 * many splits), so they agree across flags to float32 summation order, not bit for bit.
 *   CPLXAMD_LAUNCH_SHARED     other kernels hold compute units while this launch runs (an RCCL all-reduce overlapping the
 *                             backward pass): one workgroup per tile instead of the persistent forms, twice as many weight-
 *                             gradient splits -- a launch that expects every CU would wait for the held ones with its last
 *                             workgroups.
 *   CPLXAMD_LAUNCH_EXCLUSIVE  the chip is this launch's: persistent forms wherever they exist.
 *   neither                   the process default (cplxamd_gemm_set_persistent, deprecated; 1 = exclusive at start).
 *   CPLXAMD_LAUNCH_FAMILY(m)  bf16 GEMM kernel family mask of THIS launch (bit layout of cplxamd_gemm_set_family);
 *                             without it the process default applies (0xbf, env CPLXAMD_GEMM_W4).
 * Both SHARED and EXCLUSIVE, or unknown bits: CPLXAMD_EINVAL.  The flag-less entry points are the `*_fl` ones with
 * flags = 0. */
enum {
  CPLXAMD_LAUNCH_DEFAULT = 0,
  CPLXAMD_LAUNCH_SHARED = 1,
  CPLXAMD_LAUNCH_EXCLUSIVE = 2,
  CPLXAMD_LAUNCH_FAMILY_SET = 0x100,
  CPLXAMD_LAUNCH_FAMILY_SHIFT = 16
};
#define CPLXAMD_LAUNCH_FAMILY(mask) (CPLXAMD_LAUNCH_FAMILY_SET | (((mask) & 0xff) << CPLXAMD_LAUNCH_FAMILY_SHIFT))

int cplxamd_abi_version(void);

/* ------------------------------------------------------------------------------------
 * K6/K7  log-alpha, KL penalty (+ reduction, + gradients), relevance masks.
 * Replaces: GaussianMixin.log_alpha      nn/relevance/{complex/base.py:27-31, real/base.py:23-26}
 *           Cplx.__abs__                  cplx.py:183-192  (stack + norm)
 *           *.penalty                     (the four files listed at the KL kinds above)
 *           ExpiFunction fwd/bwd          nn/relevance/complex/vd.py:15-44 (scipy host round trip)
 *           named_penalties' .sum()       nn/relevance/base.py:135-139
 *           RelevanceMixin.relevance      nn/relevance/real/vd.py:16-19, complex/vd.py:50-53
 * `wi` is NULL for the real kinds.  All tensors float32, contiguous, n elements.
 * ---------------------------------------------------------------------------------- */

/* bytes of scratch the KL reductions need (independent of n) */
int64_t cplxamd_vd_kl_ws_bytes(void);

/* out_elem[n] (nullable) = penalty; out_sum[1] (nullable) = sum(penalty) (fp64 accumulate). */
int cplxamd_vd_kl_fwd(const float* wr, const float* wi, const float* log_sigma2, int kind,
                      float* out_elem, float* out_sum, void* ws, int64_t n, void* stream);

/* Gradient of  sum_j g_j * penalty_j  wrt (log_sigma2, wr, wi).  The upstream gradient is
 * either a tensor g_elem[n] or, when g_elem is NULL, the scalar *g_scalar read on the device
 * (no host sync).  Gradient outputs are nullable; they are overwritten, not accumulated. */
int cplxamd_vd_kl_bwd(const float* wr, const float* wi, const float* log_sigma2, int kind,
                      const float* g_elem, const float* g_scalar, float* g_log_sigma2,
                      float* g_wr, float* g_wi, int64_t n, void* stream);

/* One pass: out_sum = sum(penalty) AND the gradients of gscale * sum(penalty). */
int cplxamd_vd_kl_fwd_bwd(const float* wr, const float* wi, const float* log_sigma2, int kind,
                          float gscale, float* out_sum, float* g_log_sigma2, float* g_wr,
                          float* g_wi, void* ws, int64_t n, void* stream);

/* Per-step operand preparation of a bf16 VD / ARD layer fused with its KL term, ONE pass over
 * (wr, wi, log_sigma2): bf16 copies of the weight planes and of exp(log_sigma2) (the operands of the mean
 * and variance GEMMs; replaces two casts + torch.exp, complex/base.py:50-52) and, with_kl != 0,
 * out_sum = sum(penalty) plus its UNSCALED gradients (as cplxamd_vd_kl_fwd_bwd with gscale = 1).
 * Every output is nullable; wi NULL = real layer; n % 4 == 0 (else CPLXAMD_ESHAPE).
 * HBM: 12 B read + 6 B (bf16 operands) + 12 B (gradients) written per element. */
int cplxamd_vd_prep_kl(const float* wr, const float* wi, const float* log_sigma2, int kind, int with_kl,
                       void* wr_bf16, void* wi_bf16, void* s_bf16, float* out_sum, float* g_log_sigma2,
                       float* g_wr, float* g_wi, void* ws, int64_t n, void* stream);

/* out[n] = log_sigma2 - 2 log(|w| + 1e-12), evaluated so that it reproduces the reference's
 * float32 CPU result bit-for-bit wherever the libm log is correctly rounded. */
int cplxamd_vd_log_alpha(const float* wr, const float* wi, const float* log_sigma2, float* out,
                         int64_t n, void* stream);

/* g_w = g * d log_alpha / d w = -2 g w / (|w| (|w| + 1e-12)) (real: -2 g sign(w) / (|w| + 1e-12)), 0 at
 * w == 0; the gradient wrt log_sigma2 is g itself.  Backward of the differentiable `.log_alpha` property. */
int cplxamd_vd_log_alpha_bwd(const float* g, const float* wr, const float* wi, float* g_wr, float* g_wi,
                             int64_t n, void* stream);

/* mask[n] = (log_alpha <= threshold) ? 1.f : 0.f;  count[1] (nullable, int64) = #ones. */
int cplxamd_vd_mask(const float* wr, const float* wi, const float* log_sigma2, float threshold,
                    float* mask, int64_t* count, void* ws, int64_t n, void* stream);

/* torch_expi seam (nn/relevance/complex/vd.py:44): y = Ei(x), gx = g * exp(x) / x. */
int cplxamd_expi_fwd(const float* x, float* y, int64_t n, void* stream);
int cplxamd_expi_bwd(const float* g, const float* x, float* gx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * K5  local-reparameterization noise injection.
 * Replaces: CplxLinearGaussian.forward line 56   nn/relevance/complex/base.py:56
 *           LinearGaussian.forward line 49       nn/relevance/real/base.py:49
 *           cplx.randn / randn_like              cplx.py:544-562
 *   y = mu + eps * sqrt(max(s2, 1e-8))
 * mu_i / y_i / eps_i NULL  => real layer (eps ~ N(0,1)); else eps_r, eps_i ~ N(0,1/2).
 * eps_r NULL => noise from the counter-based Philox4x32-7 stream (seed, offset) defined in
 * DESIGN.md ("noise stream"); the backward regenerates it from the same (seed, offset).
 * `state` (nullable): device uint64[2] = {seed, offset}; when given it overrides the two host
 * scalars, so a hipGraph that captured the launch draws fresh noise on every replay
 * (cplxamd_philox_advance moves the stream position on the device).
 * s2 is float32; mu / y / eps / g have element type `dtype`; every pointer 16-byte aligned
 * (CPLXAMD_EALIGN otherwise).
 * ---------------------------------------------------------------------------------- */
int cplxamd_lrt_reparam_fwd(const void* mu_r, const void* mu_i, const float* s2,
                            const void* eps_r, const void* eps_i, uint64_t seed,
                            uint64_t offset, const uint64_t* state, void* y_r, void* y_i,
                            int64_t n, int dtype, void* stream);

/* g_s2 = (g_r*eps_r + g_i*eps_i) * 0.5 / sqrt(max(s2,1e-8)) * [s2 >= 1e-8]
 * g_s2 has element type gs2_dtype (float32, or bf16 when it feeds the bf16 GEMMs). */
int cplxamd_lrt_reparam_bwd(const void* g_r, const void* g_i, const float* s2,
                            const void* eps_r, const void* eps_i, uint64_t seed,
                            uint64_t offset, const uint64_t* state, void* g_s2, int64_t n,
                            int dtype, int gs2_dtype, void* stream);

/* The same two with the element type of s2 as an argument (`s2_dtype`: float32, or bf16 together with bf16
 * mu / g): the variance GEMM / convolution of a bf16 layer writes s2 in bf16, 2 bytes per output less in each
 * direction and no float32 [B, O] tensor kept for the backward. */
int cplxamd_lrt_reparam_fwd_ex(const void* mu_r, const void* mu_i, const void* s2,
                               const void* eps_r, const void* eps_i, uint64_t seed,
                               uint64_t offset, const uint64_t* state, void* y_r, void* y_i,
                               int64_t n, int dtype, int s2_dtype, void* stream);
int cplxamd_lrt_reparam_bwd_ex(const void* g_r, const void* g_i, const void* s2,
                               const void* eps_r, const void* eps_i, uint64_t seed,
                               uint64_t offset, const uint64_t* state, void* g_s2, int64_t n,
                               int dtype, int gs2_dtype, int s2_dtype, void* stream);

/* cplxamd_lrt_reparam_bwd_ex on a [rows][cols] matrix (a [B, O] gradient, or channels-last [B H W][C] planes) that
 * also returns the column sums of g_r / g_i -- the layer's bias gradient (dbr = sum_b G_r, cplx.py:646 under autograd)
 * -- without another pass over the gradient: sum_r / sum_i float32 [cols] (sum_i NULL for a real layer, g_i NULL).
 * Same noise as the flat entry point (the counter is the linear element index).  cols % 8 == 0 and cols / 8 a divisor
 * of 256 or cols a multiple of 2048, else CPLXAMD_ESHAPE (call the flat entry point + cplxamd_colsum).
 * ws: cplxamd_lrt_reparam_bwd_cols_ws_bytes(rows, cols) bytes, 16-byte aligned. */
int64_t cplxamd_lrt_reparam_bwd_cols_ws_bytes(int64_t rows, int cols);
int cplxamd_lrt_reparam_bwd_cols(const void* g_r, const void* g_i, const void* s2,
                                 const void* eps_r, const void* eps_i, uint64_t seed,
                                 uint64_t offset, const uint64_t* state, void* g_s2, int64_t rows,
                                 int cols, int dtype, int gs2_dtype, int s2_dtype, float* sum_r,
                                 float* sum_i, void* ws, int64_t ws_bytes, void* stream);

/* used[0..1] = state[0..1]; state[1] += 1  (device-resident noise stream position) */
int cplxamd_philox_advance(uint64_t* state, uint64_t* used, void* stream);

/* Writes the Philox noise itself (float32), for tests: real (eps_i NULL) or complex. */
int cplxamd_philox_normal(float* eps_r, float* eps_i, uint64_t seed, uint64_t offset,
                          int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * L0 hard-concrete gate (ABI 25; csrc/l0.hip).
 * Replaces: LinearL0.forward / gate / relevance / sparsity   nn/relevance/extensions/real/ell_zero.py:90-170
 *           LinearLASSO.relevance / sparsity                  nn/relevance/extensions/real/lasso.py:11-19
 *   train  z = clamp(1.2 sigmoid((log u - log(1 - u) - log_alpha) / 0.66) - 0.1, 0, 1)
 *   eval   z = clamp(1.2 sigmoid(-log_alpha) - 0.1, 0, 1)
 * Uniform stream (DESIGN.md "uniform stream"): element e (flat index of the [rows][cols] operand, = the flat index of
 * the reference's `u`) takes u01(Philox4x32-7(counter (e >> 2, offset), key seed)[e & 3]), u01(x) = ((x >> 8) + 0.5)
 * 2^-24.  `state` (nullable) is a device uint64[2] {seed, offset} read instead of the two arguments (graph capture),
 * as in cplxamd_lrt_reparam_fwd.  `u` (nullable, float32 [rows][cols]) supplies the uniforms instead (parity mode).
 * mode: CPLXAMD_L0_COLS -- log_alpha is [cols], one gate parameter per column (the input / output groups), else
 * [rows][cols] (group None); CPLXAMD_L0_TRAIN -- the stochastic gate, else the eval gate (u, seed, offset, state
 * ignored); CPLXAMD_L0_HARD (forward only) -- z > 0 ? 1 : 0.
 *   cplxamd_l0_gate_fwd   out = A (.) z (+ bias[c], COLS only), float32 arithmetic; a NULL: out = z (the relevance
 *                         mask).  a_dtype / out_dtype: CPLXAMD_F32 or CPLXAMD_BF16.  total (nullable, float64) = sum of
 *                         out, in a fixed order; ws: cplxamd_vd_kl_ws_bytes() bytes when total is given.
 *   cplxamd_l0_gate_bwd   the gate regenerated from the same (u | seed, offset, state): da = D (.) z and az = A (.) z
 *                         (both nullable), d_log_alpha = D (.) A (.) dz/dlog_alpha elementwise, or with COLS its sum
 *                         over the rows per column -- per-workgroup partials in ws (cplxamd_l0_gate_bwd_ws_bytes(rows,
 *                         cols) bytes) summed in a fixed order, no atomics: repeated calls give the same bits.  The
 *                         clamp passes the gradient where 0 <= pre-clamp value <= 1 (torch.clamp).  Pointers 16-byte
 *                         aligned.  Dtype combinations (d, a, da, az; an output passed as NULL takes the dtype of
 *                         its sibling, else of a): all float32; float32 d with bf16 a, da, az; bf16 d, da, az with
 *                         float32 a; all bf16.
 *   cplxamd_l1_mask       mask[n] (bool bytes, nullable) = log(|w| + 1e-20) >= threshold, correctly rounded log;
 *                         count (nullable, float64) = #ones; ws: cplxamd_vd_kl_ws_bytes() bytes when count is given.
 *   cplxamd_philox_uniform  u[n] = the uniform stream itself (tests).
 * HBM (group None, float32 W, bf16 operand): forward 10 B per weight, backward 20 B per weight.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_L0_COLS = 1, CPLXAMD_L0_TRAIN = 2, CPLXAMD_L0_HARD = 4 };
int cplxamd_l0_gate_fwd(const void* a, const float* log_alpha, const float* u, uint64_t seed, uint64_t offset,
                        const uint64_t* state, const float* bias, void* out, int64_t rows, int cols, int mode,
                        int a_dtype, int out_dtype, double* total, void* ws, void* stream);
int64_t cplxamd_l0_gate_bwd_ws_bytes(int64_t rows, int cols);
int cplxamd_l0_gate_bwd(const void* d, const void* a, const float* log_alpha, const float* u, uint64_t seed,
                        uint64_t offset, const uint64_t* state, void* da, void* az, float* d_log_alpha, int64_t rows,
                        int cols, int mode, int d_dtype, int a_dtype, int da_dtype, int az_dtype, void* ws,
                        int64_t ws_bytes, void* stream);
int cplxamd_l1_mask(const float* w, float threshold, uint8_t* mask, double* count, void* ws, int64_t n, void* stream);
int cplxamd_philox_uniform(float* u, uint64_t seed, uint64_t offset, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * K1/K4  complex and real GEMM,  C[m,n] = sum_k A[m,k] * op(B[n,k]) (+ bias[n]).
 * Replaces: cplx.linear_naive / linear_3m / linear_cat   cplx.py:634-694
 *           Cplx.__matmul__                               cplx.py:167-174
 *           the LRT variance GEMM                         nn/relevance/complex/base.py:50-54,
 *                                                         nn/relevance/real/base.py:48
 * and their autograd backward (dX = G conj(W), dW = G^T conj(X)).
 * A is addressed as A[m*a_rs + k*a_cs], B as B[n*b_rs + k*b_cs] (element strides), so one
 * entry point covers NT / NN / TN.  conj_b: use conj(B).  in_dtype: element type of A and B;
 * out_dtype: element type of C (row-major, leading dimension ldc).  bias is float32 [N].
 * accumulate != 0: C += result (C must then be float32).
 * The MFMA fast path (bf16 inputs, a_cs == b_cs == 1, K % 32 == 0, 16-byte aligned rows) is
 * chosen automatically; everything else runs the generic float32-MFMA kernel.
 * algo: CPLXAMD_ALGO_4M, or CPLXAMD_ALGO_3M = Gauss's three products t1 = Ar Br, t2 = Ai Bi,
 * t3 = (Ar + Ai)(Br + Bi): dense bf16 operands only (ESHAPE otherwise, never a silent 4M), needs
 * `ws` of cplxamd_cgemm3m_ws_bytes(M, N, K) bytes (256-B aligned), no accumulate.  The operand
 * sums are rounded to bf16, so the result is NOT bit-identical to 4M.
 * ---------------------------------------------------------------------------------- */
int cplxamd_cgemm(const void* a_r, const void* a_i, int64_t a_rs, int64_t a_cs,
                  const void* b_r, const void* b_i, int64_t b_rs, int64_t b_cs,
                  const float* bias_r, const float* bias_i, void* c_r, void* c_i, int64_t ldc,
                  int M, int N, int K, int conj_b, int in_dtype, int out_dtype, int accumulate,
                  int algo, void* ws, int64_t ws_bytes, void* stream);

/* Same, with (i) emul (nullable, float32 [M,N], leading dimension ldc, float32 C only): both planes of the
 * result are multiplied by it -- the weight gradient of a masked layer, dW * mask, nn/masked/complex.py:33-82;
 * (ii) a DEVICE-side scale on the accumulate operand: accumulate != 0 -> C = result + (*beta) * C
 * (beta NULL: 1).  Lets the weight-gradient GEMM of a VD / ARD layer finish `dW = dW_data + g_kl * dW_kl`
 * in its epilogue, g_kl being the upstream gradient of the KL term that autograd hands over as a device
 * scalar (replaces autograd's separate accumulation pass over every parameter gradient). */
int cplxamd_cgemm_ex(const void* a_r, const void* a_i, int64_t a_rs, int64_t a_cs,
                     const void* b_r, const void* b_i, int64_t b_rs, int64_t b_cs,
                     const float* bias_r, const float* bias_i, const float* emul, void* c_r, void* c_i,
                     int64_t ldc, int M, int N, int K, int conj_b, int in_dtype, int out_dtype, int accumulate,
                     const float* beta, int algo, void* ws, int64_t ws_bytes, void* stream);

/* cplxamd_cgemm_ex with a per-call launch policy (CPLXAMD_LAUNCH_*, top of this file). */
int cplxamd_cgemm_fl(const void* a_r, const void* a_i, int64_t a_rs, int64_t a_cs,
                     const void* b_r, const void* b_i, int64_t b_rs, int64_t b_cs,
                     const float* bias_r, const float* bias_i, const float* emul, void* c_r, void* c_i,
                     int64_t ldc, int M, int N, int K, int conj_b, int in_dtype, int out_dtype, int accumulate,
                     const float* beta, int algo, void* ws, int64_t ws_bytes, int flags, void* stream);

int64_t cplxamd_cgemm3m_ws_bytes(int M, int N, int K);

/* DEPRECATED (ABI 19: pass CPLXAMD_LAUNCH_SHARED / _EXCLUSIVE to the `*_fl` entry points instead; this setter only moves
 * the default that calls with neither flag read).  Process-wide switch of the persistent form of the bf16 GEMM kernels (returns the previous setting; 1 at start).
 * Persistent launches assume the whole chip: turn them off (0) while other kernels are expected to hold CUs -- e.g. an
 * RCCL all-reduce overlapping the backward pass -- and the GEMMs run one workgroup per tile, which shares CUs gracefully.
 * Results are bit-identical either way (tests/test_gpu_gemm_persist.py). */
int cplxamd_gemm_set_persistent(int on);

/* Process-wide choice of the bf16 GEMM kernel family per launch kind (returns the previous mask).  `mask` bits: which
 * launches go to the one-wave-per-SIMD kernels of round 4 (gemm_bf16_w4.hip: 4 waves, 128 x 64 complex wave tile in the
 * accumulator half of the 512-register file, operands staged through registers with both halves of every cache line
 * requested together) wherever those take the shape (full 256 x 128 complex / 256 x 256 real tiles, K % 64 == 0):
 *   bit 0 complex, bf16 out          bit 1 complex, bf16 out with the fused LRT input-gradient term     bit 2 complex, float32 out
 *   bit 3 real, bf16 out             bit 4 real, bf16 out with the fused term                           bit 5 real, float32 out
 *   bit 6 regardless of the K depth (without it: K >= 4096, or 1024 <= K < 4096 on (N,N) launches -- the family pays a
 *         prologue and an epilogue per output tile where the 8-wave kernels run persistent; profiles/r04_gemm_w4_ab.txt)
 *   bit 7 (round 5) the PERSISTENT form of the family -- one workgroup per CU, the K-tile ring running through the output-
 *         tile boundaries -- where it is built and measured faster: real bf16-out launches with the plain epilogue and no
 *         bias ((N,N); (N,T) from K = 4096), more tiles than CUs, and only for a launch that owns the chip
 *         (not CPLXAMD_LAUNCH_SHARED).  profiles/r05_gemm_w4_persistent.txt
 * 0 = the 8-wave LDS-DMA kernels of rounds 1-3 everywhere, -1 = every bit.  Start value 0xbf (env CPLXAMD_GEMM_W4=<mask>
 * overrides).  Both families produce the same bits (same
 * MFMA sequence per accumulator; tests/test_gpu_r04.py). */
int cplxamd_gemm_set_family(int mask);   /* DEPRECATED as a run-time switch: CPLXAMD_LAUNCH_FAMILY(mask) per call */

/* Optional scratch for split-K (few output tiles, long K -- e.g. the weight gradient at batch
 * 2^20, or a 10-output head): pass >= this many bytes as `ws` to cgemm / rgemm; ws may be NULL
 * (no split-K).  With split-K the float32 result is a sum of per-split partial sums. */
int64_t cplxamd_gemm_ws_bytes(int M, int N, int K, int cplx, int in_dtype, int out_dtype);

/* Input gradient of the complex LRT linear layer in ONE launch (nn/relevance/complex/base.py:43-56
 * differentiated):  dX = G conj(W) + 2 X (*) ga,  G [M, K] the output gradient, W [K, N] the bf16 weight as stored
 * ([O, I] row-major: w_rs = 1 over n ... pass the strides of W read as B[n, k], i.e. (1, I)), X [M, N] the layer
 * input and ga = d s2 . exp(log_sigma2) [M, N] (cplxamd_rgemm), all bf16, X / ga with row pitch ldx.  The elementwise
 * term rides in the epilogue of the persistent complex kernel (same arithmetic as cplxamd_cgemm followed by
 * cplxamd_lrt_dx_accum: bit-identical results), which saves the 7 plane passes of that second kernel.
 * Launches the persistent kernel does not take (partial tiles, fewer tiles than CUs, CPLXAMD_LAUNCH_SHARED = the
 * data-parallel form) carry the term in the one-tile kernel's staged epilogue, same bits.  CPLXAMD_ESHAPE when neither
 * epilogue applies (row pitches / N not multiples of 8 elements, unaligned operands): run the two calls instead --
 * nothing is dropped silently. */
int cplxamd_cgemm_lrt_dx(const void* g_r, const void* g_i, int64_t g_rs, int64_t g_cs,
                         const void* w_r, const void* w_i, int64_t w_rs, int64_t w_cs,
                         const void* x_r, const void* x_i, const void* ga, int64_t ldx,
                         void* dx_r, void* dx_i, int64_t ldc, int M, int N, int K, int dtype, void* stream);
/* The same for the REAL local-reparameterization layers (LinearVD / LinearARD, nn/relevance/real/base.py:43-49
 * differentiated): dX = G W + 2 X (*) ga in the epilogue of the persistent real kernel; bit-identical to cplxamd_rgemm
 * followed by cplxamd_lrt_dx_accum.  CPLXAMD_ESHAPE = run those two. */
int cplxamd_rgemm_lrt_dx(const void* g, int64_t g_rs, int64_t g_cs, const void* w, int64_t w_rs, int64_t w_cs,
                         const void* x, const void* ga, int64_t ldx, void* dx, int64_t ldc, int M, int N, int K, int dtype,
                         void* stream);

/* The two fused input gradients and cplxamd_rgemm_ex with a per-call launch policy (CPLXAMD_LAUNCH_*). */
int cplxamd_cgemm_lrt_dx_fl(const void* g_r, const void* g_i, int64_t g_rs, int64_t g_cs,
                            const void* w_r, const void* w_i, int64_t w_rs, int64_t w_cs,
                            const void* x_r, const void* x_i, const void* ga, int64_t ldx,
                            void* dx_r, void* dx_i, int64_t ldc, int M, int N, int K, int dtype, int flags, void* stream);
int cplxamd_rgemm_lrt_dx_fl(const void* g, int64_t g_rs, int64_t g_cs, const void* w, int64_t w_rs, int64_t w_cs,
                            const void* x, const void* ga, int64_t ldx, void* dx, int64_t ldc, int M, int N, int K,
                            int dtype, int flags, void* stream);
int cplxamd_rgemm_fl(const void* a, int64_t a_rs, int64_t a_cs, const void* b, int64_t b_rs,
                     int64_t b_cs, const float* bias, const float* emul, int emul_exp, void* c, int64_t ldc,
                     int M, int N, int K, int in_dtype, int out_dtype, int accumulate, const float* beta,
                     void* ws, int64_t ws_bytes, int flags, void* stream);
/* Which kernel a bf16 cplxamd_cgemm_fl / cplxamd_rgemm_fl call with these shapes, layouts ("N" = K-contiguous rows: ta /
 * tb = 0) and flags launches -- a pure function of its arguments and of `ncu`, the device's CU count (0: ask the current
 * device): 0 generic float32-exact kernel (the bf16 path declines), 1 8-wave one-tile, 2 8-wave persistent, 3
 * one-wave-per-SIMD (w4), 4 split-K slabs on the 8-wave kernels, 5 split-K slabs on w4, 6 w4 persistent.  `epi`: 0 plain / bias, 1 fused
 * LRT input-gradient term, 2 float32 accumulate / multiplier epilogue.  Dense operands, aligned pointers and a
 * workspace of cplxamd_gemm_ws_bytes are assumed.  (Dispatch made inspectable: the test of the per-call flags reads it.) */
int cplxamd_gemm_plan(int cplx, int M, int N, int K, int ta, int tb, int out_dtype, int epi, int flags, int ncu);

/* Batched complex GEMM (Cplx.__matmul__ on [..., M, K] @ [..., K, N], cplx.py:167-181): `batch`
 * independent products in ONE launch of the exact-f32 MFMA kernel (any strides, any dtype pair);
 * entry z reads A + z*a_bs, B + z*b_bs and writes C + z*c_bs (strides in elements).  batch <= 65535. */
int cplxamd_cgemm_batched(const void* a_r, const void* a_i, int64_t a_rs, int64_t a_cs, int64_t a_bs,
                          const void* b_r, const void* b_i, int64_t b_rs, int64_t b_cs, int64_t b_bs,
                          void* c_r, void* c_i, int64_t ldc, int64_t c_bs, int batch, int M, int N, int K,
                          int conj_b, int in_dtype, int out_dtype, void* stream);

/* real GEMM; emul (nullable, float32 [M,N] with leading dimension ldc): C = (A B^T) * emul. */
int cplxamd_rgemm(const void* a, int64_t a_rs, int64_t a_cs, const void* b, int64_t b_rs,
                  int64_t b_cs, const float* bias, const float* emul, void* c, int64_t ldc,
                  int M, int N, int K, int in_dtype, int out_dtype, int accumulate, void* ws,
                  int64_t ws_bytes, void* stream);

/* Same; emul_exp != 0: the multiplier is exp(emul[m,n]) (emul = log_sigma2: the LRT gradient
 * d log_sigma2 = (g_s2^T |x|^2) * exp(log_sigma2), nn/relevance/complex/base.py:52, without a
 * materialised exp); accumulate with the device-side scale *beta as in cplxamd_cgemm_ex. */
int cplxamd_rgemm_ex(const void* a, int64_t a_rs, int64_t a_cs, const void* b, int64_t b_rs,
                     int64_t b_cs, const float* bias, const float* emul, int emul_exp, void* c, int64_t ldc,
                     int M, int N, int K, int in_dtype, int out_dtype, int accumulate, const float* beta,
                     void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * elementwise / layout helpers used by the layers (all HBM-bound streaming kernels)
 *
 * cplxamd_abs2, _modulus, _cplx_abs_fwd, _cplx_abs_bwd, _mask_mul, _exp, _cast and (further down) _lrt_dx_accum move
 * 16 bytes per lane: every plane pointer, the mask included, must be 16-byte aligned, whatever the dtype.  A pointer
 * that is not returns CPLXAMD_EALIGN before anything is launched (after the CPLXAMD_EINVAL checks: NULL, n < 0, a
 * dtype other than F32 / BF16); n == 0 returns 0 without a launch.
 * ---------------------------------------------------------------------------------- */
/* out = xr^2 + xi^2 (xi NULL: xr^2)            nn/relevance/complex/base.py:51 */
int cplxamd_abs2(const void* xr, const void* xi, void* out, int64_t n, int in_dtype,
                 int out_dtype, void* stream);
/* out = |x| = sqrt(xr^2 + xi^2), float32, rounded exactly like torch's CPU 2-norm
 * (Cplx.__abs__, cplx.py:183-192) */
int cplxamd_modulus(const float* xr, const float* xi, float* out, int64_t n, void* stream);
/* abs(Cplx) for float32 / bf16 planes and its backward d x = g x / |x| with 0 at x == 0 (the
 * subgradient of the reference's stack + norm, cplx.py:183-192) */
int cplxamd_cplx_abs_fwd(const void* xr, const void* xi, void* out, int64_t n, int dtype, void* stream);
int cplxamd_cplx_abs_bwd(const void* g, const void* xr, const void* xi, void* dxr, void* dxi, int64_t n,
                         int dtype, void* stream);
/* out = in * mask (float32 mask) for one (in_i = out_i = NULL) or two planes, with the dtype
 * conversion of the bf16 path folded in: the sparsified weight of the masked layers
 * (nn/masked/real.py:25-71, complex.py:33-82) and, applied to gradients, its backward. */
int cplxamd_mask_mul(const void* in_r, const void* in_i, const float* mask, void* out_r, void* out_i,
                     int64_t n, int in_dtype, int out_dtype, void* stream);
/* out = exp(x), x float32                      nn/relevance/complex/base.py:52 */
int cplxamd_exp(const float* x, void* out, int64_t n, int out_dtype, void* stream);
/* dtype conversion */
int cplxamd_cast(const void* in, void* out, int64_t n, int in_dtype, int out_dtype, void* stream);

/* ---- float32-accurate products on the bf16 matrix pipe ("x3" operands; csrc/split.hip) -------------------------------
 * Replaces the float32 arithmetic of cplx.linear (cplxmodule/cplx.py:641-646) and of the local-reparameterization
 * variance products (nn/relevance/complex/base.py:43-56, real/base.py:43-49) at 2^-24-level accuracy without the 157-TFLOP/s
 * float32 MFMA: a float32 value is the exact sum of three bf16 values x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1),
 * and a product needs the six terms x0 w0, x0 w1, x1 w0, x0 w2, x2 w0, x1 w1 (the other three are below 2^-24 |x w|), each
 * exact in the bf16 MFMA with float32 accumulation.
 * cplxamd_split3 writes the pieces of  op(src)  [rows][cols] (row pitch ld_src; float32) as bf16 matrices
 *     dst + p * piece_stride + r * ld_dst + c,   p = 0 .. 2 (pattern A) or 0 .. 5 (pattern B)
 *   CPLXAMD_SPLIT_A   (x2, x1, x0)               -- the activation side; SUFFIXES of it are GEMM operands
 *   CPLXAMD_SPLIT_B   (w2, w1, w1, w0, w0, w0)   -- the weight side, replicated so that the six terms are three launches of
 *                     cplxamd_cgemm_fl / cplxamd_rgemm_fl (bf16 in, float32 out, accumulate from the second on) with
 *                     the pieces concatenated along K:   x0 . w2,   [x1|x0] . [w1|w1],   [x2|x1|x0] . [w0|w0|w0]
 *   (piece_stride = cols, ld_dst = 3 cols / 6 cols: pieces side by side in a row = K-concatenation of K-contiguous operands;
 *    piece_stride = rows * ld_dst: pieces stacked = K-concatenation of a K-major operand.)
 * op: CPLXAMD_SPLIT_ID  src;  CPLXAMD_SPLIT_ABS2  src^2 + src2^2 (src2 NULL: src^2; complex/base.py:51);
 *     CPLXAMD_SPLIT_EXP  exp(src) (log_sigma2 -> sigma^2, complex/base.py:52).  src2 only with ABS2.
 * A non-finite value is carried by the leading piece alone (the others 0).
 * cols % 8 == 0, ld_src % 4 == 0, ld_dst % 8 == 0, piece_stride % 8 == 0 (CPLXAMD_ESHAPE), 16-byte aligned pointers (CPLXAMD_EALIGN).
 * HBM: 4 (8 with src2) bytes read, 6 (pattern A) / 12 (pattern B) bytes written per element. */
enum { CPLXAMD_SPLIT_A = 0, CPLXAMD_SPLIT_B = 1 };
enum { CPLXAMD_SPLIT_ID = 0, CPLXAMD_SPLIT_ABS2 = 1, CPLXAMD_SPLIT_EXP = 2, CPLXAMD_SPLIT_MAX2 = 3 /* absmax only */ };
int cplxamd_split3(const float* src, const float* src2, int64_t ld_src, void* dst, int64_t ld_dst, int64_t piece_stride,
                   int64_t rows, int cols, int op, int pattern, void* stream);

/* ---- the same on IEEE-half pieces: three piece products instead of six ("x2" operands) -------------------------------
 * half has 11 significand bits: x s = h0 + h1 to 2^-22 with h0 = half(x s), h1 = half(x s - h0), and a product needs
 * h0 w0, h0 w1, h1 w0 (h1 w1 is below 2^-22 |x w|) -- half the matrix work of the bf16 split at 2^-22 instead of 2^-24.
 * The 5-bit exponent needs care: every operand is multiplied by a power of two s chosen from its largest magnitude
 * (cplxamd_absmax_scale: max |op(x)| s in [2^14, 2^15); s = 1 for an all-zero or non-finite tensor) before it is cut, and
 * the GEMM multiplies its accumulators by 1 / (sa sb) behind the K loop (exact).  An element keeps all 22 bits while
 * |x| >= 2^-17 max |x|; below that its second piece is subnormal and the element's error is <= 2^-39 max |x| absolute --
 * norm-wise the product is accurate to 2^-22 whatever the dynamic range.
 *   cplxamd_absmax_scale   scale[0] = s, scale[1] = 1 / s (device floats) for op(src) [rows][cols]; ws >= cplxamd_absmax_ws_bytes();
 *                          op as cplxamd_split3, or CPLXAMD_SPLIT_MAX2: max(|src|, |src2|) -- the two planes of a complex
 *                          operand must share one scale (the four real products of the complex GEMM mix them)
 *   cplxamd_split2h        pieces of op(src) * scale[0] as IEEE half, layouts as cplxamd_split3:
 *                          CPLXAMD_SPLIT_A (h1, h0)      CPLXAMD_SPLIT_B (w1, w0, w0)
 *                          launches:  h0 . w1,   [h1|h0] . [w0|w0]
 *   cplxamd_cgemm_sc_fl / cplxamd_rgemm_sc_fl   cplxamd_cgemm_fl / cplxamd_rgemm_fl for half operands (in_dtype = CPLXAMD_F16),
 *                          float32 C, with the two operands' scale buffers (both NULL: no scaling).  The MFMA kernel families
 *                          of the bf16 path compiled for v_mfma_f32_32x32x16_f16; shapes they decline: CPLXAMD_ESHAPE (there
 *                          is no generic fallback -- run the bf16 pieces). */
int64_t cplxamd_absmax_ws_bytes(void);
int cplxamd_absmax_scale(const float* src, const float* src2, int64_t ld_src, int64_t rows, int cols, int op, float* scale,
                         void* ws, void* stream);
int cplxamd_split2h(const float* src, const float* src2, int64_t ld_src, void* dst, int64_t ld_dst, int64_t piece_stride,
                    int64_t rows, int cols, int op, int pattern, const float* scale, void* stream);
int cplxamd_cgemm_sc_fl(const void* a_r, const void* a_i, int64_t a_rs, int64_t a_cs,
                        const void* b_r, const void* b_i, int64_t b_rs, int64_t b_cs,
                        const float* bias_r, const float* bias_i, const float* emul, void* c_r, void* c_i, int64_t ldc,
                        int M, int N, int K, int conj_b, int in_dtype, int accumulate, const float* beta,
                        const float* scale_a, const float* scale_b, void* ws, int64_t ws_bytes, int flags, void* stream);
int cplxamd_rgemm_sc_fl(const void* a, int64_t a_rs, int64_t a_cs, const void* b, int64_t b_rs, int64_t b_cs,
                        const float* bias, const float* emul, int emul_exp, void* c, int64_t ldc, int M, int N, int K,
                        int in_dtype, int accumulate, const float* beta, const float* scale_a, const float* scale_b,
                        void* ws, int64_t ws_bytes, int flags, void* stream);

/* The channels-last 3 x 3 convolutions on IEEE-half pieces (ABI 22; csrc/conv_cl2_f16.hip, conv_cl_wgrad_f16.hip: the bf16
 * kernels' sources compiled for the half matrix instruction): cplx.conv2d (cplxmodule/cplx.py:717-838) and its autograd in
 * float32-level accuracy for float32 layers -- the pieces are the [h1|h0] rows of cplxamd_split2h over the channels-last
 * planes read as [B H W][C] matrices, the weights' pieces are packed by cplxamd_conv2d_cl_pack (16-bit agnostic).
 *   cplxamd_conv2d_cl2h_fl   cplxamd_conv2d_cl2_fl with x: half planes [B][H][W][pitch] of which the C channels behind the
 *                            given pointers are convolved (pitch >= C: a channel window, e.g. the h0 half of [h1|h0]),
 *                            y: FLOAT32 [B][Ho][Wo][N], accumulate != 0: y += result, the result times 1 / (sa sb) from the
 *                            operands' scale buffers (both NULL: none), bias added once (pass it to the first launch).
 *                            forward y = h0 * w1 (+ b), then += [h1|h0] * [w0|w0]; the data gradient likewise (mode 1).
 *                            B H W pitch 2 < 0xF0000000 bytes per plane (CPLXAMD_ESHAPE: chunk the batch).
 *   cplxamd_conv2d_clh_wgrad(_fl / _ws_bytes)   cplxamd_conv2d_cl_wgrad on half planes: with G = [g1|g0] (2 Co channels) and
 *                            X = [x1|x0] (2 Ci) one launch gives the four piece blocks [2 Co][2 Ci][3][3]; the weight gradient is
 *                            (g0 x1) + (g1 x0) + (g0 x0) times 1 / (sg sx). */
int cplxamd_conv2d_cl2h_fl(const void* x_r, const void* x_i, int pitch, const void* w_packed, const float* bias_r,
                           const float* bias_i, float* y_r, float* y_i, int accumulate, const float* scale_a,
                           const float* scale_b, int64_t B, int H, int W, int C, int N, int pad_h, int pad_w, int mode, void* ws,
                           int64_t ws_bytes, int flags, void* stream);
/* ABI 24: the same with a contraction window that WRAPS around the pixel -- channel j of the contraction is channel
 * (c_start + j) mod pitch of the pixel (c_start, pitch multiples of 16; C + c_start <= 2 pitch).  Rows stored [h1 | h0]
 * (pitch = 2 c) read with c_start = c, C = 3 c give [h0 | h1 | h0]; against weights packed [w1 | w0 | w0] that is all three
 * piece products of a float32 convolution in ONE launch (one float32 epilogue instead of two, no accumulate pass). */
int cplxamd_conv2d_cl2h_wrap_fl(const void* x_r, const void* x_i, int pitch, int c_start, const void* w_packed,
                                const float* bias_r, const float* bias_i, float* y_r, float* y_i, int accumulate,
                                const float* scale_a, const float* scale_b, int64_t B, int H, int W, int C, int N, int pad_h,
                                int pad_w, int mode, void* ws, int64_t ws_bytes, int flags, void* stream);
int64_t cplxamd_conv2d_clh_wgrad_ws_bytes(int64_t B, int H, int W, int Ci, int Co);
int cplxamd_conv2d_clh_wgrad(const void* g_r, const void* g_i, const void* x_r, const void* x_i, const float* emul,
                             float* dw_r, float* dw_i, int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h,
                             int dil_w, int pad_h, int pad_w, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_conv2d_clh_wgrad_fl(const void* g_r, const void* g_i, const void* x_r, const void* x_i, const float* emul,
                                float* dw_r, float* dw_i, int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h,
                                int dil_w, int pad_h, int pad_w, void* ws, int64_t ws_bytes, int flags, void* stream);
/* ABI 24: the same without the block dW[0:skip_co, 0:skip_ci] (multiples of 64, both zero or both positive; those entries of
 * dw are left untouched): with G = [g1|g0], X = [x1|x0] and skip = (Co, Ci) the product g1 x1 -- 2^-22 of the result, not
 * one of the three piece products -- is not computed (3 of 4 tiles). */
int cplxamd_conv2d_clh_wgrad_skip_fl(const void* g_r, const void* g_i, const void* x_r, const void* x_i, float* dw_r, float* dw_i,
                                     int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h, int dil_w, int pad_h,
                                     int pad_w, int skip_co, int skip_ci, void* ws, int64_t ws_bytes, int flags, void* stream);
/* out[c, r] = in[r, c]  (rows x cols row-major in, ld = leading dims) */
int cplxamd_transpose(const void* in, int64_t ld_in, void* out, int64_t ld_out, int rows,
                      int cols, int dtype, void* stream);
/* out[n] = sum_m in[m, n]   (bias gradient; float32 out); ws (nullable -> slow path) holds
 * cplxamd_colsum_ws_bytes(cols) bytes of partial sums */
int64_t cplxamd_colsum_ws_bytes(int cols);
int cplxamd_colsum(const void* in, int64_t ld, float* out, int rows, int cols, int dtype,
                   void* ws, void* stream);
/* Column sums of both planes of a complex [rows, cols] tensor (a linear layer's complex bias gradient): one launch on
 * cplxamd_colsum's few-rows path, else two cplxamd_colsum passes.  ws as for cplxamd_colsum. */
int cplxamd_colsum2(const void* in_r, const void* in_i, int64_t ld, float* out_r, float* out_i, int rows, int cols,
                    int dtype, void* ws, void* stream);
/* dxr += 2 xr ga ; dxi += 2 xi ga   (LRT backward; xi/dxi NULL for real); planes 16-byte aligned
 * (CPLXAMD_EALIGN), as for the elementwise helpers above */
int cplxamd_lrt_dx_accum(void* dxr, void* dxi, const void* xr, const void* xi, const void* ga,
                         int64_t n, int dtype, int ga_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * K2  complex / real 2-d convolution (cross-correlation, NCHW, zero padding) as implicit GEMM.
 * Replaces: cplx.convnd / convnd_quick / convnd_naive / conv2d   cplx.py:717-838
 *           the LRT variance conv   nn/relevance/complex/base.py:125-133, real/base.py:152-162
 * and their autograd backward.  Planes of element type `dtype`; xi / wi / yi NULL => real conv.
 * geom = int[14] {B, Ci, Co, H, W, KH, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups};
 * weight [Co, Ci/groups, KH, KW]; bias float32 [Co] (nullable pair).
 *   fwd   : y = x (*) w (+ bias)            (no conjugation, cplx.py:719-726)
 *   dgrad : dx = g (*)^T conj(w)
 *   wgrad : dw = sum g conj(x)  (float32 out; emul nullable: dw_r *= emul, the LRT exp(ls2) factor)
 *           split-K partial slabs live in `ws` (>= cplxamd_conv2d_wgrad_ws_bytes).
 * ---------------------------------------------------------------------------------- */
int cplxamd_conv2d_out_shape(const int* geom, int* ho, int* wo);
int cplxamd_conv2d_fwd(const void* xr, const void* xi, const void* wr, const void* wi,
                       const float* bias_r, const float* bias_i, void* yr, void* yi,
                       const int* geom, int dtype, void* stream);
int cplxamd_conv2d_dgrad(const void* gr, const void* gi, const void* wr, const void* wi,
                         void* dxr, void* dxi, const int* geom, int dtype, void* stream);
int cplxamd_conv2d_wgrad_splits(const int* geom);
int64_t cplxamd_conv2d_wgrad_ws_bytes(const int* geom, int cplx);
int cplxamd_conv2d_wgrad(const void* gr, const void* gi, const void* xr, const void* xi,
                         const float* emul, float* dwr, float* dwi, const int* geom, int dtype,
                         void* ws, int64_t ws_bytes, void* stream);
/* cplxamd_conv2d_wgrad that also returns the bias gradient dbr / dbi [Co] (float32; complex: one [2][Co] array, dbi ==
 * dbr + Co; NULL = not wanted): the sum of G over batch and pixels rides as one more column of the weight-gradient GEMM
 * (its B entries are (1, 0)) and through the same slab sum -- no launches of its own -- unless that column would start a
 * tile of its own, in which case the library runs cplxamd_chansum2 / cplxamd_chansum.  Same workspace. */
int cplxamd_conv2d_wgrad_bias(const void* gr, const void* gi, const void* xr, const void* xi,
                              const float* emul, float* dwr, float* dwi, float* dbr, float* dbi, const int* geom,
                              int dtype, void* ws, int64_t ws_bytes, void* stream);
/* bf16 fast path of the same three operations (bf16 MFMA, register-gathered operand tiles).
 * ktab: device copy of the int[3*T] table written by cplxamd_conv2d_ktab_fill (a host-side
 * helper; mode 0 = fwd / wgrad table over (ci, kh, kw), 1 = dgrad table over (co, kh, kw)).
 * They return CPLXAMD_ESHAPE when the shape does not qualify (K % 32 != 0, strided dgrad):
 * the caller then uses the generic entry points above.  dgrad takes the weight repacked to
 * [groups][Ci/g][Co/g * KH * KW]. */
int cplxamd_conv2d_ktab_size(const int* geom, int mode);
int cplxamd_conv2d_ktab_fill(const int* geom, int mode, int* host_out);
int cplxamd_conv2d_bf16_fwd(const void* xr, const void* xi, const void* wr, const void* wi,
                            const float* bias_r, const float* bias_i, void* yr, void* yi,
                            const int* geom, const int* ktab, void* stream);
int cplxamd_conv2d_bf16_dgrad(const void* gr, const void* gi, const void* wtr, const void* wti,
                              void* dxr, void* dxi, const int* geom, const int* ktab,
                              void* stream);
/* The same data gradient with the float32 sums stored unrounded (dxr / dxi float32): for a caller that still adds to them
 * before the one rounding to bf16 (the transposed convolution's bias). */
int cplxamd_conv2d_bf16_dgrad_f32(const void* gr, const void* gi, const void* wtr, const void* wti,
                                  float* dxr, float* dxi, const int* geom, const int* ktab,
                                  void* stream);
int64_t cplxamd_conv2d_bf16_wgrad_ws_bytes(const int* geom, int cplx);
int cplxamd_conv2d_bf16_wgrad(const void* gr, const void* gi, const void* xr, const void* xi,
                              const float* emul, float* dwr, float* dwi, const int* geom,
                              const int* ktab, void* ws, int64_t ws_bytes, void* stream);

/* bf16 convolution, stride 1, groups 1, as ONE shifted-row MFMA GEMM over a zero-padded
 * channels-last copy of the input (conv_nhwc.hip): no gathers, operands move by LDS-DMA.
 *   cplxamd_nhwc_pad : planar NCHW bf16 x[B,C,H,W] -> out[B, Hp, Wp, C] (C % 8 == 0) with the image at
 *       rows pad_h.., columns pad_w.. and zeros elsewhere (Hp >= H + pad_h, Wp >= W + pad_w)
 *   cplxamd_conv2d_nhwc : with r(b, i, j) the flattened row index of grid position (i, j) of image b,
 *         y[b, co, ho, wo] = sum_{kh,kw,c} xp[r(b, ho + oh, wo + ow) + row_bias + kh*dil_h*Wp + kw*dil_w][c]
 *                                          * op(w[co, kh, kw, c]) (+ bias[co])      ho < Hout, wo < Wout
 *       xp_* channels-last bf16 grid [B, Hp, Wp, C], w_* bf16 [KH][KW][C/16][Cout][16] (C % 32 == 0,
 *       (KW-1)*dil_w <= 32), y_* planar NCHW [B, Cout, Hout, Wout] of out_dtype; xp_i == NULL: real
 *       convolution; conj_w: use conj(w).  row_bias <= 0; the buffer must hold -row_bias zero rows
 *       before the grid and 320 + (KH-1)*dil_h*Wp + (KW-1)*dil_w READABLE rows behind it (the bf16
 *       kernel does not clamp row indices; those rows only feed outputs that are not stored).
 * Forward (input padded by (ph, pw)): row_bias = oh = ow = 0, Hout = Hp-(KH-1)*dil_h,
 * w[kh][kw][c/16][co][c%16] = weight[co][c][kh][kw].  Data gradient: xp = the output gradient laid
 * top-left on the INPUT's padded grid (cplxamd_nhwc_pad(g, pad 0, Hp, Wp)), the roles of the two
 * channel dimensions swapped, the kernel flipped in both spatial dimensions, conj_w = 1,
 * row_bias = -((KH-1)*dil_h*Wp + (KW-1)*dil_w), (oh, ow) = (ph, pw), (Hout, Wout) = (H, W): the same
 * gradient grid then also feeds cplxamd_conv2d_nhwc_wgrad.
 * Replaces the same reference code as cplxamd_conv2d_fwd / _dgrad (cplx.py:717-838). */
int cplxamd_nhwc_pad(const void* x, void* out, int B, int C, int H, int W, int pad_h, int pad_w,
                     int Hp, int Wp, void* stream);
int cplxamd_conv2d_nhwc(const void* xp_r, const void* xp_i, const void* w_r, const void* w_i,
                        const float* bias_r, const float* bias_i, void* y_r, void* y_i, int B,
                        int Hp, int Wp, int C, int Cout, int KH, int KW, int dil_h, int dil_w,
                        int conj_w, int64_t row_bias, int oh, int ow, int Hout, int Wout,
                        int out_dtype, void* stream);

/* Exact-float32 versions of the two entry points above (conv_nhwc_f32.hip, v_mfma_f32_32x32x2_f32):
 * float32 grids / outputs, C % 16 == 0, weights packed [KH][KW][C/4][Cout][4]. */
int cplxamd_nhwc_pad_f32(const void* x, void* out, int B, int C, int H, int W, int pad_h, int pad_w,
                         int Hp, int Wp, void* stream);
int cplxamd_conv2d_nhwc_f32(const void* xp_r, const void* xp_i, const void* w_r, const void* w_i,
                            const float* bias_r, const float* bias_i, void* y_r, void* y_i, int B,
                            int Hp, int Wp, int C, int Cout, int KH, int KW, int dil_h, int dil_w,
                            int conj_w, int64_t row_bias, int oh, int ow, int Hout, int Wout,
                            void* stream);

/* Weight gradient on the same channels-last copies (conv_nhwc_wgrad.hip):
 *   dw[co, ci, kh, kw] = sum_r gp[r][co] * conj(xp[r + kh*dil_h*Wp + kw*dil_w][ci]) (* emul, real only)
 * over the rows r = (b, hp, wp) of the padded input grid.  gp_*: the output gradient laid on that
 * grid by cplxamd_nhwc_pad(g, .., pad_h = 0, pad_w = 0, Hp, Wp).  Both buffers carry ZERO tail rows
 * after the last image so that the kernel never clamps a row: gp up to a multiple of 32 rows, xp
 * 32 + (KH-1)*dil_h*Wp + (KW-1)*dil_w rows.  Ci % 8 == Co % 8 == 0, KW <= 4.  dw_* float32
 * [Co, Ci, KH, KW]; ws >= cplxamd_conv2d_nhwc_wgrad_ws_bytes. */
int64_t cplxamd_conv2d_nhwc_wgrad_ws_bytes(int B, int Hp, int Wp, int Ci, int Co, int KH, int KW,
                                           int cplx);
int cplxamd_conv2d_nhwc_wgrad(const void* gp_r, const void* gp_i, const void* xp_r, const void* xp_i,
                              const float* emul, float* dw_r, float* dw_i, int B, int Hp, int Wp,
                              int Ci, int Co, int KH, int KW, int dil_h, int dil_w, void* ws,
                              int64_t ws_bytes, void* stream);
/* exact-float32 version (float32 grids; Ci % 4 == Co % 4 == 0; gp tail up to a multiple of 16 rows) */
int64_t cplxamd_conv2d_nhwc_wgrad_f32_ws_bytes(int B, int Hp, int Wp, int Ci, int Co, int KH, int KW,
                                               int cplx);
int cplxamd_conv2d_nhwc_wgrad_f32(const void* gp_r, const void* gp_i, const void* xp_r, const void* xp_i,
                                  const float* emul, float* dw_r, float* dw_i, int B, int Hp, int Wp,
                                  int Ci, int Co, int KH, int KW, int dil_h, int dil_w, void* ws,
                                  int64_t ws_bytes, void* stream);
/* ---- complex convolution on UNPADDED channels-last planes (csrc/conv_cl.hip, conv_cl_wgrad.hip), bf16 in, fp32
 * accumulation: stride 1, groups 1, kernel width 3, zero padding 0 <= 2 pad <= dil (K - 1) per dimension (up to `same`).
 * Activations x: [B][H][W][C], y: [B][Ho][Wo][N] (Ho = H + 2 pad_h - dil_h (KH - 1), likewise Wo) -- the storage of
 * torch.channels_last tensors; no padded copies, no layout passes between layers that stay channels-last.
 * Replaces cplx.conv2d -> convnd and its autograd (cplxmodule/cplx.py:717-838) for these shapes; everything else:
 * CPLXAMD_ESHAPE, and the caller takes cplxamd_conv2d_nhwc / _bf16 / _fwd.
 *   cplxamd_conv2d_cl_pack: bf16 weight planes [Co][Ci][KH][KW] -> the kernel's per-stage LDS images (bytes:
 *       cplxamd_conv2d_cl_pack_bytes(N, C, KH, KW) with (N, C) = (Co, Ci) forward, (Ci, Co) data gradient); dgrad = 1
 *       folds the flip, the channel swap and the conjugate of the data gradient into the packing.
 *   cplxamd_conv2d_cl: mode 0 forward (C = Ci, N = Co, bias optional), mode 1 the data gradient OF that forward
 *       (x = output gradient [B][Ho][Wo][C = Co], y = input gradient [B][H][W][N = Ci]; H, W, pad_* still the forward's).
 *       Needs C % 16 == 0, N % 64 == 0, (KH * C / 16) % 6 == 0; ws >= cplxamd_conv2d_cl_ws_bytes(N).
 *   cplxamd_conv2d_cl_wgrad: dW[Co][Ci][3][3] (float32 planes, optionally times emul) from x [B][H][W][Ci] and
 *       g [B][Ho][Wo][Co]; needs KH = KW = 3, Ci % 64 == Co % 64 == 0 (any image width);
 *       ws >= cplxamd_conv2d_cl_wgrad_ws_bytes(B, H, W, Ci, Co).  Deterministic (fixed-order slab reduction).
 *   cplxamd_cl_to_nchw: channels-last [B][S][C] -> planar [B][C][S] (bf16; C % 8 == S % 8 == 0): the way back for a
 *       caller whose tensors are plain contiguous (the other direction is cplxamd_nhwc_pad with zero padding). */
int cplxamd_cl_to_nchw(const void* x_cl, void* out, int64_t B, int C, int64_t S, void* stream);
int64_t cplxamd_conv2d_cl_pack_bytes(int N, int C, int KH, int KW);
int64_t cplxamd_conv2d_cl_ws_bytes(int N);
int cplxamd_conv2d_cl_pack(const void* w_r, const void* w_i, void* out, int Co, int Ci, int KH, int KW, int dgrad,
                           void* stream);
int cplxamd_conv2d_cl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                      void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                      int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, void* stream);
/* cplxamd_conv2d_cl for dilation 1 in its 2-d-patch form (csrc/conv_cl2.hip: a 16 x 32 pixel tile stages the 18 x 34 input
 * patch once per 16-channel slice for all nine taps): same arguments, same packed weights, same results; needs KH = KW = 3,
 * dilation 1, C % 32 == 0 -- CPLXAMD_ESHAPE otherwise. */
int cplxamd_conv2d_cl2(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                       void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                       int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, void* stream);
/* Input gradient of the local-reparameterization convolutions (CplxConv2dVD / CplxConv2dARD: the layer of
 * cplxmodule/nn/relevance/complex.py:157-190, differentiated) in ONE launch:
 *     dx = dgrad(g; w) + 2 x (*) ga      per plane,
 * dgrad = cplxamd_conv2d_cl2 with mode 1 (w_packed from cplxamd_conv2d_cl_pack with dgrad = 1) and ga the variance
 * path's data gradient (cplxamd_conv2d_clr, mode 1).  g_r / g_i: [B][H + 2 pad - 2][W + 2 pad - 2][C] output gradients;
 * x_r / x_i / ga / dx_r / dx_i: [B][H][W][N], all bf16 channels-last.  Bit-identical to cplxamd_conv2d_cl2 followed by
 * cplxamd_lrt_dx_accum (the sum is formed on the bf16-rounded convolution result), minus one read-modify-write pass
 * over dx.  Shapes as cplxamd_conv2d_cl2 (CPLXAMD_ESHAPE otherwise: take the two launches). */
int cplxamd_conv2d_cl2_lrt_dx(const void* g_r, const void* g_i, const void* w_packed, const void* x_r, const void* x_i,
                              const void* ga, void* dx_r, void* dx_i, int64_t B, int H, int W, int C, int N, int pad_h,
                              int pad_w, void* ws, int64_t ws_bytes, void* stream);
/* The convolution in front of a batch-norm layer (the conv -> BN pair of the reference's networks:
 * cplxmodule/cplx.py:729-742 followed by nn/modules/batchnorm.py:62-123) with the layer's FORWARD STATISTICS formed in the
 * convolution's epilogue: cplxamd_conv2d_cl2 (forward, mode 0) that also writes, per workgroup, one row
 * [N][5] float64 of (sum re, sum im, sum re^2, sum im^2, sum re im) over the output pixels it produced -- of the bf16
 * values as stored -- into `partials`.  cplxamd_conv2d_cl2_mom_chunks: the number of rows (0: the variant does not take
 * the problem -- a shape cplxamd_conv2d_cl2 declines, a grid whose workgroups would change column tile, or
 * CPLXAMD_LAUNCH_SHARED -- use
 * cplxamd_conv2d_cl2 and the layer's own moment pass).  cplxamd_bn_fwd_partials then runs finalize + apply only: one
 * read of y less (csrc/conv_cl2.hip: conv_cl2_kernel<false, true>). */
int64_t cplxamd_conv2d_cl2_mom_chunks(int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w, int pad_h,
                                      int pad_w);
int cplxamd_conv2d_cl2_mom(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                           void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                           int pad_h, int pad_w, double* partials, int64_t partials_bytes, void* ws, int64_t ws_bytes,
                           void* stream);
int64_t cplxamd_conv2d_cl_wgrad_ws_bytes(int64_t B, int H, int W, int Ci, int Co);
int cplxamd_conv2d_cl_wgrad(const void* g_r, const void* g_i, const void* x_r, const void* x_i, const float* emul,
                            float* dw_r, float* dw_i, int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h,
                            int dil_w, int pad_h, int pad_w, void* ws, int64_t ws_bytes, void* stream);
/* The six launches above with a per-call launch policy (CPLXAMD_LAUNCH_SHARED: one workgroup per tile / twice the
 * weight-gradient splits; cplxamd_conv2d_cl2_mom declines under it -- CPLXAMD_ESHAPE, cplxamd_conv2d_cl2_mom_chunks_fl 0). */
int cplxamd_conv2d_cl_fl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                         void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                         int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, int flags, void* stream);
int cplxamd_conv2d_cl2_fl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r, const float* bias_i,
                          void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                          int pad_h, int pad_w, int mode, void* ws, int64_t ws_bytes, int flags, void* stream);
int cplxamd_conv2d_cl2_lrt_dx_fl(const void* g_r, const void* g_i, const void* w_packed, const void* x_r, const void* x_i,
                                 const void* ga, void* dx_r, void* dx_i, int64_t B, int H, int W, int C, int N, int pad_h,
                                 int pad_w, void* ws, int64_t ws_bytes, int flags, void* stream);
int64_t cplxamd_conv2d_cl2_mom_chunks_fl(int64_t B, int H, int W, int C, int N, int KH, int KW, int dil_h, int dil_w,
                                         int pad_h, int pad_w, int flags);
int cplxamd_conv2d_cl2_mom_fl(const void* x_r, const void* x_i, const void* w_packed, const float* bias_r,
                              const float* bias_i, void* y_r, void* y_i, int64_t B, int H, int W, int C, int N, int KH, int KW,
                              int dil_h, int dil_w, int pad_h, int pad_w, double* partials, int64_t partials_bytes, void* ws,
                              int64_t ws_bytes, int flags, void* stream);
int cplxamd_conv2d_cl_wgrad_fl(const void* g_r, const void* g_i, const void* x_r, const void* x_i, const float* emul,
                               float* dw_r, float* dw_i, int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h,
                               int dil_w, int pad_h, int pad_w, void* ws, int64_t ws_bytes, int flags, void* stream);
/* REAL-valued forms of the three entry points above (the CPLX = false kernels of csrc/conv_cl.hip and conv_cl_wgrad.hip): one plane each,
 * same shapes and conditions.  They carry the variance path of the local-reparameterization convolution layers
 * (conv of |x|^2 with exp(log_sigma2): nn/relevance/complex/base.py:120-135, real/base.py:116-163) and the real
 * Conv2dVD / ARD layers; cplxamd_conv2d_clr_wgrad can multiply the result by emul or exp(emul) ([Co][Ci][3][3] float32:
 * d log_sigma2 = (sum g |x|^2) * exp(log_sigma2)). */
int64_t cplxamd_conv2d_clr_pack_bytes(int N, int C, int KH, int KW);
int64_t cplxamd_conv2d_clr_ws_bytes(int N);
int cplxamd_conv2d_clr_pack(const void* w, void* out, int Co, int Ci, int KH, int KW, int dgrad, void* stream);
int cplxamd_conv2d_clr(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int H, int W, int C,
                       int N, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, int mode, void* ws,
                       int64_t ws_bytes, void* stream);
int64_t cplxamd_conv2d_clr_wgrad_ws_bytes(int64_t B, int H, int W, int Ci, int Co);
int cplxamd_conv2d_clr_wgrad(const void* g, const void* x, const float* emul, int emul_exp, float* dw, int64_t B, int H,
                             int W, int Ci, int Co, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, void* ws,
                             int64_t ws_bytes, void* stream);
int cplxamd_conv2d_clr_fl(const void* x, const void* w_packed, const float* bias, void* y, int64_t B, int H, int W, int C,
                          int N, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, int mode, void* ws,
                          int64_t ws_bytes, int flags, void* stream);
int cplxamd_conv2d_clr_wgrad_fl(const void* g, const void* x, const float* emul, int emul_exp, float* dw, int64_t B, int H,
                                int W, int Ci, int Co, int KH, int KW, int dil_h, int dil_w, int pad_h, int pad_w, void* ws,
                                int64_t ws_bytes, int flags, void* stream);
/* ------------------------------------------------------------------------------------
 * K3: complex 3-d convolution as implicit GEMM on the float32 matrix instruction (csrc/conv3d.hip; still ABI 25: exports
 * added).  The kernel behind cplx.conv_transpose3d / nn.CplxConvTranspose3d, whose forward pass is the data gradient.
 * Replaces: cplx.conv_transposend / conv_transposend_naive / conv_transpose3d   cplx.py:860-1029
 * Planar [B, C, D, H, W] operands of element type `dtype` (CPLXAMD_F32 or CPLXAMD_BF16; converted to float32 on load,
 * float32 sums, one rounding on store).  Complex only: a NULL imaginary plane is CPLXAMD_EINVAL.
 * geom = int[19] {B, Ci, Co, D, H, W, KD, KH, KW, stride_d, stride_h, stride_w, pad_d, pad_h, pad_w, dil_d, dil_h, dil_w,
 * groups} describes the forward correlation; weight [Co, Ci/groups, KD, KH, KW].
 *   fwd   : y = x (*) w                         (no conjugation, no bias)
 *   dgrad : dx = g (*)^T conj(w) (+ bias)       bias: float32 [Ci] pair (both or neither), added to the float32 sums
 *           before their one rounding.  Strides of 1 or 2 per dimension (at least one 2) run by stride phases: up to 8
 *           classes of voxels, each a GEMM over its valid taps only; every voxel of dx is written, also those of a
 *           class without a valid tap (bias, or zero).  flags: 0, or CPLXAMD_CONV3D_PLAIN = the plain path (every tap
 *           tested per voxel) at any stride -- the same sums; for measuring what the phases save.  Other bits: EINVAL.
 *   wgrad : dw = sum g conj(x)   (float32 out); split-K partial slabs live in `ws` (>= cplxamd_conv3d_wgrad_ws_bytes,
 *           which returns -1 for an invalid geometry) and are summed in a fixed order: no atomics, the same bits on
 *           every run.  The bias gradient is cplxamd_chansum2 on the output gradient (S = D * H * W).
 * Voxel and tap indices are 32-bit: a GEMM dimension or voxel count above 0x7fe00000, or a launch grid above 65535 in
 * y / z, is CPLXAMD_ESHAPE, as is an empty output or channels that the groups do not divide; a non-positive stride,
 * dilation or groups is CPLXAMD_EINVAL.  All checks precede any launch.  No host synchronisation, no allocation; an empty
 * batch returns 0 without a launch (wgrad: zero-fills dw).
 * ---------------------------------------------------------------------------------- */
#define CPLXAMD_CONV3D_PLAIN 1
int cplxamd_conv3d_out_shape(const int* geom, int* dout, int* ho, int* wo);
int cplxamd_conv3d_fwd(const void* xr, const void* xi, const void* wr, const void* wi, void* yr, void* yi,
                       const int* geom, int dtype, void* stream);
int cplxamd_conv3d_dgrad(const void* gr, const void* gi, const void* wr, const void* wi, const float* bias_r,
                         const float* bias_i, void* dxr, void* dxi, const int* geom, int dtype, int flags, void* stream);
int64_t cplxamd_conv3d_wgrad_ws_bytes(const int* geom);
int cplxamd_conv3d_wgrad(const void* gr, const void* gi, const void* xr, const void* xi, float* dwr, float* dwi,
                         const int* geom, int dtype, void* ws, int64_t ws_bytes, void* stream);

/* out[c] = sum over (batch, spatial) of an NCHW tensor (conv bias gradient); ws >= 64*C*8 bytes */
int cplxamd_chansum(const void* x, float* out, int64_t B, int C, int64_t S, int dtype, void* ws,
                    void* stream);
/* The complex bias gradient: out_r[c], out_i[c] (one [2][C] array: out_i == out_r + C) = the same sums of the two
 * planes, both planes per launch (2 launches instead of 4: small models are bound by the NUMBER of dependent
 * launches).  ws >= 2*64*C*8 bytes. */
int cplxamd_chansum2(const void* x_r, const void* x_i, float* out_r, float* out_i, int64_t B, int C, int64_t S, int dtype,
                     void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * K3  complex batch normalisation (2x2 whitening + 2x2 affine), forward and backward.
 * Replaces: whiten2x2        nn/modules/batchnorm.py:62-123
 *           cplx_batch_norm  nn/modules/batchnorm.py:189-278 (and its autograd backward)
 * Tensors: planar x / y / g [B, F, S] contiguous (S = product of spatial dims, 1 for [B,F]);
 * weight [2,2,F], bias [2,F], running_mean [2,F], running_var [2,2,F] float32 (nullable pairs);
 * saved [8,F] float32 = per-feature (mean_u, mean_v, p, q, w, Vuu, Vuv, Vvv) handed from the
 * forward to the backward.  training != 0: batch statistics (biased covariance, eps on the
 * diagonal) and in-place running-stat update x += momentum (new - x); else running stats.
 * ---------------------------------------------------------------------------------- */
int64_t cplxamd_bn_ws_bytes(int F);
int cplxamd_bn_fwd(const void* xr, const void* xi, void* yr, void* yi, int64_t B, int F,
                   int64_t S, const float* weight, const float* bias, float* running_mean,
                   float* running_var, float* saved, int training, int dtype, float momentum,
                   float eps, void* ws, int64_t ws_bytes, void* stream);
/* cplxamd_bn_fwd that also adds 1 to *tracked_inc (the module's int64 num_batches_tracked; may be NULL) in its finalize
 * launch: one launch less per layer and step than an elementwise add of its own. */
int cplxamd_bn_fwd_ex(const void* xr, const void* xi, void* yr, void* yi, int64_t B, int F,
                      int64_t S, const float* weight, const float* bias, float* running_mean,
                      float* running_var, float* saved, int training, int dtype, float momentum,
                      float eps, int64_t* tracked_inc, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_bn_bwd(const void* gr, const void* gi, const void* xr, const void* xi, void* dxr,
                   void* dxi, int64_t B, int F, int64_t S, const float* weight,
                   const float* saved, float* dweight, float* dbias, int training, int dtype,
                   void* ws, int64_t ws_bytes, void* stream);
/* The same, plus (dx_sums != NULL) the per-feature sums over all rows of the two dX planes as stored, float32 [2][F] --
 * the bias gradient of a convolution / linear layer whose output this batch-norm normalised, for free: the apply pass
 * already holds every dX value.  Only on the row-kernel path (cplxamd_bn_rows_path(B, F, S) == 1: S == 1, F % 8 == 0,
 * F <= 1024, B >= 4096), else CPLXAMD_ESHAPE. */
int cplxamd_bn_rows_path(int64_t B, int F, int64_t S);
int cplxamd_bn_bwd_sums(const void* gr, const void* gi, const void* xr, const void* xi, void* dxr,
                        void* dxi, int64_t B, int F, int64_t S, const float* weight,
                        const float* saved, float* dweight, float* dbias, int training, int dtype,
                        float* dx_sums, void* ws, int64_t ws_bytes, void* stream);

/* ABI 24: cplxamd_bn_bwd_sums that also leaves per-block maxima of |dX| (both planes, as stored) in amax_partial[2048]
 * (float32, ZEROED by the caller; row-kernel path only): cplxamd_absmax_scale_partials(amax_partial, 2048, scale) then gives
 * the {s, 1 / s} that cplxamd_absmax_scale would have computed from dX -- the consumer that cuts dX into half pieces (a
 * float32 convolution's backward on 'x2' pieces) reads the planes once less. */
int cplxamd_bn_bwd_sums_amax(const void* gr, const void* gi, const void* xr, const void* xi, void* dxr, void* dxi, int64_t B,
                             int F, int64_t S, const float* weight, const float* saved, float* dweight, float* dbias,
                             int training, int dtype, float* dx_sums, float* amax_partial, void* ws, int64_t ws_bytes,
                             void* stream);
int cplxamd_absmax_scale_partials(const float* partial, int n, float* scale, void* stream);

/* ABI 24: the backward of a batch-norm layer that directly follows a channels-last 3 x 3 convolution, WITHOUT its apply
 * pass (nn/modules/batchnorm.py:189-278 under autograd followed by the autograd of cplx.py:717-838).  The layer's input
 * gradient is dX = E g + C (x - mu) - k with per-channel 2 x 2 real matrices E, C and constants k:
 *   cplxamd_bn_bwd_coef            sums + finalize of cplxamd_bn_bwd (dweight, dbias as there) and coef[F][12] float32 =
 *                                  (mu mv | e00 e01 e10 e11 | cuu cuv cvv | ku kv | pad); no dX is written.  dx_sums (may be
 *                                  NULL): float32 [2][F], the per-feature sums of dX over all rows -- the bias gradient of the
 *                                  layer that produced x -- from the sums this pass has anyway: E sum(g) - count k (the C term
 *                                  sums to zero against the batch mean and C = 0 in evaluation mode; in training mode the
 *                                  whole expression is zero up to rounding, which is what the reference's float32 sum of dX
 *                                  gives too);
 *   cplxamd_conv2d_cl_wgrad_bn_fl  the convolution's weight gradient, which forms dX tile by tile on the way into its
 *                                  LDS stages (bn_apply's arithmetic with the means multiplied out: the same bf16 values
 *                                  up to one rounding step in a few elements), multiplies it against x, and also stores it
 *                                  (dy_r / dy_i: the data gradient reads it next).  g, z (= the batch-norm layer's input =
 *                                  the convolution's output), dy: [B][Ho][Wo][Co] bf16 channels-last planes; x:
 *                                  [B][H][W][Ci]; shapes and ws as cplxamd_conv2d_cl_wgrad.
 * Against cplxamd_bn_bwd_sums + cplxamd_conv2d_cl_wgrad_fl: one pass over 6 planes less (4 read, 2 written). */
int cplxamd_bn_bwd_coef(const void* gr, const void* gi, const void* xr, const void* xi, int64_t B, int F, int64_t S,
                        const float* weight, const float* saved, float* dweight, float* dbias, int training, int dtype,
                        float* coef, float* dx_sums, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_conv2d_cl_wgrad_bn_fl(const void* g_r, const void* g_i, const void* z_r, const void* z_i, const float* coef,
                                  const void* x_r, const void* x_i, void* dy_r, void* dy_i, float* dw_r, float* dw_i,
                                  int64_t B, int H, int W, int Ci, int Co, int KH, int KW, int dil_h, int dil_w, int pad_h,
                                  int pad_w, void* ws, int64_t ws_bytes, int flags, void* stream);

/* Batch statistics shared between data-parallel ranks ("optional SyncBN"; the reference normalises
 * with the statistics of the local batch only, nn/modules/batchnorm.py:70-99).  A pass is split around ONE
 * all-reduce issued by the caller:
 *   cplxamd_bn_moments  -> this rank's totals, double [F][5] = sum u, v, u^2, v^2, u v (gr == gi == NULL) or
 *                          double [F][6] = the backward sums of g and g x (x - mean) (gr, gi, saved given);
 *   [caller: all-reduce(SUM) of the totals and of the position count B * S, both staying on the device]
 *   cplxamd_bn_fwd_sync / cplxamd_bn_bwd_sync -> finalize + apply from the summed totals (`moments`) and `count`
 *                          (device pointer to ONE double).  Backward: dweight / dbias are this rank's sums (from
 *                          `local_moments`, the array cplxamd_bn_moments wrote before the all-reduce) -- the gradient
 *                          exchange averages them like every other parameter gradient -- while dX uses the totals.
 * Always training-mode statistics; everything else as cplxamd_bn_fwd / cplxamd_bn_bwd_sums. */
int cplxamd_bn_moments(const void* xr, const void* xi, const void* gr, const void* gi, const float* saved,
                       int64_t B, int F, int64_t S, int dtype, double* moments, void* ws, int64_t ws_bytes,
                       void* stream);
int cplxamd_bn_fwd_sync(const void* xr, const void* xi, void* yr, void* yi, int64_t B, int F, int64_t S,
                        const float* weight, const float* bias, float* running_mean, float* running_var,
                        float* saved, int dtype, float momentum, float eps, const double* moments,
                        const double* count, void* ws, int64_t ws_bytes, void* stream);
/* Training-mode forward with the statistics pass done by the producer of x: `partials` = `chunks` rows [row][F][5]
 * float64 of (sum re, sum im, sum re^2, sum im^2, sum re im) over disjoint parts of the batch (what
 * cplxamd_conv2d_cl2_mom writes).  Finalize + apply; otherwise as cplxamd_bn_fwd_ex with training = 1. */
int cplxamd_bn_fwd_partials(const void* xr, const void* xi, void* yr, void* yi, int64_t B, int F, int64_t S,
                            const float* weight, const float* bias, float* running_mean, float* running_var,
                            float* saved, int dtype, float momentum, float eps, int64_t* tracked_inc,
                            const double* partials, int chunks, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_bn_bwd_sync(const void* gr, const void* gi, const void* xr, const void* xi, void* dxr, void* dxi,
                        int64_t B, int F, int64_t S, const float* weight, const float* saved, float* dweight,
                        float* dbias, int dtype, float* dx_sums, const double* moments, const double* local_moments,
                        const double* count, void* ws, int64_t ws_bytes, void* stream);

/* Elementwise complex product (div == 0) or quotient (div != 0) of two planar complex tensors in one launch
 * (Cplx.__mul__ / __truediv__, cplxmodule/cplx.py:135-165: 6 / 12 elementwise torch kernels), with the reference's
 * operation order -- no fused multiply-add -- so float32 values are bit-identical.  conj_b: b is conjugated first;
 * neg: the result is negated (together they give the gradients: d(ab)/da = g conj(b), d(a/b)/da = g / conj(b),
 * d(a/b)/db = -(g conj(a/b)) / conj(b)).  16-byte aligned planes of n elements. */
int cplxamd_cplx_mul(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* o_r, void* o_i, int64_t n,
                     int div, int conj_b, int neg, int dtype, void* stream);
/* ReLU applied to the real and the imaginary plane (CplxToCplx[torch.nn.ReLU], nn/modules/base.py:167-199) in one launch.
 * bwd == 0: o = relu(a) (NaN passes, as torch).  bwd != 0: a = the saved OUTPUTS, o = (a <= 0 ? 0 : g)
 * (= aten::threshold_backward on the result).  16-byte aligned planes of n elements. */
int cplxamd_split_relu(const void* a_r, const void* a_i, const void* g_r, const void* g_i, void* o_r, void* o_i, int64_t n,
                       int bwd, int dtype, void* stream);
/* ------------------------------------------------------------------------------------
 * layout converters and the non-GEMM layers either side of the path.
 *   cplxamd_deinterleave / _interleave : x[2n] <-> (re[n], im[n])   cplx.py:451-470
 *       (from_interleaved_real(copy=True) / to_interleaved_real along the last dim)
 *   cplxamd_modrelu_fwd / _bwd : y = z * relu(1 - tau / max(|z|, 1e-5))   cplx.py:565-616
 *       tau: tau_numel == 0 -> the value `tau_value`; 1 -> read from the device pointer (a
 *       learnable scalar, no host sync); n -> one threshold per element (pre-broadcast).
 *       bwd writes dz and, if dtau != NULL, the elementwise d/dtau (float32 [n]; the caller
 *       sums it down to the parameter's shape).
 *   cplxamd_cplx_dropout : y = x * keep / (1 - p), ONE Bernoulli(1 - p) draw per complex element
 *       (nn/modules/extra.py:7-25); keep comes from the Philox4x32-7 stream (seed, offset) or
 *       the device pair `state`; applying it to the gradient is the backward.
 * All planes contiguous, 16-byte aligned, n = number of complex elements.
 * ---------------------------------------------------------------------------------- */
int cplxamd_deinterleave(const void* x, void* re, void* im, int64_t n, int dtype, void* stream);
int cplxamd_interleave(const void* re, const void* im, void* out, int64_t n, int dtype, void* stream);
int cplxamd_modrelu_fwd(const void* zr, const void* zi, const float* tau, float tau_value, int tau_numel,
                        void* yr, void* yi, int64_t n, int dtype, void* stream);
int cplxamd_modrelu_bwd(const void* zr, const void* zi, const float* tau, float tau_value, int tau_numel,
                        const void* gr, const void* gi, void* dzr, void* dzi, float* dtau, int64_t n,
                        int dtype, void* stream);
int cplxamd_cplx_dropout(const void* xr, const void* xi, void* yr, void* yi, double p, uint64_t seed,
                         uint64_t offset, const uint64_t* state, int64_t n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Complex elementary functions (cplx.exp / log / sin / cos / tan / sinh / cosh / tanh, cplxmodule/cplx.py:482-541; csrc/
 * cplxfn.hip), one launch each way.  Added after ABI 25 was published: these are new exports only, nothing existing
 * changes, so the version stays 25 and every consumer of ABI 25 keeps working.
 *   cplxamd_cplx_fn_fwd  y = f(z)
 *   cplxamd_cplx_fn_bwd  dz = conj(f'(z)) g   (the gradient of the real pair (re, im), as autograd defines it), f'
 *                        recomputed from the saved input z
 * float32 arithmetic for F32 and BF16 (BF16 rounded once on store).  tan and tanh stay finite wherever the true value is
 * (Kahan's form, saturated past |Re| = 11 for tanh, |Im| = 11 for tan), where the reference's sin / cos and sinh / cosh
 * quotients give NaN; exp, sin, cos, sinh and cosh may give inf where one of the reference's real factors overflows.
 * n complex elements in planes sharing one dense layout, 16-byte aligned.  Checked before any launch: a NULL pointer with
 * n > 0, n < 0, an unknown fn or a dtype other than F32 / BF16 -> CPLXAMD_EINVAL; n == 0 -> 0.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_FN_EXP = 0, CPLXAMD_FN_LOG, CPLXAMD_FN_SIN, CPLXAMD_FN_COS,
       CPLXAMD_FN_TAN, CPLXAMD_FN_SINH, CPLXAMD_FN_COSH, CPLXAMD_FN_TANH };
int cplxamd_cplx_fn_fwd(const void* z_r, const void* z_i, void* y_r, void* y_i,
                        int64_t n, int fn, int dtype, void* stream);
int cplxamd_cplx_fn_bwd(const void* z_r, const void* z_i, const void* g_r, const void* g_i,
                        void* dz_r, void* dz_i, int64_t n, int fn, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Welch power spectra (cplxmodule/utils/spectrum.py:7-82 pwelch; csrc/spectrum.hip).  New exports under ABI 25, as the
 * cplxamd_cplx_fn_* block: nothing existing changes.
 *   x: `rows` signals of `t` complex samples, sample i of row r at x_r / x_i [r * x_row_stride + i * x_stride] (element
 *      strides: interleaved complex passes x_i = x_r + 1 and x_stride = 2).  window: n values; segments start every
 *      `step` samples, S = (t - n) / step + 1 of them.
 *   pxx[r][k] = sum_s |FFT_n(x_seg(r, s) * window)_k|^2 / (S * scale), scale = fs * sum w^2 (DENSITY) or (sum w)^2
 *      (SPECTRUM), computed on the device.  Contiguous [rows, n].
 *   cplxamd_welch_bwd: dx (strided as x, written, not accumulated) of sum_{r,k} g[r][k] pxx[r][k], g contiguous [rows, n]:
 *      the gradient of the real pair (re, im), dx = 2 / (S scale) sum_s w_j sum_k g_k X_{s,k} e^{+2 pi i j k / n}.
 * dtype: F32 (x, window, pxx, g, dx float32), BF16 (x and dx bf16, window / pxx / g float32, float32 arithmetic) or
 * F64.  1 <= n <= CPLXAMD_WELCH_MAX_N.  Deterministic: no atomics, fixed summation orders.
 * cplxamd_welch_plan is a pure function (no GPU): the path the transform takes (CPLXAMD_WELCH_*) and the workspace
 * bytes of each direction (nullable outputs); CPLXAMD_EINVAL for n outside [1, CPLXAMD_WELCH_MAX_N] or a bad dtype.
 * fwd / bwd check every argument before any launch: CPLXAMD_EINVAL (bad value / NULL), CPLXAMD_EWS (workspace smaller
 * than the plan's), CPLXAMD_ESHAPE (more than 2^31 - 1 workgroups).
 * ---------------------------------------------------------------------------------- */
#define CPLXAMD_WELCH_MAX_N (1 << 22)
enum { CPLXAMD_WELCH_DIRECT = 0,             /* n = 2^k <= 16384 (float32, bf16) / 8192 (float64), in LDS             */
       CPLXAMD_WELCH_FOURSTEP = 1,           /* n = 2^k above that: four-step N1 x N2 through the workspace             */
       CPLXAMD_WELCH_BLUESTEIN = 2,          /* other n, M = 2^ceil(log2(2n - 1)) within the LDS limit                  */
       CPLXAMD_WELCH_BLUESTEIN_FOURSTEP = 3  /* other n, M above it                                                     */ };
enum { CPLXAMD_WELCH_DENSITY = 0, CPLXAMD_WELCH_SPECTRUM = 1 };
int cplxamd_welch_plan(int64_t n, int64_t rows, int64_t segments, int dtype, int64_t* ws_fwd_bytes,
                       int64_t* ws_bwd_bytes);
int cplxamd_welch_fwd(const void* x_r, const void* x_i, int64_t x_row_stride, int64_t x_stride, int64_t rows, int64_t t,
                      const void* window, int64_t n, int64_t step, int scaling, double fs, void* pxx, void* ws,
                      int64_t ws_bytes, int dtype, void* stream);
int cplxamd_welch_bwd(const void* x_r, const void* x_i, int64_t x_row_stride, int64_t x_stride, int64_t rows, int64_t t,
                      const void* window, int64_t n, int64_t step, int scaling, double fs, const void* g, void* dx_r,
                      void* dx_i, int64_t dx_row_stride, int64_t dx_stride, void* ws, int64_t ws_bytes, int dtype,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * Discrete Fourier transforms of planar complex tensors (cplx.fft / ifft / fft2 / fftn; csrc/fft.hip on the engine of
 * csrc/fft_engine.h, which the Welch spectra share).  New exports under ABI 25: nothing existing changes.
 *   y[v][k] = scale * sum_{j < n_in} x[v][j] e^{-+ 2 pi i j k / n},  k in [0, n),  for every vector v of the batch.
 * Element j of vector v = (i0, i1, i2) lies at x_r / x_i [sum_r i_r x_stride[r] + j x_es], output k at y_r / y_i
 * [sum_r i_r y_stride[r] + k y_es]: element strides, 64-bit offsets, `runs` batch runs with run 0 outermost (the vectors
 * one workgroup transforms together are consecutive in the LAST run).  x strides may be zero (broadcast); x and y must
 * not overlap, and distinct outputs must not alias.  Elements n_in .. n - 1 of a vector are zeros and are never loaded.
 * Dtype pairs (in, out): (F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16), (F64, F64); bf16 is widened on load, the
 * arithmetic is float32 (float64 for F64), and every output is rounded once, on store.  The transform is unnormalised:
 * `scale` multiplies the result before that rounding.
 * cplxamd_fft_plan is a pure function (no GPU): it returns the path (CPLXAMD_WELCH_*; DIRECT / BLUESTEIN here mean "inside
 * one workgroup's LDS", the FOURSTEP codes "through the workspace") of a length-n transform of `vectors` vectors whose
 * INPUT dtype is `dtype`, how many vectors one workgroup transforms (2048 / M for a packed M = 2^k in [8, 1024], 256 below
 * 8, else 1; M = n, or Bluestein's 2^ceil(log2(2n - 1))), and the workspace bytes (nullable outputs); CPLXAMD_EINVAL for
 * n outside [1, CPLXAMD_WELCH_MAX_N], negative `vectors` or a bad dtype.  cplxamd_fft goes through the same plan and
 * checks every argument before any launch: CPLXAMD_EINVAL (NULL pointer -- the workspace included --, bad dtype pair, n /
 * n_in / strides / runs / sizes out of range, unknown bits in `inverse`, a scale that is not finite), CPLXAMD_ESHAPE
 * (more than 2^31 - 1 vectors), CPLXAMD_EWS (workspace smaller than the plan's).  Zero vectors: no launch, returns 0.
 * The tables of a call (twiddles, chirp, B-hat) are built in its workspace: no state in the library, no atomics, the same
 * input gives the same bits, capturable in a hipGraph.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_FFT_INVERSE = 1,              /* e^{+2 pi i jk/n}, unnormalised                                          */
       CPLXAMD_FFT_ONE_PER_WORKGROUP = 2     /* measurement only: run a packed length with one vector per workgroup     */ };
typedef struct cplxamd_fft_desc {
  int64_t n;            /* transform length, 1 .. 2^22 (CPLXAMD_WELCH_MAX_N) */
  int64_t n_in;         /* inputs read per vector, 1 .. n; elements n_in .. n-1 are zeros (never loaded) */
  int64_t x_es, y_es;   /* element strides along the transformed dim, in elements; x_es may be any value >= 0, y_es >= 1 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t inverse;      /* 0: e^{-2 pi i jk/n}; 1: e^{+2 pi i jk/n} (unnormalised); CPLXAMD_FFT_* bits */
  int64_t size[3], x_stride[3], y_stride[3];
  double  scale;        /* multiplies the result in the epilogue, before its one rounding */
} cplxamd_fft_desc;     /* 120 bytes */
int cplxamd_fft_plan(int64_t n, int64_t vectors, int dtype, int* vectors_per_workgroup, int64_t* ws_bytes);
int cplxamd_fft(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_fft_desc* d,
                int in_dtype, int out_dtype, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Real-input and real-output transforms (cplx.rfft / irfft / rfft2 / rfftn / hfft / ihfft; csrc/rfft.hip on the same
 * engine, batch and descriptor).  New exports under ABI 25: nothing existing changes, cplxamd_fft rejects the bits below.
 * With h = n / 2, w_k = 1 for k = 0 and (n even) k = h, else 2, and the sign of CPLXAMD_FFT_INVERSE:
 *   R2C (default)       y[v][k] = scale [w_k] sum_{j < n_in} x[v][j] e^{-+ 2 pi i jk/n},  k in [0, h];  n_in <= n reals of
 *                       x_r are read (x_i is not looked at and may be NULL); Im y_0 and (n even) Im y_h are stored as 0.
 *                       CPLXAMD_RFFT_WEIGHTED multiplies by w_k (the adjoint of the Hermitian extension).
 *   CPLXAMD_RFFT_C2R    y[v][j] = scale Re sum_{k < n_in} c_k X[v][k] e^{-+ 2 pi i jk/n},  j in [0, n);  n_in <= h + 1
 *                       entries of x_r / x_i are read, Im X_0 and (n even) Im X_h are ignored; y_r alone is written (y_i
 *                       may be NULL).  c_k = w_k with CPLXAMD_RFFT_WEIGHTED (the transform of the Hermitian extension:
 *                       irfft, hfft), c_k = 1 without (the adjoint of R2C).
 * `n` of the descriptor is the REAL length in both directions.  Even n runs one complex transform of h points (packing
 * before, untangling after), odd n of n points; dtype pairs, strides, runs, rounding, errors and the workspace rules are
 * cplxamd_fft's.  cplxamd_rfft_plan is a pure function: the path of that complex transform (CPLXAMD_WELCH_*), its length
 * (`complex_n`: h or n), the power of two actually run (`points`: complex_n, or Bluestein's M), the vectors per
 * workgroup and the workspace bytes, which include the table e^{-2 pi i k/n}, k < h (nullable outputs); `c2r` is 0 or 1.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_RFFT_C2R = 4,                 /* half spectrum in, reals out (default: reals in, half spectrum out)      */
       CPLXAMD_RFFT_WEIGHTED = 8             /* R2C: outputs times w_k; C2R: c_k = w_k (Hermitian extension)            */ };
int cplxamd_rfft_plan(int64_t n, int64_t vectors, int dtype, int c2r, int64_t* complex_n, int64_t* points,
                      int* vectors_per_workgroup, int64_t* ws_bytes);
int cplxamd_rfft(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_fft_desc* d,
                 int in_dtype, int out_dtype, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Short-time Fourier transforms (cplx.stft / istft; csrc/stft.hip on the kernels of cplxamd_rfft and cplxamd_fft).  New
 * exports under ABI 25: nothing existing changes.  With N = n_fft / 2 + 1, the sign and w_k / c_k of cplxamd_rfft
 * (CPLXAMD_FFT_INVERSE, CPLXAMD_RFFT_WEIGHTED in `flags`), a window `win` of n_fft values and P = length + 2 pad:
 *   cplxamd_stft   S[row][f][k] = scale [w_k] sum_{j < n_fft} win[j] x[row][src(f hop + j)] e^{-+ 2 pi i jk/n_fft},
 *                  row < rows, f < frames, k < N.  src(q) is the sample index of position q of the virtually padded
 *                  signal, or "zero" (the term is dropped, nothing is loaded): outside [0, P) zero; with i = q - pad,
 *                  CPLXAMD_STFT_PAD_ZERO gives i when 0 <= i < length, else zero; CPLXAMD_STFT_PAD_REFLECT (pad < length)
 *                  gives -i for i < 0 and 2 (length - 1) - i for i >= length.  Sample i of a row lies at
 *                  x[row sig_row_stride + i sig_es] (strides >= 0), S at y_r / y_i [row spec_row_stride + f
 *                  spec_frame_stride + k spec_es] (strides >= 1; outputs must not alias).  One launch of the R2C kernels
 *                  with the frame axis as the innermost batch run: no frame and no padded copy is materialised.
 *   cplxamd_istft  y[row][t] = e[t] sum_{p in fold(t)} sum_{f ascending, 0 <= p - f hop < n_fft} F[row][f][p - f hop],
 *                  t < length, with F[row][f][j] = win[j] scale Re sum_{k < N} c_k X[row][f][k] e^{-+ 2 pi i jk/n_fft} held in
 *                  the workspace in the compute type, and fold(t) the positions q with src(q) = t, ascending: pad + t, and
 *                  for _REFLECT also pad - t (1 <= t <= pad) and pad + 2 (length - 1) - t (length - 1 - pad <= t <=
 *                  length - 2).  X is read at x_r / x_i with the spec strides (>= 0), y written with the sig strides
 *                  (sig_es >= 1), rounded once.  `envelope` NULL: e = 1 (the adjoint of cplxamd_stft with the same
 *                  fields).  Otherwise it points to length + 1 values of the compute type that the call WRITES: e[t] = 1 /
 *                  env[t], env[t] = sum_{f ascending} win^2[t + pad - f hop] (e = 0 where no frame covers t + pad), and
 *                  at [length] the minimum of |env| over the covered t (untouched when there is none).
 * CPLXAMD_STFT_FULL in `flags` selects the full spectrum on the kernels of cplxamd_fft: N = n_fft, x = x_re + i x_im with
 * x_im the plane `sig_imag` (same strides as x; NULL: a plane of zeros that is never read), no w_k (CPLXAMD_RFFT_WEIGHTED
 * is an error); in cplxamd_istft c_k = 1, F is complex (no Re; two planes of frames in the workspace), y receives the real
 * part and `sig_imag` the imaginary part (NULL: it is not written).  Without the flag `sig_imag` must be NULL.
 * dtype (of x, S, X and y alike): F32, BF16 (float32 arithmetic, window, frames and envelope) or F64; `window` and
 * `envelope` have the compute type.  No atomics and fixed summation orders: the same input gives the same bits.
 * cplxamd_stft_plan is a pure function: frames = 1 + (padded_length - n_fft) / hop, the path (return value), the complex
 * length, the points and the vectors per workgroup of the underlying transform (as cplxamd_rfft_plan for rows x frames
 * vectors; `full` nonzero: as cplxamd_fft_plan of n_fft points), the rows one synthesis chunk holds (frames of a chunk stay within 256 MiB; one row may exceed it) and the
 * workspace bytes of each direction for signals / outputs of `length` samples (nullable outputs); CPLXAMD_EINVAL for
 * out-of-range arguments.  cplxamd_stft_src / _fold are the index maps, compiled from the code the kernels use, for
 * host-side proofs of the addresses: the sample index of (frame, j), -1 for "zero", -2 for arguments out of range; and
 * the number of fold positions of t written to positions[0 .. 2] (CPLXAMD_EINVAL out of range).  The launchers check every
 * argument before any launch: CPLXAMD_EINVAL (NULL, dtype, any field out of range, unknown flag bits, a scale that is not
 * finite, an envelope given to cplxamd_stft), CPLXAMD_ESHAPE (more than 2^31 - 1 frames in all, or offsets beyond 64
 * bits), CPLXAMD_EWS.  Zero rows (and for cplxamd_stft zero frames): no launch, returns 0.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_STFT_PAD_ZERO = 0, CPLXAMD_STFT_PAD_REFLECT = 1 };
enum { CPLXAMD_STFT_FULL = 16 };                 /* full spectrum of a complex signal (default: one-sided, real signal)     */
typedef struct cplxamd_stft_desc {
  int64_t n_fft;             /* frame and transform length, 1 .. 2^22 */
  int64_t hop;               /* >= 1 */
  int64_t frames;            /* per row, >= 0 */
  int64_t length;            /* samples per row: read by cplxamd_stft, written by cplxamd_istft; >= 1 */
  int64_t pad;               /* virtual samples in front of sample 0 (and behind the last), 0 .. 2^22 */
  int64_t rows;
  int64_t sig_row_stride, sig_es;                        /* the signal, in elements */
  int64_t spec_row_stride, spec_frame_stride, spec_es;   /* the spectrogram planes, in elements */
  int32_t pad_mode;          /* CPLXAMD_STFT_PAD_* */
  int32_t flags;             /* CPLXAMD_FFT_INVERSE | CPLXAMD_RFFT_WEIGHTED | CPLXAMD_STFT_FULL */
  const void* window;        /* n_fft values of the compute type */
  void* envelope;            /* cplxamd_istft only, see above; NULL: e = 1 */
  void* sig_imag;            /* CPLXAMD_STFT_FULL only: the signal's imaginary plane (read by cplxamd_stft), or NULL */
  double scale;
} cplxamd_stft_desc;         /* 128 bytes */
int cplxamd_stft_plan(int64_t n_fft, int64_t hop, int64_t padded_length, int64_t rows, int64_t length, int dtype, int full,
                      int64_t* complex_n, int64_t* points, int* vectors_per_workgroup, int64_t* frames,
                      int64_t* rows_per_chunk, int64_t* analysis_ws_bytes, int64_t* synthesis_ws_bytes);
int64_t cplxamd_stft_src(const cplxamd_stft_desc* d, int64_t frame, int64_t j);
int cplxamd_stft_fold(const cplxamd_stft_desc* d, int64_t t, int64_t* positions);
int cplxamd_stft(const void* x, void* y_r, void* y_i, const cplxamd_stft_desc* d, int dtype, void* ws, int64_t ws_bytes,
                 void* stream);
int cplxamd_istft(const void* x_r, const void* x_i, void* y, const cplxamd_stft_desc* d, int dtype, void* ws,
                  int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Linear convolution and correlation along the last dim by overlap-save on the FFT engine (cplx.fftconvolve;
 * csrc/fftconv.hip, fftconv_wgrad.hip).  New exports under ABI 25: nothing existing changes.  Two primitives over rows
 * r = (i0, i1, i2) of up to three batch runs (run 0 outermost), with a[.] = 0 outside [0, a_len):
 *   cplxamd_fftconv        y[r][n] = sum_{m < k} a[r][n + start - m] b[r][m]              (conj = 0: convolution)
 *                          y[r][n] = sum_{m < k} a[r][n + start + m] conj(b[r][m])        (conj = 1: correlation)
 *                          for n in [0, c_len).  b is the filter: a run whose b stride is 0 shares one filter, and one
 *                          spectrum H-hat = FFT_L(b zero-padded to L) / L is built per DISTINCT filter (the product of
 *                          the sizes of the runs with a non-zero b stride) in the workspace, by the packed transform
 *                          kernel of cplxamd_fft with n_in = k.  One launch then runs, per block of L = 2^log_l points,
 *                          load -> FFT -> times H-hat (or its conjugate) -> inverse FFT -> store inside one workgroup;
 *                          y is written once, rounded once.  start and start + c_len may lie anywhere (zeros result
 *                          where no product exists).
 *   cplxamd_fftconv_wgrad  y[f][m] = sum_{rows of f} sum_{n < a_len} conj(a[r][n]) b[r][n + m + start],  m in [0, k),
 *                          with b[.] = 0 outside [0, c_len).  A run whose y stride is 0 is REDUCED: its rows are summed
 *                          into one result.  Per (result, chunk) one workgroup accumulates conj(A-hat) B-hat over its
 *                          chunk of (reduced row, block) pairs in ascending order in registers and writes one partial
 *                          spectrum to the workspace; the partials of a result are summed in ascending chunk order (one
 *                          thread per entry), then one inverse transform keeps k taps (scale 1 / L, one rounding).  No
 *                          atomics.  It has its own block length (the plan's WGRAD fields).
 * Element j of row r of operand t lies at t_r / t_i [sum_q i_q t_stride[q] + j t_es] (y: element stride 1).  a_i, b_i and
 * y_i may each be NULL: a NULL input plane is a plane of zeros that is never read, a NULL y_i is not written (the real
 * part alone is wanted).  dtype (of every plane): F32, BF16 (widened on load, float32 arithmetic and spectra, rounded once
 * on store) or F64.  Each is the other's gradient, so derivatives of every order stay on these two.
 * cplxamd_fftconv_plan is a pure function (no GPU).  It fills out[CPLXAMD_FFTCONV_PLAN_FIELDS] (see the enum) for
 * operands of a_len and k entries, the window (start, c_len), `rows` rows, `filters` distinct filters / results and
 * `conj`; log_l = 0 asks for the plan's own L, a value in [1, 13] with 2^log_l >= k forces it (measurements, exact tests).
 * Returns CPLXAMD_FFTCONV_FUSED, or CPLXAMD_FFTCONV_COMPOSED for k > 4096 (the caller composes cplxamd_fft launches of
 * 2^out[CPLXAMD_FFTCONV_LOG_L] >= a_len + k - 1 points; above 2^22: CPLXAMD_ESHAPE), or CPLXAMD_ESHAPE (fused: filter spectra
 * or one partial spectrum per result beyond 1 TiB, pair counts beyond 64 bits), or CPLXAMD_EINVAL (sizes < 1 -- rows and
 * filters < 0 --, a bad dtype, 2^log_l < k, log_l > 13).  Block j of a row loads a[j S + in_shift + i], i < L, and stores
 * entry i of the cyclic result to y[j S + ((i - out_lo) mod L)] where that index is below min(n_valid, c_len - j S).
 * The launchers run the same plan and check before any launch: CPLXAMD_EINVAL (NULL a_r / b_r / y_r / d / ws, dtype, a
 * field out of range, a composed length), CPLXAMD_ESHAPE (more than 2^31 - 1 blocks), CPLXAMD_EWS.  No rows: returns 0.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_FFTCONV_FUSED = 0, CPLXAMD_FFTCONV_COMPOSED = 1 };
enum { CPLXAMD_FFTCONV_LOG_L = 0,        /* L = 2^this (COMPOSED: of the composed transform length)                    */
       CPLXAMD_FFTCONV_S,                /* outputs per block = the block stride along a row                           */
       CPLXAMD_FFTCONV_BLOCKS,           /* blocks per row                                                             */
       CPLXAMD_FFTCONV_VPW,              /* blocks per workgroup: 2048 / L up to L = 1024 (256 below 8), else 1        */
       CPLXAMD_FFTCONV_IN_SHIFT,         /* see above                                                                  */
       CPLXAMD_FFTCONV_OUT_LO,
       CPLXAMD_FFTCONV_N_VALID,
       CPLXAMD_FFTCONV_WS_BYTES,         /* of cplxamd_fftconv                                                         */
       CPLXAMD_FFTCONV_WGRAD_LOG_L,      /* the same for cplxamd_fftconv_wgrad: its own L, S, blocks per row of a,     */
       CPLXAMD_FFTCONV_WGRAD_S,
       CPLXAMD_FFTCONV_WGRAD_BLOCKS,
       CPLXAMD_FFTCONV_WGRAD_CHUNKS,     /* chunks per result, pairs per chunk                                         */
       CPLXAMD_FFTCONV_WGRAD_PER_CHUNK,
       CPLXAMD_FFTCONV_WGRAD_WS_BYTES,
       CPLXAMD_FFTCONV_PLAN_FIELDS };
typedef struct cplxamd_fftconv_desc {
  int64_t a_len;        /* entries of a row of a, >= 1 */
  int64_t k;            /* filter taps: entries of b (cplxamd_fftconv) or of y (cplxamd_fftconv_wgrad), >= 1 */
  int64_t c_len;        /* entries of y (cplxamd_fftconv) or of b (cplxamd_fftconv_wgrad), >= 1 */
  int64_t start;        /* any sign */
  int64_t a_es, b_es;   /* element strides along the last dim, >= 0 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t conj;         /* cplxamd_fftconv: 0 convolution, 1 correlation; cplxamd_fftconv_wgrad: 0 */
  int32_t log_l;        /* 0: the plan's choice; else L = 2^log_l >= k, log_l <= 13 */
  int32_t reserved;     /* 0 */
  int64_t size[3], a_stride[3], b_stride[3], y_stride[3];
} cplxamd_fftconv_desc; /* 160 bytes */
int cplxamd_fftconv_plan(int64_t a_len, int64_t k, int64_t start, int64_t c_len, int64_t rows, int64_t filters, int dtype,
                         int conj, int log_l, int64_t* out);
int cplxamd_fftconv(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                    const cplxamd_fftconv_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_fftconv_wgrad(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                          const cplxamd_fftconv_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Rational rate change along the last dim on direct-form polyphase kernels (cplx.upfirdn, cplx.resample_poly;
 * csrc/upfirdn.hip, upfirdn_wgrad.hip).  New exports under ABI 25: nothing existing changes.  Write au for a row of a
 * upsampled by `up`: au[i up] = a[i], zero elsewhere and outside the row (never materialised).  Two primitives over rows
 * r = (i0, i1, i2) of up to three batch runs (run 0 outermost):
 *   cplxamd_upfirdn        y[r][n] = sum_{m < k} b[r][m] au[r][n down + off - m]             (conj = 0: convolution)
 *                          y[r][n] = sum_{m < k} conj(b[r][m]) au[r][n down + off + m]       (conj = 1: correlation)
 *                          for n in [0, c_len).  b is the filter (k <= 4096 taps); a run whose b stride is 0 shares one.
 *                          A workgroup takes `vpw` tiles of T consecutive outputs, stages the samples of a the tiles
 *                          touch (zeros outside the row) and the filter in polyphase-major order into LDS, and spends
 *                          ceil(k / up) complex multiply-adds per output: structural zeros are never multiplied.  When
 *                          the filter and the span exceed the LDS budget the taps are walked in `segs` segments of
 *                          `jseg` taps per phase, in ascending order, the sums staying in registers (the same bits).
 *   cplxamd_upfirdn_wgrad  y[f][m] = sum_{rows of f} sum_{n < c_len} conj(au[r][n down + off - m]) b[r][n],  m in [0, k).
 *                          A run whose y stride is 0 is REDUCED.  Workgroup (result, chunk, block of <= 1024 taps) walks
 *                          its chunk of (reduced row, tile of Tn entries of b) pairs in ascending order, one thread per
 *                          tap, and writes a partial to the workspace; a finishing kernel adds the partials of a result
 *                          in ascending chunk order and rounds once.  No atomics: reruns give the same bits.
 * Element j of row r of operand t lies at t_r / t_i [sum_q i_q t_stride[q] + j t_es] (y: element stride 1).  a_i, b_i and
 * y_i may each be NULL: a NULL input plane is a plane of zeros that is never read (the kernels are compiled per real /
 * complex operand pair), a NULL y_i is not written.  dtype (of every plane): F32, BF16 (float32 arithmetic, rounded
 * once on store) or F64.  Each is the other's gradient with up and down swapped.
 * cplxamd_upfirdn_plan is a pure function (no GPU).  It fills out[CPLXAMD_UPFIRDN_PLAN_FIELDS] (see the enum) for rows of
 * a_len entries, k taps, c_len results (wgrad: entries of b), the rates, `rows` rows, `filters` distinct filters / results
 * and the kinds of the operands (a_cplx, b_cplx: 0 real, 1 complex).  Returns CPLXAMD_UPFIRDN_FUSED, or
 * CPLXAMD_UPFIRDN_COMPOSED for k > 4096 (the caller composes cplxamd_fftconv), or CPLXAMD_EINVAL (sizes, up or down < 1,
 * rows or filters < 0, a bad dtype or flag), or CPLXAMD_ESHAPE (up or down above 2^30, lengths above 2^40, |off| above 2^48,
 * more than 2^31 - 1 workgroups, partials beyond 1 TiB).
 * The launchers run the same plan and check before any launch: CPLXAMD_EINVAL (NULL a_r / b_r / y_r / d, a NULL ws of
 * cplxamd_upfirdn_wgrad, dtype, a field out of range, a composed length), CPLXAMD_ESHAPE, CPLXAMD_EWS.  No rows: returns 0.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_UPFIRDN_FUSED = 0, CPLXAMD_UPFIRDN_COMPOSED = 1 };
enum { CPLXAMD_UPFIRDN_T = 0,            /* outputs per tile                                                            */
       CPLXAMD_UPFIRDN_TILES,            /* tiles per row                                                               */
       CPLXAMD_UPFIRDN_VPW,              /* tiles per workgroup (> 1 only when a row is one tile)                       */
       CPLXAMD_UPFIRDN_SPAN,             /* staged samples of a per tile and segment                                    */
       CPLXAMD_UPFIRDN_PHASES,           /* staged phases: min(up, k)                                                   */
       CPLXAMD_UPFIRDN_JSEG,             /* taps per phase and segment; ceil(k / up) when the filter is staged whole    */
       CPLXAMD_UPFIRDN_SEGS,             /* segments                                                                    */
       CPLXAMD_UPFIRDN_LDS_BYTES,
       CPLXAMD_UPFIRDN_THREADS,
       CPLXAMD_UPFIRDN_GRID,
       CPLXAMD_UPFIRDN_WGRAD_TN,         /* cplxamd_upfirdn_wgrad: entries of b per tile, tiles per row,                */
       CPLXAMD_UPFIRDN_WGRAD_TILES,
       CPLXAMD_UPFIRDN_WGRAD_KB,         /* taps per workgroup, blocks of taps                                          */
       CPLXAMD_UPFIRDN_WGRAD_KBLOCKS,
       CPLXAMD_UPFIRDN_WGRAD_SPAN,       /* staged samples of a per tile                                                */
       CPLXAMD_UPFIRDN_WGRAD_LDS_BYTES,
       CPLXAMD_UPFIRDN_WGRAD_CHUNKS,     /* chunks per result, pairs per chunk                                          */
       CPLXAMD_UPFIRDN_WGRAD_PER_CHUNK,
       CPLXAMD_UPFIRDN_WGRAD_WS_BYTES,
       CPLXAMD_UPFIRDN_PLAN_FIELDS };
typedef struct cplxamd_upfirdn_desc {
  int64_t a_len;        /* entries of a row of a, >= 1 */
  int64_t k;            /* filter taps: entries of b (cplxamd_upfirdn) or of y (cplxamd_upfirdn_wgrad), >= 1 */
  int64_t c_len;        /* entries of y (cplxamd_upfirdn) or of b (cplxamd_upfirdn_wgrad), >= 1 */
  int64_t up, down;     /* >= 1 */
  int64_t off;          /* any sign */
  int64_t a_es, b_es;   /* element strides along the last dim, >= 0 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t conj;         /* cplxamd_upfirdn: 0 convolution, 1 correlation; cplxamd_upfirdn_wgrad: 0 */
  int64_t size[3], a_stride[3], b_stride[3], y_stride[3];
} cplxamd_upfirdn_desc; /* 168 bytes */
int cplxamd_upfirdn_plan(int64_t a_len, int64_t k, int64_t c_len, int64_t up, int64_t down, int64_t off, int64_t rows,
                         int64_t filters, int dtype, int conj, int a_cplx, int b_cplx, int64_t* out);
int cplxamd_upfirdn(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                    const cplxamd_upfirdn_desc* d, int dtype, void* stream);
int cplxamd_upfirdn_wgrad(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                          const cplxamd_upfirdn_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Recursive (IIR) filtering along the last dim on a chunk-parallel kernel (cplx.lfilter, cplx.sosfilt; csrc/iir.hip).
 * New exports under ABI 25: nothing existing changes.  One primitive over rows r = (i0, i1, i2) of up to three batch runs
 * (run 0 outermost), each row cut into `segments` segments of seg_len samples (the last one shorter):
 *   for every (row, segment): take the entering state zi[r][seg] (zeros when zi_r is NULL), run the cascade of
 *   `sections` direct-form-II-transposed sections of order `order` over the segment's samples in order, carrying one
 *   state per section, store y (unless y_r is NULL) and the final state zf[r][seg] (unless zf_r is NULL).
 *     section:  y[n] = b0 x[n] + z0,   z_i = b_{i+1} x[n] - a_{i+1} y[n] + z_{i+1}  (i < order, z_order = 0)
 *   CPLXAMD_IIR_REVERSE runs the recurrence from the last sample of the row to the first (segment 0 is then the END of
 *   the row), CPLXAMD_IIR_CONJ conjugates the coefficients.  x_r NULL is a null input (zeros that are never read).
 * The coefficients of row r lie at c_r / c_i [sum_q i_q c_stride[q]] as [sections][2 (order + 1)] dense entries, section s
 * holding b0 .. b_order, a0 .. a_order; a0 is NOT read (the caller normalises: it counts as 1).  A run whose c stride is 0
 * shares one filter.  Sample j of row r of x lies at x_r / x_i [sum_q i_q x_stride[q] + j x_es]; y likewise with element
 * stride 1.  zi and zf are dense [rows][segments][sections][order] planes, rows in run order.
 * `cplx` = 0: real arithmetic, every imaginary pointer must be NULL.  `cplx` = 1: complex arithmetic; x_i, c_i, zi_i may
 * each be NULL (a plane of zeros that is never read), y_i / zf_i must be given where y_r / zf_r are.
 * dtype (of every plane): F32, BF16 (float32 arithmetic and state, rounded once on store) or F64.
 * Order: 1 .. 8 with one section, 1 .. 2 with 2 .. 16 sections (kernels are compiled for 2 and 8 states and the
 * coefficients zero-padded).  Section s + 1 reads section s's tile from LDS; x is read once and y written once.
 * Inside a tile of LANES * CHUNK samples (a workgroup is one wave, a lane per chunk) each lane runs one chunk of CHUNK
 * samples from zero state, the chunk-final states are combined across the lanes IN ORDER with the CHUNK-step transition
 * M = A^CHUNK (P_c = M P_{c-1} + s_c; only M is ever applied, so integer operands stay exact as long as the sequential
 * recurrence's values times CHUNK + 1 fit the mantissa), and every chunk is corrected by the zero-input response of its
 * entering state; the tables (`order` zero-input responses of CHUNK samples, M) are rebuilt in LDS by every workgroup,
 * nothing is kept in the library.  No workgroup waits for another, no atomics: reruns give the same bits.
 * cplxamd_iir_plan is a pure function (no GPU): fills out[CPLXAMD_IIR_PLAN_FIELDS] for rows of n samples;
 * force_segments > 0 cuts every row into that many segments (at most n), 0 lets the plan choose.  Returns
 * CPLXAMD_IIR_ROW (one segment) or CPLXAMD_IIR_SPLIT, or CPLXAMD_EINVAL / CPLXAMD_ESHAPE (n above 2^40, order or sections
 * out of range, more than 2^31 - 1 workgroups).
 * cplxamd_iir checks before any launch: CPLXAMD_EINVAL (NULL c_r / d, neither y_r nor zf_r, a plane that `cplx`
 * forbids or a missing one, dtype, a field out of range, seg_len * segments < n), CPLXAMD_ESHAPE.  No rows: returns 0.
 * The state planes zi and zf are in the COMPUTE type whatever the dtype: float32 for F32 and BF16, float64 for F64.
 * cplxamd_iir_scan is the split path's hand-off between launches: for every row, sequentially over its segments,
 *   e[r][0] = zi[r] (or zeros),  e[r][k + 1] = M[r / rows_per_filter] e[r][k] + z[r][k],   k + 1 < segments
 * with z [rows][segments][w] the segment-final states from zero entering state (one cplxamd_iir launch with zi NULL
 * and y NULL), M [filters][w][w] the transition of a full segment stored as M[f][j][i] = component i of the final state
 * from the unit entering state e_j (one cplxamd_iir launch of `filters * w` rows of seg_len null samples), w =
 * sections * order, and rows_per_filter consecutive rows sharing a filter; it writes the entering states
 * e [rows][segments][w], which a last cplxamd_iir launch takes as zi.  One thread per row, fixed order, compute-type
 * planes (dtype F32 or F64); m_i, zi_i NULL are planes of zeros, cplx = 0 forbids every imaginary pointer.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_IIR_ROW = 0, CPLXAMD_IIR_SPLIT = 1 };
enum { CPLXAMD_IIR_REVERSE = 1, CPLXAMD_IIR_CONJ = 2 };
enum { CPLXAMD_IIR_CHUNK = 0,            /* samples per lane                                                            */
       CPLXAMD_IIR_LANES,                /* chunks per tile                                                             */
       CPLXAMD_IIR_TILE,                 /* samples per tile: CHUNK * LANES                                             */
       CPLXAMD_IIR_TILES,                /* tiles per segment                                                           */
       CPLXAMD_IIR_SEGMENTS,
       CPLXAMD_IIR_SEG_LEN,
       CPLXAMD_IIR_BUCKET,               /* compiled states per section: 2 or 8                                         */
       CPLXAMD_IIR_LDS_BYTES,
       CPLXAMD_IIR_THREADS,
       CPLXAMD_IIR_GRID,                 /* rows * segments                                                             */
       CPLXAMD_IIR_WS_BYTES,             /* split path: z, M and e of cplxamd_iir_scan for `filters` filters            */
       CPLXAMD_IIR_PLAN_FIELDS };
typedef struct cplxamd_iir_desc {
  int64_t n;            /* samples per row, >= 1 */
  int64_t order;        /* states per section */
  int64_t sections;     /* >= 1 */
  int64_t segments;     /* >= 1 */
  int64_t seg_len;      /* >= 1, seg_len * segments >= n > seg_len * (segments - 1) */
  int64_t x_es;         /* element stride of x along the last dim, >= 0 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t flags;        /* CPLXAMD_IIR_REVERSE | CPLXAMD_IIR_CONJ */
  int64_t size[3], x_stride[3], c_stride[3], y_stride[3];
} cplxamd_iir_desc; /* 152 bytes */
int cplxamd_iir_plan(int64_t n, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype, int cplx,
                     int64_t force_segments, int64_t* out);
int cplxamd_iir(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r, const void* zi_i,
                void* y_r, void* y_i, void* zf_r, void* zf_i, const cplxamd_iir_desc* d, int cplx, int dtype, void* stream);
int cplxamd_iir_scan(const void* z_r, const void* z_i, const void* m_r, const void* m_i, const void* zi_r,
                     const void* zi_i, void* e_r, void* e_i, int64_t rows, int64_t rows_per_filter, int64_t segments,
                     int64_t width, int cplx, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Zero-phase filtering (cplx.filtfilt, cplx.sosfiltfilt; csrc/filtfilt.hip): the EXTENDED pass of the recurrence above.
 * New exports under ABI 25: nothing existing changes, cplxamd_iir and its descriptor are as they were.  The pass is
 * cplxamd_iir's primitive (same kernel body, same tile / chunk / segment scheme, same rules) with three additions:
 *   1. the row the recurrence sees has n + 2 edge LOGICAL samples: x extended by `edge` < n samples on each side, formed
 *      by the loader from x where it lies (no padded copy).  Logical sample m is, by the index map cplxamd_filtfilt_src,
 *      x[j], x[k] or 2 x[k] - x[j]:   ODD 2 x[0] - x[edge - m] | x[m - edge] | 2 x[n - 1] - x[2 (n - 1) + edge - m],
 *      EVEN x[edge - m] | .. | x[2 (n - 1) + edge - m],  CONSTANT x[0] | .. | x[n - 1].  edge = 0: the row itself.
 *   2. CPLXAMD_FILTFILT_SCALE: zi is a UNIT state [sections][order] per filter (found through z_stride, as the
 *      coefficients are through c_stride) and the entering state of the row is that state times the first logical sample
 *      in processing order (the last one under CPLXAMD_FILTFILT_REVERSE); a complex product when cplx = 1.  Only with
 *      segments = 1.  Without the flag zi is cplxamd_iir's dense [rows][segments][sections][order].
 *   3. only the logical samples [y_lo, y_lo + y_n) are stored, at y[m - y_lo], in out_dtype.
 * x is read in in_dtype, y written in out_dtype: (F32, F32), (BF16, F32), (F32, BF16) or (F64, F64).  The coefficients
 * and every state plane are in the compute type (float32; float64 for F64).  Zero-phase filtering is two passes: x ->
 * a compute-type workspace of n + 2 edge samples (SCALE), then the workspace reversed -> y with the window [edge, edge + n)
 * (REVERSE | SCALE, edge 0): for bf16 operands the intermediate signal is never rounded to bf16.
 * cplxamd_filtfilt_plan (pure, no GPU) fills out[CPLXAMD_FILTFILT_PLAN_FIELDS]: cplxamd_iir_plan's fields for rows of
 * n + 2 edge samples (the LDS bytes with the anchors: two more words per plane), then the extended length and the bytes
 * of the intermediate workspace; `dtype` is the operands'.  Returns as cplxamd_iir_plan (EINVAL also for edge < 0 or
 * edge >= n).  cplxamd_filtfilt_src (pure) writes out[0] = j, out[1] = k (-1 where absent) of logical sample m; returns
 * 0, or EINVAL for m outside [0, n + 2 edge), edge outside [0, n), n < 1 or an unknown mode.
 * cplxamd_filtfilt_pass checks before any launch as cplxamd_iir does, and: the dtype pair, the mode, 0 <= edge < n,
 * 0 <= y_lo, 1 <= y_n, y_lo + y_n <= n + 2 edge (when y_r is given), SCALE with zi_r and one segment.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_FILTFILT_ODD = 0, CPLXAMD_FILTFILT_EVEN = 1, CPLXAMD_FILTFILT_CONSTANT = 2 };
enum { CPLXAMD_FILTFILT_REVERSE = 1, CPLXAMD_FILTFILT_SCALE = 2 };
enum { CPLXAMD_FILTFILT_LEN = CPLXAMD_IIR_PLAN_FIELDS,   /* n + 2 edge                                              */
       CPLXAMD_FILTFILT_SIGNAL_BYTES,                    /* the intermediate: rows (n + 2 edge) compute-type planes */
       CPLXAMD_FILTFILT_PLAN_FIELDS };
typedef struct cplxamd_filtfilt_desc {
  int64_t n;            /* samples per row of x, >= 1 */
  int64_t edge;         /* extension on each side, 0 <= edge < n */
  int64_t y_lo, y_n;    /* the logical samples that are stored */
  int64_t order, sections, segments, seg_len; /* as cplxamd_iir_desc, over the n + 2 edge logical samples */
  int64_t x_es;         /* element stride of x along the last dim, >= 0 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t flags;        /* CPLXAMD_FILTFILT_REVERSE | CPLXAMD_FILTFILT_SCALE */
  int32_t mode;         /* CPLXAMD_FILTFILT_ODD / _EVEN / _CONSTANT */
  int32_t reserved;     /* 0 */
  int64_t size[3], x_stride[3], c_stride[3], z_stride[3], y_stride[3];
} cplxamd_filtfilt_desc; /* 208 bytes */
int cplxamd_filtfilt_plan(int64_t n, int64_t edge, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype,
                          int cplx, int64_t force_segments, int64_t* out);
int cplxamd_filtfilt_src(int64_t m, int64_t n, int64_t edge, int mode, int64_t* out);
int cplxamd_filtfilt_pass(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r,
                          const void* zi_i, void* y_r, void* y_i, void* zf_r, void* zf_i, const cplxamd_filtfilt_desc* d,
                          int cplx, int in_dtype, int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Strided complex tensor contraction (cplx.einsum with two operands, cplxmodule/cplx.py:1032-1059; csrc/einsum.hip).  A new
 * export under ABI 25: nothing existing changes.
 *   C[b.., m.., n..] = sum_{k..} op(A)[b.., m.., k..] * op(B)[b.., n.., k..],   op = identity or conjugate per operand
 * on planar re / im operands.  The four index groups (CPLXAMD_EINSUM_BATCH / _M / _N / _K) are lists of up to
 * CPLXAMD_EINSUM_MAX_MODES modes; mode 0 of a group is the outermost, the last one runs fastest.  A mode is an extent and
 * its ELEMENT stride in A, B and C (stride_a of an N mode, stride_b of an M mode and stride_c of a K mode are not read).
 * nmodes == 0 stands for one mode of extent 1.  Strides may be zero (broadcast) or negative in A and B; a C stride of a
 * mode of extent > 1 must not be zero.  Every extent and the product of the extents of a group must fit 31 bits.
 * in_dtype = out_dtype = CPLXAMD_F32 (v_mfma_f32_32x32x2_f32: an fmaf chain in k order) or CPLXAMD_BF16
 * (v_mfma_f32_32x32x16_bf16, float32 accumulation, one rounding on store).  The descriptor is a HOST struct and is copied
 * into the kernel arguments: one launch, no workspace, no device-side table, no synchronisation (capturable); no atomics,
 * the same inputs give the same bits.  Any base-pointer alignment and any strides are taken; 16-byte loads are used per
 * operand when the innermost K mode has stride 1 and the base pointer, the other strides and that extent allow it.
 * Checked before any GPU call: NULL pointer, nmodes outside [0, 8], negative extent, zero C stride -> CPLXAMD_EINVAL;
 * a dtype other than F32 / BF16 or in_dtype != out_dtype, a group or the grid beyond 2^31 - 1 -> CPLXAMD_ESHAPE; an
 * empty result (an extent 0 among batch / M / N) -> 0 without a launch; an empty K group writes zeros.
 * ---------------------------------------------------------------------------------- */
#define CPLXAMD_EINSUM_MAX_MODES 8
enum { CPLXAMD_EINSUM_BATCH = 0, CPLXAMD_EINSUM_M = 1, CPLXAMD_EINSUM_N = 2, CPLXAMD_EINSUM_K = 3 };
typedef struct cplxamd_einsum_desc {
  int32_t nmodes[4];
  int32_t extent[4][CPLXAMD_EINSUM_MAX_MODES];
  int64_t stride_a[4][CPLXAMD_EINSUM_MAX_MODES];
  int64_t stride_b[4][CPLXAMD_EINSUM_MAX_MODES];
  int64_t stride_c[4][CPLXAMD_EINSUM_MAX_MODES];
} cplxamd_einsum_desc;   /* 912 bytes */
int cplxamd_ceinsum(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* c_r, void* c_i,
                    const cplxamd_einsum_desc* d, int conj_a, int conj_b, int in_dtype, int out_dtype, void* stream);
/* The host-side decisions of cplxamd_ceinsum as a pure function (no GPU call; cplxamd_ceinsum itself goes through it):
 * for descriptor `d`, operand plane ADDRESSES a_r .. b_i (only their low four bits are looked at, nothing is
 * dereferenced) and dtype = in_dtype = out_dtype, writes plan[CPLXAMD_EINSUM_PLAN_*]: the load mode of each operand
 * (CPLXAMD_EINSUM_LOAD_*: KFAST scalar loads along k, KVEC 16-byte loads along k, ROWS scalar loads along the rows, ROWVEC
 * 16-byte loads along the rows, bf16 only), whether the operands and the M / N groups were swapped (C's unit stride lies in
 * an M mode), the tile edge (64 | 128) and the number of workgroups (0: an empty result, no launch).  The modes are those
 * AFTER the swap: MODE_A is the mode of the operand the kernel loads as A, i.e. of the caller's B when SWAPPED is 1.
 * Returns what cplxamd_ceinsum returns for the same descriptor and dtype (CPLXAMD_EINVAL also for a NULL `plan`).
 * A new export under ABI 25: nothing existing changes. */
enum { CPLXAMD_EINSUM_LOAD_KFAST = 0, CPLXAMD_EINSUM_LOAD_KVEC = 1, CPLXAMD_EINSUM_LOAD_ROWS = 2, CPLXAMD_EINSUM_LOAD_ROWVEC = 3 };
enum { CPLXAMD_EINSUM_PLAN_MODE_A = 0, CPLXAMD_EINSUM_PLAN_MODE_B = 1, CPLXAMD_EINSUM_PLAN_SWAPPED = 2,
       CPLXAMD_EINSUM_PLAN_TILE = 3, CPLXAMD_EINSUM_PLAN_GRID = 4, CPLXAMD_EINSUM_PLAN_SIZE = 5 };
int cplxamd_einsum_plan(const cplxamd_einsum_desc* d, uint64_t a_r, uint64_t a_i, uint64_t b_r, uint64_t b_i, int dtype,
                        int64_t* plan);

/* Complex abs-max pooling (cplx.max_poolnd, cplx.py:1114-1175): in every window the element of
 * largest modulus keeps both its parts (first maximum in row-major window order, as torch).
 * pool = int[14]: B, C, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw.  idx: int32 [B, C, Ho, Wo],
 * the selected position h * W + w, written by fwd and read by bwd (a deterministic gather). */
int cplxamd_cplx_maxpool2d_fwd(const void* zr, const void* zi, void* yr, void* yi, int32_t* idx,
                               const int* pool, int dtype, void* stream);
int cplxamd_cplx_maxpool2d_bwd(const void* gr, const void* gi, const int32_t* idx, void* dzr, void* dzi,
                               const int* pool, int dtype, void* stream);
/* the same pair on channels-last planes ([B][H][W][C] in, [B][Ho][Wo][C] out and idx): a pooling layer inside a
 * channels-last convolution stack needs no layout copy */
int cplxamd_cplx_maxpool2d_fwd_cl(const void* zr, const void* zi, void* yr, void* yi, int32_t* idx,
                                  const int* pool, int dtype, void* stream);
int cplxamd_cplx_maxpool2d_bwd_cl(const void* gr, const void* gi, const int32_t* idx, void* dzr, void* dzi,
                                  const int* pool, int dtype, void* stream);

/* Bilinear layers: cplx.bilinear (cplx.py:1062-1087), the variance term of
 * CplxBilinearGaussian / BilinearGaussian (nn/relevance/complex/base.py:59-84, real/base.py:52-77).
 *   y[b,o] = sum_i u[b,i] T[b,o,i] + bias[o],   u = conj(x1) if conj_u else x1,
 * where T[b,(o,i)] = sum_j W[o,i,j] x2[b,j] comes from cplxamd_cgemm / cplxamd_rgemm with the
 * weight read as stored ([O*I1, I2]).  u: [B, I1], T: [B, O, I1], y, g: [B, O], all contiguous and
 * of one dtype; bias float32 [O] or NULL.  Real tensors: every imaginary plane NULL.
 * bwd: dT = g conj(u) (real: g u), du = sum_o g conj(T) mapped back to x1 (conjugated again when
 * conj_u); either output pair may be NULL (T may then be NULL too when du is not wanted). */
int cplxamd_bilinear_reduce_fwd(const void* ur, const void* ui, const void* tr, const void* ti,
                                const float* bias_r, const float* bias_i, void* yr, void* yi, int64_t B,
                                int O, int I1, int conj_u, int dtype, void* stream);
int cplxamd_bilinear_reduce_bwd(const void* ur, const void* ui, const void* tr, const void* ti,
                                const void* gr, const void* gi, void* dx1r, void* dx1i, void* dtr,
                                void* dti, int64_t B, int O, int I1, int conj_u, int dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * float64 (ABI 23; csrc/f64.hip): the contractions of the reference's `.double()` models and the exponential integral,
 * as a PARITY mode -- plain v_fma_f64 kernels, nothing tuned.  The float64 layers of the host package
 * (cplxmodule_amd/f64.py) spell their elementwise algebra with torch ops under autograd, as the reference does, and call
 * these for what torch would hand to a vendor library (or to scipy on the host).
 *   cplxamd_gemm_f64     C[z][m][n] = sum_k A[z][m][k] op(B[z][n][k]) (+ bias[n]); element strides (row, column, batch) per
 *                        operand, planar complex (a_i / b_i / c_i all non-NULL) or real (all NULL); conj_b: conj(B).
 *                        cplx.py:634-648, :167-174 and their autograd (dX = G conj(W), dW = G^T conj(X)).
 *   cplxamd_conv2d_f64   mode 0: y = x (*) w + bias (p = x, q = w); mode 1: dx = data gradient (p = g, q = w); mode 2:
 *                        dw = weight gradient (p = g, q = x); NCHW planes, complex or real, any stride / padding / dilation /
 *                        groups; geom = {B, Ci, Co, H, W, KH, KW, sh, sw, ph, pw, dh, dw, groups}.  cplx.py:717-838.
 *   cplxamd_expi_f64     y = Ei(x), both signs, ~1e-15 relative to scipy.special.expi.  nn/relevance/complex/vd.py:15-44.
 * ---------------------------------------------------------------------------------- */
int cplxamd_gemm_f64(const double* a_r, const double* a_i, int64_t a_rs, int64_t a_cs, int64_t a_bs,
                     const double* b_r, const double* b_i, int64_t b_rs, int64_t b_cs, int64_t b_bs,
                     const double* bias_r, const double* bias_i, double* c_r, double* c_i, int64_t ldc, int64_t c_bs,
                     int batch, int M, int N, int K, int conj_b, void* stream);
int cplxamd_conv2d_f64(const double* p_r, const double* p_i, const double* q_r, const double* q_i, const double* bias_r,
                       const double* bias_i, double* out_r, double* out_i, const int* geom, int mode, void* stream);
int cplxamd_expi_f64(const double* x, double* y, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * Finishing kernels of the semi-unitary initialiser (cplx_trabelsi_independent_, cplxmodule/nn/init.py:90-123; csrc/
 * init.hip).  New exports under ABI 25: nothing existing changes.  The unitary polar factor of a random matrix comes from
 * the Newton-Schulz recurrence X <- X (1.5 I - 0.5 X^H X) on cplxamd_cgemm_fl / cplxamd_gemm_f64; these three passes are
 * what is left around the two GEMMs of a step.  Planes are dense, dtype = CPLXAMD_F32 or CPLXAMD_F64 (the arithmetic of
 * the iteration); sums are float64, reduced in a fixed order through `ws` (cplxamd_init_ws_bytes() bytes, 8-byte aligned):
 * the same input gives the same bits, no atomics.
 *   cplxamd_init_moments      out[0..2] = sum re, sum im, sum (re^2 + im^2) over n elements (device float64[3]).
 *   cplxamd_init_ns_poly      P = a I + b G on the k x k planes of G (one fma on the diagonal, one product elsewhere, in
 *                             the planes' arithmetic) and *resid2 = ||G - I||_F^2 (device float64).
 *   cplxamd_init_scale_store  out = in * f on [rows, cols] planes, or with transpose != 0 the hermitian transpose
 *                             out[c][r] = conj(in[r][c]) * f ([cols, rows]); the float64 product is rounded ONCE to
 *                             out_dtype: F32 or BF16 for F32 planes, F64 for F64 planes (the casts a parameter needs;
 *                             any other pair: CPLXAMD_EINVAL).  f is derived ON THE DEVICE from moments[0..2] (device float64,
 *                             as cplxamd_init_moments writes them; n = rows * cols):
 *                               CPLXAMD_INIT_SCALE_NORM   f = target / sqrt(m2)                       (1 / ||in||_F)
 *                               CPLXAMD_INIT_SCALE_STD    f = target / sqrt(m2 / n - |m0 + i m1|^2 / n^2)   (std -> target)
 *                               CPLXAMD_INIT_SCALE_CONST  f = target (moments not read, may be NULL)
 *                             The launcher cannot know a device value, so a bad factor is reported on the device: when the
 *                             radicand is 0, negative or not finite (or f is not finite) NOTHING is stored and *status
 *                             (device float64, nullable) is set to 1, else to 0 -- never an infinite or NaN output.
 * Checked before any launch (CPLXAMD_EINVAL): NULL planes / outputs / ws, n <= 0, k <= 0, rows or cols <= 0, a plane dtype
 * other than F32 / F64, an unknown out_dtype or mode, a NaN target; more than 2^31 - 1 tiles: CPLXAMD_ESHAPE.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_INIT_SCALE_NORM = 0, CPLXAMD_INIT_SCALE_STD = 1, CPLXAMD_INIT_SCALE_CONST = 2 };
int64_t cplxamd_init_ws_bytes(void);
int cplxamd_init_moments(const void* re, const void* im, int64_t n, int dtype, double* out, void* ws, void* stream);
int cplxamd_init_ns_poly(const void* g_r, const void* g_i, void* p_r, void* p_i, int k, double a, double b, int dtype,
                         double* resid2, void* ws, void* stream);
int cplxamd_init_scale_store(const void* in_r, const void* in_i, void* out_r, void* out_i, int64_t rows, int64_t cols,
                             int transpose, int mode, double target, const double* moments, double* status, int in_dtype,
                             int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Structured compaction of the masked layers (cplxmodule_amd/compact.py; csrc/compact.hip).  New exports under ABI 25:
 * nothing existing changes.  A masked layer whose mask has dead rows (output features) or dead columns (input features)
 * runs the dense kernels on gathered operands and expands the results.  Every kernel is a deterministic copy (no
 * atomics), capturable, on CPLXAMD_F32 or CPLXAMD_BF16 planes; a second plane (`*_i`) is optional and always comes with
 * its output.  Index lists are int32.
 *   cplxamd_live_index      mask float32 [O, C, T] (T = 1: a linear weight; a convolution weight has T = kh kw).  rows /
 *                           cols: the ascending lists of the indices o / c with any(mask[o, :, :] != 0) /
 *                           any(mask[:, c, :] != 0), padded with the LOWEST-numbered dead indices (list kept ascending) up
 *                           to min(total, the next multiple of `granule`); an empty live set stays empty.  inv_rows[O] /
 *                           inv_cols[C]: position in the list, or -1.  counts (device int32[4]) = live rows, listed rows,
 *                           live columns, listed columns.  rows / cols must hold O / C entries (only the listed prefix
 *                           is written).  1 <= O, C, T <= 2^20 (else CPLXAMD_ESHAPE); ws: cplxamd_live_index_ws_bytes(O, C).
 *   cplxamd_gather_axis     out[o, j, i] = src[o, idx[j], i]: src [outer, axis, inner] -> out [outer, n_idx, inner].
 *   cplxamd_expand_axis     its adjoint as ONE pass over the full output (no memset, no scatter):
 *                           out[o, a, i] = inv[a] >= 0 ? src[o, inv[a], i] : fill[a]   (fill float32 [axis], NULL: 0),
 *                           src [outer, n_idx, inner] -> out [outer, axis, inner].
 *                           Both move 16 bytes per lane where inner and the pointers allow it, single elements otherwise.
 *   cplxamd_compact_weight  out[r, c, t] = w[rows[r], cols[c], t] * mask[rows[r], cols[c], t], w [O, C, T] ->
 *                           out [n_rows, n_cols, T] converted to out_dtype (the compacted cplxamd_mask_mul).
 *   cplxamd_expand_weight   its adjoint: out[o, c, t] = src[inv_rows[o], inv_cols[c], t] * mask[o, c, t] where both
 *                           inverse entries are >= 0, else an exact 0; src [n_rows, n_cols, T] -> out [O, C, T].
 * ---------------------------------------------------------------------------------- */
int64_t cplxamd_live_index_ws_bytes(int64_t O, int64_t C);
int cplxamd_live_index(const float* mask, int64_t O, int64_t C, int64_t T, int granule, int* rows, int* cols, int* inv_rows,
                       int* inv_cols, int* counts, void* ws, int64_t ws_bytes, void* stream);
int cplxamd_gather_axis(const void* src_r, const void* src_i, const int* idx, void* out_r, void* out_i, int64_t outer,
                        int64_t axis, int64_t n_idx, int64_t inner, int dtype, void* stream);
int cplxamd_expand_axis(const void* src_r, const void* src_i, const int* inv, const float* fill_r, const float* fill_i,
                        void* out_r, void* out_i, int64_t outer, int64_t n_idx, int64_t axis, int64_t inner, int dtype,
                        void* stream);
int cplxamd_compact_weight(const void* w_r, const void* w_i, const float* mask, const int* rows, const int* cols, void* out_r,
                           void* out_i, int64_t O, int64_t C, int64_t T, int64_t n_rows, int64_t n_cols, int in_dtype,
                           int out_dtype, void* stream);
int cplxamd_expand_weight(const void* src_r, const void* src_i, const float* mask, const int* inv_rows, const int* inv_cols,
                          void* out_r, void* out_i, int64_t O, int64_t C, int64_t T, int64_t n_rows, int64_t n_cols,
                          int in_dtype, int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Chirp-z transforms of planar complex tensors (cplx.czt / zoom_fft; csrc/czt.hip on the engine of csrc/fft_engine.h).
 * New exports under ABI 25: nothing existing changes.  With w = e^{w_log + 2 pi i w_turn}, a = e^{a_log + 2 pi i a_turn}:
 *   y[v][k] = scale * sum_{j < n} x[v][j] a^{-j} w^{jk},  k in [0, m)                       (flags = 0)
 *   y[v][k] = scale * a^{-k} sum_{j < n} x[v][j] w^{jk},  k in [0, m)                       (CPLXAMD_CZT_A_OUT)
 * for every vector v of the batch; the adjoint of the first form with (n, m, w, a) is the second with (m, n, conj w, conj
 * a), i.e. both turn fractions negated.  Planes, element strides and batch runs are cplxamd_fft's (x strides may be zero,
 * x and y must not overlap); x_i may be NULL: a plane of zeros that is never read.  Dtype pairs (in, out) as cplxamd_fft:
 * bf16 is widened on load, the arithmetic is float32 (float64 for F64), every output is rounded once, on store.
 * The transform is Bluestein's convolution of length n + m - 1 at M = 2^ceil(log2(n + m - 1)), M >= 8.  cplxamd_czt_plan is
 * a pure function (no GPU): it returns the path (CPLXAMD_CZT_*), how many vectors one workgroup transforms (2048 / M when
 * packed, else 1) and the workspace bytes (nullable outputs); CPLXAMD_EINVAL for n or m < 1, negative `vectors` or a bad
 * dtype, CPLXAMD_ESHAPE for M above CPLXAMD_WELCH_MAX_N.  cplxamd_czt goes through the same plan and checks every argument
 * before any launch: CPLXAMD_EINVAL (NULL pointer other than x_i -- the workspace included --, bad dtype pair, n / m /
 * strides / runs / sizes out of range, unknown flags, a contour parameter or scale that is not finite), CPLXAMD_ESHAPE (M
 * too large, more than 2^31 - 1 vectors), CPLXAMD_EWS (workspace smaller than the plan's).  Zero vectors: no launch,
 * returns 0.  The tables of a call (twiddles, opening and closing chirp, B-hat) are built in its workspace, in float64
 * from the log-moduli and turn fractions (the phase theta i^2 / 2 mod 1 exactly reduced) and rounded once: no state in the
 * library, no atomics, the same input gives the same bits, capturable in a hipGraph.  Off the unit circle the tables span
 * a factor e^D, D = |w_log| max(n, m)^2 / 2 + |a_log| n, and the result loses that much precision (a property of the
 * algorithm): callers should refuse D beyond ln 2^24 (float32) / ln 2^53 (float64); the library does not look at D.
 * ---------------------------------------------------------------------------------- */
enum { CPLXAMD_CZT_PACKED = 0,               /* M <= 1024: 2048 / M vectors per 256-thread workgroup, one launch        */
       CPLXAMD_CZT_FUSED = 1,                /* M = 2048 .. 8192: one vector per workgroup, one launch                  */
       CPLXAMD_CZT_WORKSPACE = 2             /* M above that: through the workspace (four-step above the LDS limit)     */ };
enum { CPLXAMD_CZT_A_OUT = 1                 /* the power of a multiplies the outputs (a^{-k}), not the inputs          */ };
typedef struct cplxamd_czt_desc {
  int64_t n, m;         /* inputs read and outputs written per vector, each >= 1, n + m - 1 <= 2^22 */
  int64_t x_es, y_es;   /* element strides along the transformed dim, in elements; x_es >= 0, y_es >= 1 */
  int32_t runs;         /* 0 .. 3 batch runs, run 0 outermost */
  int32_t flags;        /* CPLXAMD_CZT_* bits */
  int64_t size[3], x_stride[3], y_stride[3];
  double  w_log, w_turn;  /* ln |w| and arg(w) / 2 pi */
  double  a_log, a_turn;  /* ln |a| and arg(a) / 2 pi */
  double  scale;        /* multiplies the result in the epilogue, before its one rounding */
} cplxamd_czt_desc;     /* 152 bytes */
int cplxamd_czt_plan(int64_t n, int64_t m, int64_t vectors, int dtype, int* vectors_per_workgroup, int64_t* ws_bytes);
int cplxamd_czt(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_czt_desc* d,
                int in_dtype, int out_dtype, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CPLXAMD_H */
