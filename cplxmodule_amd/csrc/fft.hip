// Discrete Fourier transforms of planar complex tensors (cplx.fft / ifft / fft2 / fftn: cplxmodule_amd/fft.py) on the
// engine of fft_engine.h.  One call transforms every vector of a strided batch along one dim:
//     y[v][k] = scale * sum_{j < n_in} x[v][j] e^{-+ 2 pi i j k / n},   k in [0, n)
// x and y are plane pairs with an element stride along the transformed dim and up to three batch runs (size, x stride, y
// stride), run 0 outermost: vector v of the batch is (i0, i1, i2) in row-major order of the runs.  Elements n_in .. n - 1
// of a vector are zeros that are never loaded (zero padding costs no copy).  bf16 planes are widened on load, the
// arithmetic is float32 (float64 for float64 planes), and every output is rounded once, on store.
//
// Paths (fft_plan_t in fft_engine.h, which rfft.hip shares; the codes are Welch's):
//   packed      M = 2^k <= 1024 points (M = n, or Bluestein's M = 2^ceil(log2(2n - 1))): a 256-thread workgroup transforms
//               V = 256 / kNT<k> vectors (2048 / M; 256 for M < 8), vector threadIdx.x / kNT on lane threadIdx.x % kNT and
//               its own LDS slice.  The V vectors are consecutive in the innermost run.  Along the last dim the engine's
//               loader reads along the vector; along a non-last dim (vectors closer together than their elements) the
//               V x M tile is staged through LDS with the vector index fastest across lanes (STAGED below).
//               A slice is the two padded planes plus one word: an ODD number of words, so that equal positions of
//               neighbouring vectors fall on different banks (for M < 16 pad() adds nothing and the engine's own padding
//               cannot do it; lengths up to 8 are one register stage and touch LDS only in Bluestein's to_lds).
//               The barriers of a stage lie outside its guards: the threads of a partly filled last workgroup load zeros,
//               run every stage and skip the stores -- nothing returns early.
//   one vector  per workgroup for 2^11 .. 2^kLogLMax direct and 2^11 .. 2^13 Bluestein: the same kernel with V = 1.
//   workspace   everything longer: batches of at most GL vectors are gathered into C2 buffers (with the chirp), run
//               through fft_vectors (four-step above the LDS limit), for Bluestein multiplied by B-hat and run back, and
//               scattered with the closing chirp, the scale and the one rounding.
// Bluestein (welch_lds's sequence, plus the closing chirp that |.|^2 let Welch drop):
//     X_k = chirp_k IFFT_M(FFT_M(a) . B-hat)_k,  a_j = x_j chirp_j,  chirp_j = e^{-i pi j^2 / n};
// the inverse transform conjugates the chirp and B-hat (b is even, so FFT(conj b) = conj B-hat).
// The per-call tables (twiddles, chirp, B-hat) are built in the caller's workspace; the library keeps no state.  No
// atomics: the same input gives the same bits.  No kernel uses scratch (-Rpass-analysis=kernel-resource-usage).
#include "fft_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

extern "C" {

int cplxamd_fft_plan(int64_t n, int64_t vectors, int dtype, int* vectors_per_workgroup, int64_t* ws_bytes) {
  FftPlan p;
  if (const int e = fft_plan_for(n, vectors, dtype, p)) return e;
  if (vectors_per_workgroup) *vectors_per_workgroup = p.vpw;
  if (ws_bytes) *ws_bytes = p.bytes;
  return p.path;
}

int cplxamd_fft(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_fft_desc* d, int in_dtype,
                int out_dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_r || !x_i || !y_r || !y_i || !d || !ws) return CPLXAMD_EINVAL;
  const bool f32ish_in = in_dtype == CPLXAMD_F32 || in_dtype == CPLXAMD_BF16;
  const bool f32ish_out = out_dtype == CPLXAMD_F32 || out_dtype == CPLXAMD_BF16;
  if (!((f32ish_in && f32ish_out) || (in_dtype == CPLXAMD_F64 && out_dtype == CPLXAMD_F64))) return CPLXAMD_EINVAL;
  if (d->n < 1 || d->n > CPLXAMD_WELCH_MAX_N || d->n_in < 1 || d->n_in > d->n || d->x_es < 0 || d->y_es < 1 || d->runs < 0 ||
      d->runs > 3 || (d->inverse & ~(CPLXAMD_FFT_INVERSE | CPLXAMD_FFT_ONE_PER_WORKGROUP)) || !(d->scale - d->scale == 0))
    return CPLXAMD_EINVAL;
  Batch b;
  if (const int e = batch_of(*d, b)) return e;
  FftPlan p;
  if (const int e = fft_plan_for(d->n, b.total, in_dtype, p)) return e;
  if (b.total > 0x7fffffffll) return CPLXAMD_ESHAPE;     // workgroups are indexed by one grid dimension
  if (ws_bytes < p.bytes) return CPLXAMD_EWS;
  if (b.total == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (in_dtype == CPLXAMD_F64) return fft_t<double, double, double>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
  if (in_dtype == CPLXAMD_BF16)
    return out_dtype == CPLXAMD_BF16 ? fft_t<bf16_t, bf16_t, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st)
                                     : fft_t<bf16_t, float, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
  return out_dtype == CPLXAMD_BF16 ? fft_t<float, bf16_t, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st)
                                   : fft_t<float, float, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
}

}  // extern "C"
