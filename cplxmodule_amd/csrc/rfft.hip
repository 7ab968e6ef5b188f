// Real-input and real-output Fourier transforms (cplx.rfft / irfft / rfft2 / rfftn / hfft / ihfft: cplxmodule_amd/rfft.py)
// on the engine of fft_engine.h, with the batch, the plan and the kernel structure of fft.hip.  Two linear primitives,
// each the other's adjoint (h = n / 2; w_k = 1 for k = 0 and, n even, k = h, else 2; sg = -1, or +1 with
// CPLXAMD_FFT_INVERSE):
//   R2C   y_k = scale [w_k] sum_{j < n_in} x_j e^{sg 2 pi i jk/n},  k in [0, h]      (real planes in, plane pair out)
//   C2R   x_j = scale Re sum_{k < n_in} c_k X_k e^{sg 2 pi i jk/n}, j in [0, n)      (plane pair in, real plane out)
// with c_k = w_k (CPLXAMD_RFFT_WEIGHTED: the Hermitian extension, irfft / hfft) or c_k = 1 (the plain adjoint of R2C);
// the weights of R2C are the adjoint of the Hermitian extension.  Inputs beyond n_in are zeros that are never loaded; Im
// X_0 and, n even, Im X_h are not read by C2R and are stored as zeros by R2C.
//
// Even n runs ONE complex transform of h points (HALF), on every path of fft.hip -- packed (so a workgroup holds twice
// the vectors of the complex transform of n points), one vector per workgroup, through the workspace:
//   R2C   z_j = x_2j + i x_2j+1,  Z = FFT_h(z),  X_k = (Z_k + conj Z_h-k) / 2 - (i / 2) t_k (Z_k - conj Z_h-k), indices
//         mod h, t_k = e^{sg 2 pi i k/n}.  Z_k and Z_h-k lie on different lanes: the result goes back to the vector's LDS
//         slice (to_lds) and every output reads its pair from there.
//   C2R   Z_k = (X_k + conj X_h-k) + i t_k (X_k - conj X_h-k), k < h, formed by the loader from two loads per element;
//         z = FFT_h(Z) with the sign sg, x_2j = Re z_j, x_2j+1 = Im z_j.
// h need not be a power of two: Bluestein's opening chirp comes after the packing, its closing chirp before the
// untangling.  t_k (multiples of 2 pi / n, which the M-point table does not hold) is one more per-call table in the
// caller's workspace.  Odd n (and n = 1) runs the complex transform of n points: R2C's loader reads no imaginary plane
// and k <= h alone is stored; C2R's loader forms the extension (p <= h ? X_p : conj X_n-p) and the real part alone is
// stored.  No zero plane, no plane written and dropped.  Barriers outside the guards, the STAGED tile order, 64-bit
// offsets, no atomics, no scratch: as fft.hip.
#include "rfft_impl.h"

namespace cplxamd {
namespace sp {
extern template int rfft_any<true>(const void*, const void*, void*, void*, const cplxamd_fft_desc&, int, int, const Batch&,
                                   const RfftPlan&, char*, hipStream_t);        // rfft_c2r.hip
}  // namespace sp
}  // namespace cplxamd

using namespace cplxamd;
using namespace cplxamd::sp;

extern "C" {

int cplxamd_rfft_plan(int64_t n, int64_t vectors, int dtype, int c2r, int64_t* complex_n, int64_t* points,
                      int* vectors_per_workgroup, int64_t* ws_bytes) {
  RfftPlan p;
  if (c2r != 0 && c2r != 1) return CPLXAMD_EINVAL;         // both directions run the same complex transform
  if (const int e = rfft_plan_for(n, vectors, dtype, p)) return e;
  if (complex_n) *complex_n = p.L;
  if (points) *points = p.c.M;
  if (vectors_per_workgroup) *vectors_per_workgroup = p.c.vpw;
  if (ws_bytes) *ws_bytes = p.bytes;
  return p.c.path;
}

int cplxamd_rfft(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_fft_desc* d, int in_dtype,
                 int out_dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_r || !y_r || !d || !ws) return CPLXAMD_EINVAL;
  const bool c2r = (d->inverse & CPLXAMD_RFFT_C2R) != 0;
  if (c2r ? !x_i : !y_i) return CPLXAMD_EINVAL;
  const bool f32ish_in = in_dtype == CPLXAMD_F32 || in_dtype == CPLXAMD_BF16;
  const bool f32ish_out = out_dtype == CPLXAMD_F32 || out_dtype == CPLXAMD_BF16;
  if (!((f32ish_in && f32ish_out) || (in_dtype == CPLXAMD_F64 && out_dtype == CPLXAMD_F64))) return CPLXAMD_EINVAL;
  if (d->n < 1 || d->n > CPLXAMD_WELCH_MAX_N || d->n_in < 1 || d->n_in > (c2r ? d->n / 2 + 1 : d->n) || d->x_es < 0 ||
      d->y_es < 1 || d->runs < 0 || d->runs > 3 ||
      (d->inverse & ~(CPLXAMD_FFT_INVERSE | CPLXAMD_RFFT_C2R | CPLXAMD_RFFT_WEIGHTED)) || !(d->scale - d->scale == 0))
    return CPLXAMD_EINVAL;
  Batch b;
  if (const int e = batch_of(*d, b)) return e;
  RfftPlan p;
  if (const int e = rfft_plan_for(d->n, b.total, in_dtype, p)) return e;
  if (b.total > 0x7fffffffll) return CPLXAMD_ESHAPE;     // workgroups are indexed by one grid dimension
  if (ws_bytes < p.bytes) return CPLXAMD_EWS;
  if (b.total == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  return c2r ? rfft_any<true>(x_r, x_i, y_r, y_i, *d, in_dtype, out_dtype, b, p, (char*)ws, st)
             : rfft_any<false>(x_r, x_i, y_r, y_i, *d, in_dtype, out_dtype, b, p, (char*)ws, st);
}

}  // extern "C"
