// Short-time Fourier transforms (cplx.stft / istft: cplxmodule_amd/stft.py): one-sided spectra of real signals on the
// real-transform kernels of rfft_impl.h, full spectra (CPLXAMD_STFT_FULL: N = n_fft, complex x and F, no w_k / c_k, no
// Re; a null imaginary plane of the signal is zeros on the way in and is not written on the way out) on the complex
// kernels of fft_impl.h.  Two linear primitives, each the other's adjoint (N = n_fft / 2 + 1; sg, w_k, c_k as in rfft.hip):
//   analysis   S[row][f][k] = scale [w_k] sum_{j < n_fft} win[j] x[row][src(f hop + j)] e^{sg 2 pi i jk/n_fft},  k < N
//   synthesis  y[row][t] = e[t] sum_{p in fold(t)} sum_{f ascending, 0 <= p - f hop < n_fft} F[row][f][p - f hop],
//              F[row][f][j] = win[j] scale Re sum_{k < N} c_k X[row][f][k] e^{sg 2 pi i jk/n_fft}
// src (stft_impl.h) maps a position of the virtually padded signal -- `pad` virtual samples on either side, zeros or the
// reflection -- to a sample or to "zero"; fold(t) is its inverse image, at most three positions.  e is 1, or the
// reciprocal of the window envelope sum_f win^2[t + pad - f hop], which the call also hands back with its minimum.
//
// Analysis is ONE launch of the R2C kernels with the frame axis as the innermost batch run: framing, index map and
// window live in the loader (RIo::real_in, Io::in under the StftIn policy), so the packed, one-vector-per-workgroup, Bluestein
// and workspace paths and both the half-length (even n_fft) and the full-length (odd) routes get them from one place.
// No frame, no padded signal and no windowed copy is ever materialised; the overlapping reads of neighbouring frames
// are served by the caches.  Synthesis runs the C2R kernels into a workspace of frames (the window fused into the
// store, StftOut), then ONE gather pass in which every output sample sums its frames in ascending order: no atomics,
// the same input gives the same bits.  Rows are processed in chunks whose frames fit the cap of the four-step buffers
// (a single larger row takes what it needs).  Every argument is checked before any launch; no kernel uses scratch.
#include "stft_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TO, typename T>
int synthesis_t(const void* xr, const void* xi, void* y, const cplxamd_stft_desc& d, int in_dtype, const StftPlan& p, char* ws,
                hipStream_t st) {
  T* env = (T*)(ws + p.off_env);
  T* F = (T*)(ws + p.off_F);
  T* Fi = (T*)(ws + p.off_Fi);
  T* e = (T*)d.envelope;
  const bool full = (d.flags & CPLXAMD_STFT_FULL) != 0;
  if (e) {
    stft_envelope<T><<<ew_grid(d.length), kET, 0, st>>>((const T*)d.window, d.n_fft, d.hop, d.frames, d.pad, d.length, env, e);
    CPLXAMD_CHECK_LAUNCH();
    const int64_t covered = (d.frames - 1) * d.hop + d.n_fft - d.pad;          // what torch.istft checks: the kept range
    const int64_t count = d.frames < 1 || covered < 1 ? 0 : (covered < d.length ? covered : d.length);
    if (count > 0) {
      stft_env_min<T><<<1, kET, 0, st>>>(env, count, e + d.length);
      CPLXAMD_CHECK_LAUNCH();
    }
  }
  for (int64_t r0 = 0; r0 < d.rows; r0 += p.chunk) {
    const int64_t nr = d.rows - r0 < p.chunk ? d.rows - r0 : p.chunk;
    if (d.frames > 0) {                                   // every chunk runs under the first's plan and finds its tables
      if (const int err = full ? stft_full_frames(xr, xi, F, Fi, d, r0, nr, in_dtype, p.c.c, ws, st, r0 == 0)
                               : stft_frames(xr, xi, F, d, r0, nr, in_dtype, p.c, ws, st, r0 == 0))
        return err;
    }
    stft_overlap_add<TO, T><<<ew_grid(nr * d.length), kET, 0, st>>>(F, nr, d.n_fft, d.hop, d.frames, d.pad, d.pad_mode, d.length,
                                                                   e, (TO*)y + r0 * d.sig_row_stride, d.sig_row_stride, d.sig_es);
    CPLXAMD_CHECK_LAUNCH();
    if (full && d.sig_imag) {
      stft_overlap_add<TO, T><<<ew_grid(nr * d.length), kET, 0, st>>>(Fi, nr, d.n_fft, d.hop, d.frames, d.pad, d.pad_mode,
                                                                     d.length, e, (TO*)d.sig_imag + r0 * d.sig_row_stride,
                                                                     d.sig_row_stride, d.sig_es);
      CPLXAMD_CHECK_LAUNCH();
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int cplxamd_stft_plan(int64_t n_fft, int64_t hop, int64_t padded_length, int64_t rows, int64_t length, int dtype, int full,
                      int64_t* complex_n, int64_t* points, int* vectors_per_workgroup, int64_t* frames,
                      int64_t* rows_per_chunk, int64_t* analysis_ws_bytes, int64_t* synthesis_ws_bytes) {
  if (n_fft < 1 || n_fft > CPLXAMD_WELCH_MAX_N || hop < 1 || padded_length < n_fft || rows < 0 || length < 0)
    return CPLXAMD_EINVAL;
  const int64_t fr = 1 + (padded_length - n_fft) / hop;
  StftPlan p;
  if (const int e = stft_plan_for(n_fft, fr, rows, length, dtype, full != 0, p)) return e;
  if (complex_n) *complex_n = p.r.L;
  if (points) *points = p.r.c.M;
  if (vectors_per_workgroup) *vectors_per_workgroup = p.r.c.vpw;
  if (frames) *frames = fr;
  if (rows_per_chunk) *rows_per_chunk = p.chunk;
  if (analysis_ws_bytes) *analysis_ws_bytes = p.r.bytes;
  if (synthesis_ws_bytes) *synthesis_ws_bytes = p.syn_bytes;
  return p.r.c.path;
}

int64_t cplxamd_stft_src(const cplxamd_stft_desc* d, int64_t frame, int64_t j) {
  if (!d || d->hop < 1 || d->n_fft < 1 || d->length < 1 || d->pad < 0 || frame < 0 || frame >= d->frames || j < 0 ||
      j >= d->n_fft || (d->pad_mode != CPLXAMD_STFT_PAD_ZERO && d->pad_mode != CPLXAMD_STFT_PAD_REFLECT) ||
      (d->pad_mode == CPLXAMD_STFT_PAD_REFLECT && d->pad >= d->length))
    return -2;
  return stft_src(frame * d->hop + j, d->length, d->pad, d->pad_mode);
}

int cplxamd_stft_fold(const cplxamd_stft_desc* d, int64_t t, int64_t* positions) {
  if (!d || !positions || d->length < 1 || d->pad < 0 || t < 0 || t >= d->length ||
      (d->pad_mode != CPLXAMD_STFT_PAD_ZERO && d->pad_mode != CPLXAMD_STFT_PAD_REFLECT) ||
      (d->pad_mode == CPLXAMD_STFT_PAD_REFLECT && d->pad >= d->length))
    return CPLXAMD_EINVAL;
  int64_t p[3];
  const int c = stft_fold(t, d->length, d->pad, d->pad_mode, p);
  for (int a = 0; a < c; ++a) positions[a] = p[a];
  return c;
}

int cplxamd_stft(const void* x, void* y_r, void* y_i, const cplxamd_stft_desc* d, int dtype, void* ws, int64_t ws_bytes,
                 void* stream) {
  if (!x || !y_r || !y_i || !d || !ws) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (const int e = stft_check(*d, true)) return e;
  if (d->envelope) return CPLXAMD_EINVAL;
  StftPlan p;
  const bool full = (d->flags & CPLXAMD_STFT_FULL) != 0;
  if (const int e = stft_plan_for(d->n_fft, d->frames, d->rows, d->length, dtype, full, p)) return e;
  if (ws_bytes < p.r.bytes) return CPLXAMD_EWS;
  if (d->rows == 0 || d->frames == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (full) return stft_full_analysis(x, d->sig_imag, y_r, y_i, *d, dtype, p.r.c, w, st);
  if (dtype == CPLXAMD_F64) return stft_analysis_t<double, double>(x, y_r, y_i, *d, p.r, w, st);
  if (dtype == CPLXAMD_BF16) return stft_analysis_t<bf16_t, float>(x, y_r, y_i, *d, p.r, w, st);
  return stft_analysis_t<float, float>(x, y_r, y_i, *d, p.r, w, st);
}

int cplxamd_istft(const void* x_r, const void* x_i, void* y, const cplxamd_stft_desc* d, int dtype, void* ws, int64_t ws_bytes,
                  void* stream) {
  if (!x_r || !x_i || !y || !d || !ws) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (const int e = stft_check(*d, false)) return e;
  StftPlan p;
  const bool full = (d->flags & CPLXAMD_STFT_FULL) != 0;
  if (const int e = stft_plan_for(d->n_fft, d->frames, d->rows, d->length, dtype, full, p)) return e;
  if (ws_bytes < p.syn_bytes) return CPLXAMD_EWS;
  if (d->rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (dtype == CPLXAMD_F64) return synthesis_t<double, double>(x_r, x_i, y, *d, dtype, p, w, st);
  if (dtype == CPLXAMD_BF16) return synthesis_t<bf16_t, float>(x_r, x_i, y, *d, dtype, p, w, st);
  return synthesis_t<float, float>(x_r, x_i, y, *d, dtype, p, w, st);
}

}  // extern "C"
