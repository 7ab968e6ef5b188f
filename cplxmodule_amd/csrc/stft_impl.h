// Short-time Fourier transforms on the real-transform kernels of rfft_impl.h (one-sided spectra of real signals) and the
// complex kernels of fft_impl.h (full spectra): the index maps, the loader / store policies, the overlap-add pass and the
// launchers of both directions.  stft.hip describes them; compiled in four translation units, one per direction and
// kernel family (stft.hip: one-sided analysis; stft_c2r.hip, stft_c2c.hip, stft_c2c_inv.hip: the other transforms).
#pragma once
#include "fft_impl.h"
#include "rfft_impl.h"

namespace cplxamd {
namespace sp {

// ---- the index maps: the same code on the host (cplxamd_stft_src / _fold, the host tests) and in the kernels ------------
// Sample index of position q of the virtually padded signal (`pad` virtual samples, then `len` samples, then `pad`
// virtual samples), or -1 for "zero".  CPLXAMD_STFT_PAD_ZERO: every virtual sample is a zero; _REFLECT (pad < len):
// the signal mirrored about its first and its last sample.
__host__ __device__ __forceinline__ int64_t stft_src(int64_t q, int64_t len, int64_t pad, int mode) {
  if (q < 0 || q >= len + 2 * pad) return -1;
  int64_t i = q - pad;
  if (mode == CPLXAMD_STFT_PAD_REFLECT) {
    if (i < 0) i = -i;
    else if (i >= len) i = 2 * (len - 1) - i;
  }
  return i >= 0 && i < len ? i : -1;
}

// The padded positions that stft_src maps to sample t, ascending, into p[3]; returns how many (1 .. 3: pad < len).
__host__ __device__ __forceinline__ int stft_fold(int64_t t, int64_t len, int64_t pad, int mode, int64_t (&p)[3]) {
  int c = 0;
  if (mode == CPLXAMD_STFT_PAD_REFLECT && t >= 1 && t <= pad) p[c++] = pad - t;
  p[c++] = pad + t;
  if (mode == CPLXAMD_STFT_PAD_REFLECT && t <= len - 2 && t >= len - 1 - pad) p[c++] = pad + 2 * (len - 1) - t;
  return c;
}

// ---- policies of RIo ------------------------------------------------------------------------------------------------------
// Analysis: the batch's x offsets are virtual, xo = (row << shift) + frame * hop with (frames - 1) hop + n_fft <= 2^shift,
// so row and frame come from the batch decomposition of the vector, whichever rows a packed workgroup spans, and an
// element load splits them again with a shift and a mask (no division).
inline int stft_shift(int64_t vlen) { return 64 - __builtin_clzll((unsigned long long)(vlen > 1 ? vlen : 1)); }

template <typename TI, typename T>
struct StftIn {
  static constexpr bool kFramed = true, kWindowed = false;
  const T* w;
  int64_t len, pad, rs, es;                               // rs, es: row and sample strides of the signal, in elements
  int shift, mode;
  __device__ __forceinline__ int64_t at(int64_t xo, int64_t j) const {   // element offset of the sample, -1 for "zero"
    const int64_t i = stft_src((xo & ((1ll << shift) - 1)) + j, len, pad, mode);
    return i < 0 ? -1 : (xo >> shift) * rs + i * es;
  }
  __device__ __forceinline__ T load(const TI* x, int64_t xo, int64_t j) const {
    const int64_t o = at(xo, j);
    return o < 0 ? (T)0 : w[j] * (T)ld<TI>::at(x + o);
  }
  // the complex loader: a null xi is a plane of zeros that is never read
  __device__ __forceinline__ C2<T> load2(const TI* xr, const TI* xi, int64_t xo, int64_t j) const {
    const int64_t o = at(xo, j);
    if (o < 0) return {0, 0};
    return {w[j] * (T)ld<TI>::at(xr + o), xi ? w[j] * (T)ld<TI>::at(xi + o) : (T)0};
  }
};

// Synthesis: the window in the store of the outputs (real: C2R; both planes: inverse C2C).
template <typename T>
struct StftOut {
  static constexpr bool kFramed = false, kWindowed = true;
  const T* w;
  __device__ __forceinline__ T win(int64_t j) const { return w[j]; }
};

// ---- the overlap-add pass ---------------------------------------------------------------------------------------------
// env[t] = sum_{f ascending} w^2[t + pad - f hop] (0 where no frame covers t + pad), e[t] = 1 / env[t] (0 there)
template <typename T>
__global__ __launch_bounds__(kET) void stft_envelope(const T* w, int64_t n, int64_t hop, int64_t frames, int64_t pad,
                                                    int64_t len, T* env, T* e) {
  for (int64_t t = (int64_t)blockIdx.x * kET + threadIdx.x; t < len; t += (int64_t)gridDim.x * kET) {
    const int64_t p = t + pad;
    int64_t f = p >= n ? (p - n) / hop + 1 : 0;
    const int64_t f1 = p / hop < frames - 1 ? p / hop : frames - 1;
    const bool covered = f <= f1;
    T s = 0;
    for (; f <= f1; ++f) s += w[p - f * hop] * w[p - f * hop];
    env[t] = s;
    e[t] = covered ? (T)1 / s : (T)0;
  }
}

// *out = min |env[t]| over t < count (count >= 1), by one workgroup: a minimum does not depend on the order
template <typename T>
__global__ __launch_bounds__(kET) void stft_env_min(const T* env, int64_t count, T* out) {
  __shared__ T part[kET];
  T m = fabs(env[0]);
  for (int64_t t = threadIdx.x; t < count; t += kET) m = fmin(m, fabs(env[t]));
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = kET / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmin(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = part[0];
}

// y[row][t] = e[t] * sum_{p in fold(t), ascending} sum_{f ascending, 0 <= p - f hop < n} F[row][f][p - f hop], rounded once
template <typename TO, typename T>
__global__ __launch_bounds__(kET) void stft_overlap_add(const T* F, int64_t rows, int64_t n, int64_t hop, int64_t frames,
                                                       int64_t pad, int mode, int64_t len, const T* e, TO* y, int64_t yrs,
                                                       int64_t yes) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < rows * len; i += (int64_t)gridDim.x * kET) {
    const int64_t row = i / len, t = i - row * len;
    const T* Fr = F + row * frames * n;
    int64_t ps[3];
    const int c = stft_fold(t, len, pad, mode, ps);
    T acc = 0;
    for (int a = 0; a < c; ++a) {
      const int64_t p = ps[a];
      int64_t f = p >= n ? (p - n) / hop + 1 : 0;
      const int64_t f1 = p / hop < frames - 1 ? p / hop : frames - 1;
      for (; f <= f1; ++f) acc += Fr[f * n + p - f * hop];
    }
    st_t(y + row * yrs + t * yes, e ? e[t] * acc : acc);
  }
}

// ---- plan -------------------------------------------------------------------------------------------------------------
struct StftPlan {
  RfftPlan r;                                             // of the analysis: rows * frames vectors
  RfftPlan c;                                             // of the synthesis transform: chunk * frames vectors, every chunk
  int64_t chunk;                                          // rows per synthesis chunk
  int64_t off_env, off_F, off_Fi, syn_bytes;              // synthesis: [transform of a chunk | env | F (full: | F imag)]
};

// the plan of the transform itself: the half-length / odd real plan, or (full) the complex plan in the same struct
inline int stft_fft_plan(int64_t n, int64_t vectors, int dtype, bool full, RfftPlan& p) {
  if (!full) return rfft_plan_for(n, vectors, dtype, p);
  if (const int e = fft_plan_for(n, vectors, dtype, p.c)) return e;
  p.half = false;
  p.L = n;
  p.off_rt = p.bytes = p.c.bytes;
  return 0;
}

inline int stft_plan_for(int64_t n, int64_t frames, int64_t rows, int64_t len, int dtype, bool full, StftPlan& p) {
  if (frames < 0 || rows < 0 || len < 0 || frames > 0x7fffffffll) return CPLXAMD_EINVAL;
  int64_t vectors;
  if (__builtin_mul_overflow(rows, frames, &vectors)) return CPLXAMD_ESHAPE;
  if (const int e = stft_fft_plan(n, vectors, dtype, full, p.r)) return e;
  const int64_t cs = dtype == CPLXAMD_F64 ? 8 : 4;
  const int64_t row_bytes = (frames > 0 ? frames : 1) * n * cs * (full ? 2 : 1);
  int64_t chunk = kLargeWs / row_bytes;                   // the cap of the four-step and Welch buffers; a row takes its own
  if (chunk < 1) chunk = 1;
  if (chunk > rows) chunk = rows > 0 ? rows : 1;
  p.chunk = chunk;
  if (const int e = stft_fft_plan(n, chunk * frames, dtype, full, p.c)) return e;
  p.off_env = p.c.bytes;
  p.off_F = p.off_env + al256((len > 0 ? len : 1) * cs);
  p.off_Fi = p.off_F + (full ? al256(chunk * row_bytes / 2) : 0);
  p.syn_bytes = p.off_F + (full ? 2 * al256(chunk * row_bytes / 2) : al256(chunk * row_bytes));
  return 0;
}

// every field of a descriptor that both directions read; `analysis`: the signal is the input (any stride >= 0)
inline int stft_check(const cplxamd_stft_desc& d, bool analysis) {
  if (d.n_fft < 1 || d.n_fft > CPLXAMD_WELCH_MAX_N || d.hop < 1 || d.hop > (1ll << 40) || d.frames < 0 ||
      d.frames > 0x7fffffffll || d.length < 1 || d.length > (1ll << 48) || d.pad < 0 || d.pad > CPLXAMD_WELCH_MAX_N ||
      d.rows < 0 || !d.window || !(d.scale - d.scale == 0) ||
      (d.flags & ~(CPLXAMD_FFT_INVERSE | CPLXAMD_RFFT_WEIGHTED | CPLXAMD_STFT_FULL)))
    return CPLXAMD_EINVAL;
  // a full spectrum has no Hermitian weights; only a full spectrum has an imaginary signal plane
  if ((d.flags & CPLXAMD_STFT_FULL) ? (d.flags & CPLXAMD_RFFT_WEIGHTED) != 0 : d.sig_imag != nullptr) return CPLXAMD_EINVAL;
  if (d.pad_mode != CPLXAMD_STFT_PAD_ZERO && d.pad_mode != CPLXAMD_STFT_PAD_REFLECT) return CPLXAMD_EINVAL;
  if (d.pad_mode == CPLXAMD_STFT_PAD_REFLECT && d.pad >= d.length) return CPLXAMD_EINVAL;
  if (analysis ? (d.sig_es < 0 || d.sig_row_stride < 0 || d.spec_es < 1 || d.spec_frame_stride < 1 || d.spec_row_stride < 0)
               : (d.sig_es < 1 || d.sig_row_stride < 0 || d.spec_es < 0 || d.spec_frame_stride < 0 || d.spec_row_stride < 0))
    return CPLXAMD_EINVAL;
  int64_t vectors, span = 1, all;
  if (__builtin_mul_overflow(d.rows, d.frames, &vectors) || vectors > 0x7fffffffll) return CPLXAMD_ESHAPE;
  // the virtual offsets (row << stft_shift(span)) + frame * hop + j are 64-bit
  if (d.frames > 0 && (__builtin_mul_overflow(d.frames - 1, d.hop, &span) || __builtin_add_overflow(span, d.n_fft, &span)))
    return CPLXAMD_ESHAPE;
  if (stft_shift(span) > 62 || d.rows > (INT64_MAX >> stft_shift(span))) return CPLXAMD_ESHAPE;
  if (__builtin_mul_overflow(d.rows, d.length, &all)) return CPLXAMD_ESHAPE;       // the gather pass indexes rows * length
  return 0;
}

// `synthesis`: spectrogram in, frames out (C2R, or for a full spectrum C2C)
inline cplxamd_fft_desc stft_fft_desc(const cplxamd_stft_desc& d, bool synthesis) {
  const bool full = (d.flags & CPLXAMD_STFT_FULL) != 0;
  cplxamd_fft_desc f{};
  f.n = d.n_fft;
  f.n_in = synthesis && !full ? d.n_fft / 2 + 1 : d.n_fft;
  f.x_es = synthesis ? d.spec_es : d.sig_es;
  f.y_es = synthesis ? 1 : d.spec_es;
  f.inverse = full ? (d.flags & CPLXAMD_FFT_INVERSE)
                   : (d.flags & (CPLXAMD_FFT_INVERSE | CPLXAMD_RFFT_WEIGHTED)) | (synthesis ? CPLXAMD_RFFT_C2R : 0);
  f.scale = d.scale;
  return f;
}

// ---- analysis ---------------------------------------------------------------------------------------------------------
// the batch (runs 0 and 2: rows, frames) and the loader policy of an analysis
template <typename TI, typename T>
StftIn<TI, T> stft_in(const cplxamd_stft_desc& d, Batch& b) {
  const int shift = stft_shift((d.frames - 1) * d.hop + d.n_fft);
  b = Batch{d.rows * d.frames, 1, d.frames, {1ll << shift, 0, d.hop}, {d.spec_row_stride, 0, d.spec_frame_stride}};
  return StftIn<TI, T>{(const T*)d.window, d.length, d.pad, d.sig_row_stride, d.sig_es, shift, d.pad_mode};
}

template <typename TI, typename T>
int stft_analysis_t(const void* x, void* yr, void* yi, const cplxamd_stft_desc& d, const RfftPlan& p, char* ws, hipStream_t st) {
  Batch b;
  const StftIn<TI, T> pol = stft_in<TI, T>(d, b);
  return rfft_t<TI, TI, T, false>(x, nullptr, yr, yi, stft_fft_desc(d, false), b, p, ws, st, pol);
}

// the full spectrum (C2C; a null xi is a plane of zeros): a translation unit of its own
template <typename TI, typename T>
int stft_full_analysis_t(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_stft_desc& d, const FftPlan& p,
                         char* ws, hipStream_t st) {
  Batch b;
  const StftIn<TI, T> pol = stft_in<TI, T>(d, b);
  return fft_t<TI, TI, T>(xr, xi, yr, yi, stft_fft_desc(d, false), b, p, ws, st, pol);
}
int stft_full_analysis(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_stft_desc& d, int dtype,
                       const FftPlan& p, char* ws, hipStream_t st);             // stft_c2c.hip

// ---- synthesis --------------------------------------------------------------------------------------------------------
// the transform of rows [r0, r0 + nr) into F, windowed: one translation unit of its own
template <typename TI, typename T>
int stft_frames_t(const void* xr, const void* xi, T* F, const cplxamd_stft_desc& d, int64_t r0, int64_t nr, const RfftPlan& p,
                  char* ws, hipStream_t st, bool build) {
  const Batch b{nr * d.frames, 1, d.frames, {d.spec_row_stride, 0, d.spec_frame_stride}, {d.frames * d.n_fft, 0, d.n_fft}};
  const StftOut<T> pol{(const T*)d.window};
  const TI* pr = (const TI*)xr + r0 * d.spec_row_stride;
  const TI* pi = (const TI*)xi + r0 * d.spec_row_stride;
  return rfft_t<TI, T, T, true>(pr, pi, F, nullptr, stft_fft_desc(d, true), b, p, ws, st, pol, build);
}
// `build`: the first chunk of a call writes the tables, the others find them
int stft_frames(const void* xr, const void* xi, void* F, const cplxamd_stft_desc& d, int64_t r0, int64_t nr, int in_dtype,
                const RfftPlan& p, char* ws, hipStream_t st, bool build);       // stft_c2r.hip

// the full spectrum: inverse (or forward) C2C into the two frame planes Fr, Fi, windowed
template <typename TI, typename T>
int stft_full_frames_t(const void* xr, const void* xi, T* Fr, T* Fi, const cplxamd_stft_desc& d, int64_t r0, int64_t nr,
                       const FftPlan& p, char* ws, hipStream_t st, bool build) {
  const Batch b{nr * d.frames, 1, d.frames, {d.spec_row_stride, 0, d.spec_frame_stride}, {d.frames * d.n_fft, 0, d.n_fft}};
  const StftOut<T> pol{(const T*)d.window};
  const TI* pr = (const TI*)xr + r0 * d.spec_row_stride;
  const TI* pi = (const TI*)xi + r0 * d.spec_row_stride;
  return fft_t<TI, T, T>(pr, pi, Fr, Fi, stft_fft_desc(d, true), b, p, ws, st, pol, build);
}
int stft_full_frames(const void* xr, const void* xi, void* Fr, void* Fi, const cplxamd_stft_desc& d, int64_t r0, int64_t nr,
                     int in_dtype, const FftPlan& p, char* ws, hipStream_t st, bool build);   // stft_c2c_inv.hip

}  // namespace sp
}  // namespace cplxamd
