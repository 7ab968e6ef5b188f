// Welch power spectra (cplxmodule/utils/spectrum.py:7-82 pwelch) on one power-of-two FFT engine, forward and gradient.
//
// The reference spells Welch's method as window_view -> * window -> torch.fft.fft -> abs^2 -> mean: the whole
// [rows, segments, n] windowed block and its spectrum go through memory several times.  Here one launch reads every
// segment straight from x (two plane pointers + element strides: interleaved complex and planar Cplx alike), windows,
// transforms and accumulates |X_k|^2 over a chunk of segments in registers; a second small launch adds the chunks in a
// fixed order, scales and writes [rows, n].  No atomics anywhere: repeated runs give the same bits.
//
// Engine (fft_run): a Stockham FFT of a power-of-two length L <= 2^kLogLMax (16384 float32 / 8192 float64 points, 136
// KiB of LDS either way) held by one workgroup, compiled per length: every stage, stride and thread count is a
// compile-time constant, and each kernel's launch bound is the thread count it is launched with (kNT: 8 values per
// thread up to 4096 points, 16 at 8192, 32 at 16384; at most 512 threads).  Radix-8 butterflies (one leading radix-2 / 4
// stage when 3 does not divide log2 L) run in registers; between stages the values make one LDS round trip, planes
// padded by one word per 16 (pad()), so the strided writes of the first stages spread over the banks.  Twiddles come
// from a table in the caller's workspace (tables), so a butterfly costs loads, not sincos.  The first stage reads from
// its loader (global memory, or LDS), the last stage's outputs stay in registers at k = j + r L / R (out_k): the
// consumer squares / multiplies them in place.  No kernel uses scratch (-Rpass-analysis=kernel-resource-usage).
//
// Size classes (welch_path):
//   DIRECT               n a power of two within the LDS limit: welch_lds<.., false, log2 n>, one launch.
//   BLUESTEIN            other n with M = 2^ceil(log2(2n - 1)) within it: the chirp-z transform in the same launch,
//                        X_k = e^{-i pi k^2 / n} IFFT_M(FFT_M(a) . B)_k,  a_j = x_j w_j e^{-i pi j^2 / n} (j < n),
//                        B = FFT_M(b) with b_m = e^{+i pi m^2 / n} / M for |m| < n (built per call in the workspace; the
//                        1 / M of the convolution rides on it, so no intermediate grows by M).  |X_k|^2 needs no chirp.
//   FOURSTEP             n = 2^k above the limit: batches of segments through the workspace, N = N1 N2: a column pass
//                        (FFT over n1 of x[n1 N2 + n2], twiddle e^{-2 pi i n2 k1 / N}) and a row pass (FFT over n2) that
//                        writes X[k1 + N1 k2] in natural order, both on fft_run.
//   BLUESTEIN_FOURSTEP   the chirp-z transform with M above the limit: the FFTs of length M go through the four-step passes.
// Every twiddle comes from an exactly reduced integer argument q / m (q = k j mod m, chirps j^2 mod 2n in 64-bit
// integers) through sincospi, accurate to about one ulp, once per call into the workspace tables (twiddles e^{-2 pi i q /
// M}, chirp e^{-i pi j^2 / n}): no large-argument __sinf-class intrinsics, no state in the library.
//
// Gradient (welch_bwd):  P_k = c sum_s |X_{s,k}|^2,  c = 1 / (S scale).  With autograd's convention for complex inputs
// (the gradient of the real pair (re, im), i.e. dL/dre + i dL/dim, which is also what each plane of a Cplx receives),
//     dx[s step + j] += 2 c w_j sum_k g_k X_{s,k} e^{+2 pi i j k / n} = 2 c w_j n IFFT(g . X_s)[j]
// -- no conjugation of X.  X_s is recomputed, each segment's term goes to the workspace D[row][s][j], and a gather adds
// the segments that cover each sample in ascending s.  Bluestein: the inverse DFT of length n is a second chirp-z
// transform with conj(B) (b is even, so FFT(conj b) = conj B); the chirps between the two cancel.
#include "common.h"
#include "launch.h"

#include <type_traits>

namespace cplxamd {
namespace sp {

template <typename T> struct C2 { T re, im; };

template <typename T> constexpr int kLogLMax = sizeof(T) == 4 ? 14 : 13;   // 16384 float32 / 8192 float64 points in LDS
constexpr int kLogFusedMax = 13;    // the Bluestein pair and the backward in one workgroup: up to 8192 points
// complex values per thread and threads of a length-2^LOGL transform: 8 per thread up to 2^12 (at most 512 threads),
// then 16 (2^13) and 32 (2^14), so no workgroup exceeds 512 threads and every kernel has the 256-VGPR budget of
// __launch_bounds__(512) or more: at 1024 threads the 128-VGPR cap made the fused kernels spill to scratch
template <int LOGL> constexpr int kEOf = LOGL >= 14 ? 32 : LOGL == 13 ? 16 : 8;
template <int LOGL> constexpr int kNT = (1 << LOGL) / kEOf<LOGL> > 0 ? (1 << LOGL) / kEOf<LOGL> : 1;
constexpr int64_t kLargeWs = 256ll << 20;                // four-step batch buffers
constexpr int kTargetWgs = 2048;                          // workgroups of a fused launch (segments split to reach it)
constexpr int kET = 256;                                  // elementwise kernels

__host__ __device__ constexpr int pad(int i) { return i + (i >> 4); }
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ void sincospi_t(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void sincospi_t(double x, double* s, double* c) { sincospi(x, s, c); }

// e^{sg 2 pi i q / m}, q reduced exactly into (-m/2, m/2] before the one rounding of 2q / m
template <typename T>
__device__ __forceinline__ C2<T> cis(T sg, int64_t q, int64_t m) {
  q %= m;
  if (q < 0) q += m;
  if (2 * q > m) q -= m;
  T s, c;
  sincospi_t((T)(2 * q) / (T)m, &s, &c);
  return {c, sg * s};
}
template <typename T> __device__ __forceinline__ C2<T> cmul(C2<T> a, C2<T> b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T> __device__ __forceinline__ C2<T> cmulc(C2<T> a, C2<T> b) {   // a conj(b)
  return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}

// cos / sin (2 pi k / 16)
__device__ constexpr double c16(int k) {
  switch (k & 15) {
    case 0: return 1.0; case 1: return 0.92387953251128673848; case 2: return 0.70710678118654752440;
    case 3: return 0.38268343236508977173; case 4: return 0.0; case 5: return -0.38268343236508977173;
    case 6: return -0.70710678118654752440; case 7: return -0.92387953251128673848; case 8: return -1.0;
    case 9: return -0.92387953251128673848; case 10: return -0.70710678118654752440;
    case 11: return -0.38268343236508977173; case 12: return 0.0; case 13: return 0.38268343236508977173;
    case 14: return 0.70710678118654752440; default: return 0.92387953251128673848;
  }
}
__device__ constexpr double s16(int k) { return c16(k - 4); }
template <int LR> __device__ constexpr int brev(int i) {
  int r = 0;
  for (int b = 0; b < LR; ++b) r |= ((i >> b) & 1) << (LR - 1 - b);
  return r;
}

// R-point DFT of v[0..R), natural order in and out, sign sg (-1 forward), twiddles as constants
template <typename T, int R>
__device__ __forceinline__ void dft(C2<T>* v, T sg) {
  constexpr int LR = R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : 4;
  C2<T> w[R];
#pragma unroll
  for (int i = 0; i < R; ++i) w[i] = v[brev<LR>(i)];
#pragma unroll
  for (int h = 1; h < R; h *= 2) {
#pragma unroll
    for (int k = 0; k < h; ++k) {
      const int q = k * (8 / h);                         // e^{sg 2 pi i k / 2h} = e^{sg 2 pi i q / 16}
#pragma unroll
      for (int i = k; i < R; i += 2 * h) {
        const C2<T> a = w[i];
        C2<T> b = w[i + h];
        if (q == 4) b = {-sg * b.im, sg * b.re};
        else if (q != 0) b = cmul(b, C2<T>{(T)c16(q), sg * (T)s16(q)});
        w[i] = {a.re + b.re, a.im + b.im};
        w[i + h] = {a.re - b.re, a.im - b.im};
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) v[i] = w[i];
}

// the twiddle table of the call: tw[q] = e^{-2 pi i q / 2^ltw}, q in [0, 2^ltw) (tables); sg > 0 conjugates
template <typename T>
__device__ __forceinline__ C2<T> twid(const C2<T>* tw, int64_t q, T sg) {
  const C2<T> a = tw[q];
  return {a.re, sg < 0 ? a.im : -a.im};
}

// One Stockham stage of radix R on a length-L transform whose previous stages had span NS (all compile-time): thread t
// owns butterflies j = t + b NT, b < E / R; elements j + r L / R in, (j / NS) NS R + j % NS + r NS out.  The first stage
// reads its loader, the others LDS; the last keeps its outputs in registers.  tsh: log2 of the table size over NS R.
template <typename T, int E, int NT, int L, int R, int NS, bool FIRST, bool LAST, typename Load>
__device__ __forceinline__ void stage(C2<T> (&v)[E], T* sre, T* sim, int t, T sg, const C2<T>* tw, int tsh, Load& load) {
  constexpr int NB = L / R;
#pragma unroll
  for (int b = 0; b < E / R; ++b) {
    const int j = t + b * NT;
    if (j < NB) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int p = j + r * NB;
        if constexpr (FIRST) v[b * R + r] = load(p);
        else v[b * R + r] = C2<T>{sre[pad(p)], sim[pad(p)]};
      }
      if constexpr (NS > 1) {
        const int jm = j & (NS - 1);
#pragma unroll
        for (int r = 1; r < R; ++r) v[b * R + r] = cmul(v[b * R + r], twid(tw, (int64_t)(jm * r) << tsh, sg));
      }
      dft<T, R>(&v[b * R], sg);
    }
  }
  if constexpr (!LAST) {
    __syncthreads();
#pragma unroll
    for (int b = 0; b < E / R; ++b) {
      const int j = t + b * NT;
      if (j < NB) {
        const int o = (j / NS) * NS * R + (j & (NS - 1));
#pragma unroll
        for (int r = 0; r < R; ++r) {
          sre[pad(o + r * NS)] = v[b * R + r].re;
          sim[pad(o + r * NS)] = v[b * R + r].im;
        }
      }
    }
    __syncthreads();
  }
}

// radix plan of a length 2^LOGL: one leading radix-2 / 4 / 8 stage, then radix 8
template <int LOGL> constexpr int kLead = LOGL % 3 == 0 ? 3 : LOGL % 3;
template <int LOGL> constexpr int kLastLR = LOGL == 0 ? 0 : (LOGL == kLead<LOGL> ? kLead<LOGL> : 3);

// FFT of length 2^LOGL (sg -1 forward, +1 unnormalised inverse) by one workgroup of kNT<LOGL> threads; the input comes
// from load(p), p in [0, L), the result stays in v laid out as out_k describes.  Callers sync before the loader reads
// LDS that the stages overwrite.  ltw: log2 of the twiddle table's size.
template <typename T, int LOGL, int DONE = 0, typename Load>
__device__ __forceinline__ void fft_run(C2<T> (&v)[kEOf<LOGL>], T* sre, T* sim, int t, T sg, const C2<T>* tw, int ltw,
                                        Load& load) {
  if constexpr (LOGL == 0) {
    if (t == 0) v[0] = load(0);
  } else {
    constexpr int LR = DONE == 0 ? kLead<LOGL> : 3;
    stage<T, kEOf<LOGL>, kNT<LOGL>, (1 << LOGL), (1 << LR), (1 << DONE), DONE == 0, DONE + LR == LOGL>(
        v, sre, sim, t, sg, tw, ltw - (DONE + LR), load);
    if constexpr (DONE + LR < LOGL) fft_run<T, LOGL, DONE + LR>(v, sre, sim, t, sg, tw, ltw, load);
  }
}

// where fft_run's result lives: v[b R + r] holds k = j + r NB, j = t + b NT (R the last stage's radix); false if none
template <int LOGL>
__device__ __forceinline__ bool out_k(int e, int t, int& k) {
  constexpr int LR = kLastLR<LOGL>, NB = (1 << LOGL) >> LR;
  const int j = t + (e >> LR) * kNT<LOGL>;
  k = j + (e & ((1 << LR) - 1)) * NB;
  return j < NB;
}

// the result back to LDS in natural order (for a second transform on the same data)
template <typename T, int LOGL>
__device__ __forceinline__ void to_lds(const C2<T> (&v)[kEOf<LOGL>], T* sre, T* sim, int t) {
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kEOf<LOGL>; ++e) {
    int k;
    if (out_k<LOGL>(e, t, k)) {
      sre[pad(k)] = v[e].re;
      sim[pad(k)] = v[e].im;
    }
  }
  __syncthreads();
}

template <typename TI> struct ld;
template <> struct ld<float> { static __device__ __forceinline__ float at(const float* p) { return *p; } };
template <> struct ld<double> { static __device__ __forceinline__ double at(const double* p) { return *p; } };
template <> struct ld<bf16_t> { static __device__ __forceinline__ float at(const bf16_t* p) { return bf16_to_f32(*p); } };
__device__ __forceinline__ void st_t(float* p, float v) { *p = v; }
__device__ __forceinline__ void st_t(double* p, double v) { *p = v; }
__device__ __forceinline__ void st_t(bf16_t* p, float v) { *p = f32_to_bf16(v); }

// Welch segment source: x[row][s step + p] w[p] (times the chirp e^{-i pi p^2 / n} for Bluestein), 0 for p >= n
template <typename TI, typename T>
struct Seg {
  const TI* xr; const TI* xi; int64_t xes; const T* w; int64_t n; const C2<T>* chirp;   // chirp NULL: direct
  __device__ __forceinline__ C2<T> at(int64_t base, int64_t p) const {
    if (p >= n) return {0, 0};
    const int64_t o = base + p * xes;
    const T wp = w[p];
    C2<T> a{(T)ld<TI>::at(xr + o) * wp, (T)ld<TI>::at(xi + o) * wp};
    if (chirp) a = cmul(a, chirp[p]);
    return a;
  }
};

// ---- fused forward: one workgroup = one chunk of G segments of one row -----------------------------------------------
// Bluestein: B-hat carries the 1 / M of the convolution, so c_k = X_k chirp+_k keeps the magnitude of X.
template <typename TI, typename T, bool BLUE, int LOGM>
__global__ __launch_bounds__(kNT<LOGM>) void welch_lds(Seg<TI, T> src, int64_t xrs, int64_t step, int64_t S, int64_t G,
                                                      int64_t chunks, const C2<T>* tw, const C2<T>* bhat, T* part) {
  constexpr int E = kEOf<LOGM>, M = 1 << LOGM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sre = (T*)smem;
  T* sim = sre + pad(M) + 1;
  __shared__ int zero;
  if (threadIdx.x == 0) zero = 0;
  __syncthreads();
  const volatile int* s_zero = &zero;
  int t = threadIdx.x;
  const int64_t row = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int64_t s0 = ch * G, s1 = s0 + G < S ? s0 + G : S;
  auto from_lds = [&](int p) { return C2<T>{sre[pad(p)], sim[pad(p)]}; };
  T acc[E];
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    acc[e] = 0;
    v[e] = {0, 0};
  }
  for (int64_t s = s0; s < s1; ++s) {
    // t through a volatile LDS read per segment: the compiler may not hoist the addresses of every stage out of this
    // loop (at 8192 / 16384 points those hoisted addresses overflowed the register file into scratch)
    const int t = threadIdx.x + *s_zero;
    const int64_t base = row * xrs + s * step * src.xes;
    auto seg = [&](int p) { return src.at(base, p); };
    fft_run<T, LOGM>(v, sre, sim, t, (T)-1, tw, LOGM, seg);
    if constexpr (BLUE) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGM>(e, t, k)) v[e] = cmul(v[e], bhat[k]);
      }
      to_lds<T, LOGM>(v, sre, sim, t);
      fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += v[e].re * v[e].re + v[e].im * v[e].im;
    if constexpr (BLUE) __syncthreads();                 // the next segment's first stage writes LDS read here
  }
  T* out = part + (row * chunks + ch) * src.n;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGM>(e, t, k) && k < src.n) out[k] = acc[e];
  }
}

// ---- fused backward: D[row][s][j] = w_j y_j, y the unnormalised inverse transform of g . X_s -------------------------
template <typename TI, typename T, bool BLUE, int LOGM>
__global__ __launch_bounds__(kNT<LOGM>) void welch_bwd_lds(Seg<TI, T> src, int64_t xrs, int64_t step, int64_t S,
                                                          int64_t G, int64_t chunks, const C2<T>* tw, const C2<T>* bhat,
                                                          const T* g, C2<T>* D) {
  constexpr int E = kEOf<LOGM>, M = 1 << LOGM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sre = (T*)smem;
  T* sim = sre + pad(M) + 1;
  __shared__ int zero;
  if (threadIdx.x == 0) zero = 0;
  __syncthreads();
  const volatile int* s_zero = &zero;
  const int64_t n = src.n;
  const int64_t row = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int64_t s0 = ch * G, s1 = s0 + G < S ? s0 + G : S;
  const T* gr = g + row * n;
  auto from_lds = [&](int p) { return C2<T>{sre[pad(p)], sim[pad(p)]}; };
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = {0, 0};
  for (int64_t s = s0; s < s1; ++s) {
    // t through a volatile LDS read per segment: the compiler may not hoist the addresses of every stage out of this
    // loop (at 8192 / 16384 points those hoisted addresses overflowed the register file into scratch)
    const int t = threadIdx.x + *s_zero;
    const int64_t base = row * xrs + s * step * src.xes;
    auto seg = [&](int p) { return src.at(base, p); };
    fft_run<T, LOGM>(v, sre, sim, t, (T)-1, tw, LOGM, seg);
    if constexpr (BLUE) {                                // c = IFFT(A B-hat): X_k = chirp_k c_k
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGM>(e, t, k)) v[e] = cmul(v[e], bhat[k]);
      }
      to_lds<T, LOGM>(v, sre, sim, t);
      fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {                        // direct: g X;  Bluestein: a'_k = g_k c_k
      int k;
      if (out_k<LOGM>(e, t, k)) {
        const T gk = k < n ? gr[k] : (T)0;
        v[e] = {gk * v[e].re, gk * v[e].im};
      }
    }
    to_lds<T, LOGM>(v, sre, sim, t);
    if constexpr (BLUE) {                                // y_j = chirp+_j IFFT(FFT(a') conj B-hat)_j
      fft_run<T, LOGM>(v, sre, sim, t, (T)-1, tw, LOGM, from_lds);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGM>(e, t, k)) v[e] = cmulc(v[e], bhat[k]);
      }
      to_lds<T, LOGM>(v, sre, sim, t);
    }
    fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
    C2<T>* d = D + (row * S + s) * n;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      int j;
      if (out_k<LOGM>(e, t, j) && j < n) {
        C2<T> y = v[e];
        if constexpr (BLUE) y = cmulc(y, src.chirp[j]);
        const T wj = src.w[j];
        d[j] = {wj * y.re, wj * y.im};
      }
    }
    __syncthreads();                                     // the next segment's first stage writes LDS
  }
}

// ---- one pass of a batched FFT through global memory: vector (b = blockIdx.y, u = blockIdx.x) of length 2^LOGL,
// element p at in[b vs + u in_u + p in_e]; output k at out[b vs + u out_u + k out_e], times e^{sg 2 pi i u k / 2^ltw}
// when `twiddle` (the four-step twiddle) ---------------------------------------------------------------------------------
template <typename T, int LOGL>
__global__ __launch_bounds__(kNT<LOGL>) void fft_pass(const C2<T>* in, C2<T>* out, int64_t vs, int64_t in_u, int64_t in_e,
                                                     int64_t out_u, int64_t out_e, const C2<T>* tw, int ltw, bool twiddle,
                                                     T sg) {
  constexpr int E = kEOf<LOGL>, L = 1 << LOGL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sre = (T*)smem;
  T* sim = sre + pad(L) + 1;
  const int t = threadIdx.x;
  const int64_t u = blockIdx.x, b = blockIdx.y;
  const C2<T>* src = in + b * vs + u * in_u;
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = {0, 0};
  auto load = [&](int p) { return src[p * in_e]; };
  fft_run<T, LOGL>(v, sre, sim, t, sg, tw, ltw, load);
  C2<T>* dst = out + b * vs + u * out_u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGL>(e, t, k)) {
      C2<T> y = v[e];
      if (twiddle) y = cmul(y, twid(tw, u * k, sg));          // u k < N1 N2 = 2^ltw
      dst[k * out_e] = y;
    }
  }
}

// ---- elementwise helpers ---------------------------------------------------------------------------------------------
// Bluestein filter b_m = e^{+i pi m^2 / n} / M for |m| < n (index m mod M), 0 elsewhere: the 1 / M of the cyclic
// convolution IFFT(FFT(a) FFT(b)) / M rides on the filter (exact, M a power of two), so every intermediate keeps the
// magnitude of X
template <typename T>
__global__ __launch_bounds__(kET) void chirp_filter(C2<T>* b, int64_t n, int64_t M) {
  const T inv = (T)1 / (T)M;
  for (int64_t m = (int64_t)blockIdx.x * kET + threadIdx.x; m < M; m += (int64_t)gridDim.x * kET) {
    const int64_t a = m < n ? m : (M - m < n ? M - m : -1);
    const C2<T> c = a < 0 ? C2<T>{0, 0} : cis<T>((T)1, (a * a) % (2 * n), 2 * n);
    b[m] = {c.re * inv, c.im * inv};
  }
}

// tw[q] = e^{-2 pi i q / M};  chirp[j] = e^{-i pi j^2 / n} = e^{-2 pi i (j^2 mod 2n) / 2n}
template <typename T>
__global__ __launch_bounds__(kET) void tables(C2<T>* tw, int64_t M, C2<T>* chirp, int64_t n) {
  for (int64_t q = (int64_t)blockIdx.x * kET + threadIdx.x; q < M; q += (int64_t)gridDim.x * kET) {
    tw[q] = cis<T>((T)-1, q, M);
    if (chirp && q < n) chirp[q] = cis<T>((T)-1, (q * q) % (2 * n), 2 * n);
  }
}

// buf[v][p] = segment (row, s) of global vector index v0 + v, p in [0, M)
template <typename TI, typename T>
__global__ __launch_bounds__(kET) void seg_load(Seg<TI, T> src, int64_t xrs, int64_t step, int64_t S, int64_t v0,
                                                int64_t nv, int64_t M, C2<T>* buf) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * M; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / M, p = i % M, gv = v0 + v;
    buf[i] = src.at((gv / S) * xrs + (gv % S) * step * src.xes, p);
  }
}

// buf[v][k] *= h[k] (conj: conj(h[k])); with g: buf[v][k] = g[row][k] buf[v][k] for k < n, 0 beyond
template <typename T>
__global__ __launch_bounds__(kET) void vec_scale(C2<T>* buf, int64_t nv, int64_t M, const C2<T>* h, bool conj_h,
                                                 const T* g, int64_t n, int64_t S, int64_t v0) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * M; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / M, k = i % M;
    C2<T> y = buf[i];
    if (h) y = conj_h ? cmulc(y, h[k]) : cmul(y, h[k]);
    if (g) {
      const T gk = k < n ? g[((v0 + v) / S) * n + k] : (T)0;
      y = {gk * y.re, gk * y.im};
    }
    buf[i] = y;
  }
}

// P[row][k] += sum over this batch's segments of row (ascending) |buf[v][k]|^2; rows r0 .. r1 of the batch
template <typename T>
__global__ __launch_bounds__(kET) void pow_accum(const C2<T>* buf, int64_t v0, int64_t nv, int64_t S, int64_t M, int64_t n,
                                                 T* P) {
  const int64_t r0 = v0 / S, r1 = (v0 + nv - 1) / S;
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < (r1 - r0 + 1) * n; i += (int64_t)gridDim.x * kET) {
    const int64_t row = r0 + i / n, k = i % n;
    const int64_t a = row * S > v0 ? row * S : v0, e = (row + 1) * S < v0 + nv ? (row + 1) * S : v0 + nv;
    T acc = P[row * n + k];
    for (int64_t gv = a; gv < e; ++gv) {
      const C2<T> y = buf[(gv - v0) * M + k];
      acc += y.re * y.re + y.im * y.im;
    }
    P[row * n + k] = acc;
  }
}

// D[v0 + v][j] = w_j y_j (Bluestein: y_j = chirp+_j buf[v][j]) for j < n
template <typename T>
__global__ __launch_bounds__(kET) void seg_store(const C2<T>* buf, int64_t v0, int64_t nv, int64_t M, int64_t n,
                                                 const T* w, const C2<T>* chirp, C2<T>* D) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * n; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / n, j = i % n;
    C2<T> y = buf[v * M + j];
    if (chirp) y = cmulc(y, chirp[j]);
    D[(v0 + v) * n + j] = {w[j] * y.re, w[j] * y.im};
  }
}

// sc[0] = fs sum w^2 (density) or (sum w)^2 (spectrum): one workgroup, fixed order
template <typename T>
__global__ __launch_bounds__(kET) void win_scale(const T* w, int64_t n, int scaling, double fs, T* sc) {
  __shared__ T red[2][kET];
  T a = 0, b = 0;
  for (int64_t i = threadIdx.x; i < n; i += kET) {
    a += w[i];
    b += w[i] * w[i];
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int h = kET / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sc[0] = scaling == CPLXAMD_WELCH_DENSITY ? (T)fs * red[1][0] : red[0][0] * red[0][0];
}

// out[row][k] = sum_ch part[row][ch][k] (ascending ch) * f / sc[0]
template <typename T>
__global__ __launch_bounds__(kET) void combine(const T* part, int64_t rows, int64_t chunks, int64_t n, T f, const T* sc,
                                               T* out) {
  const T c = f / sc[0];
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < rows * n; i += (int64_t)gridDim.x * kET) {
    const int64_t row = i / n, k = i % n;
    const T* p = part + row * chunks * n + k;
    T acc = 0;
    for (int64_t ch = 0; ch < chunks; ++ch) acc += p[ch * n];
    out[i] = acc * c;
  }
}

// dx[row][m] = f / sc[0] * sum over the segments s covering m (ascending) of D[row][s][m - s step]; 0 where none does
template <typename TO, typename T>
__global__ __launch_bounds__(kET) void gather(const C2<T>* D, int64_t rows, int64_t T_len, int64_t n, int64_t step,
                                              int64_t S, T f, const T* sc, TO* dxr, TO* dxi, int64_t drs, int64_t des) {
  const T c = f / sc[0];
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < rows * T_len; i += (int64_t)gridDim.x * kET) {
    const int64_t row = i / T_len, m = i % T_len;
    const int64_t lo = m >= n ? (m - n) / step + 1 : 0, hi0 = m / step, hi = hi0 < S - 1 ? hi0 : S - 1;
    T ar = 0, ai = 0;
    for (int64_t s = lo; s <= hi; ++s) {
      const C2<T> d = D[(row * S + s) * n + (m - s * step)];
      ar += d.re;
      ai += d.im;
    }
    const int64_t o = row * drs + m * des;
    st_t(dxr + o, ar * c);
    st_t(dxi + o, ai * c);
  }
}

// ---- plan --------------------------------------------------------------------------------------------------------------
struct Plan {
  int path, logM, logN1, logN2;
  bool fwd_fused, bwd_fused;
  int64_t M, chunks, G, GL;             // fused: chunks per row, G segments per chunk; through the workspace: GL vectors
  int64_t off_tw, off_chirp, off_bhat, off_part, off_buf, off_tmp, off_D, fwd_bytes, bwd_bytes;
};

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

template <typename T>
int make_plan(int64_t n, int64_t rows, int64_t S, Plan& p) {
  if (n < 1 || n > CPLXAMD_WELCH_MAX_N || rows < 0 || S < 0) return CPLXAMD_EINVAL;
  const bool pow2 = (n & (n - 1)) == 0;
  int64_t M = 1;
  if (pow2) M = n;
  else while (M < 2 * n - 1) M <<= 1;
  p.M = M;
  p.logM = 63 - __builtin_clzll((unsigned long long)M);
  // fused in one workgroup: a forward power-of-two transform up to the LDS limit; the Bluestein pair and the backward
  // (three or four transforms per segment, more values live) up to 8192 points, where they stay free of scratch
  p.fwd_fused = pow2 ? p.logM <= kLogLMax<T> : p.logM <= kLogFusedMax;
  p.bwd_fused = p.logM <= kLogFusedMax;
  p.path = (pow2 ? CPLXAMD_WELCH_DIRECT : CPLXAMD_WELCH_BLUESTEIN) + (p.fwd_fused ? 0 : 1);
  p.logN1 = (p.logM + 1) / 2;
  p.logN2 = p.logM - p.logN1;
  const int64_t cs = sizeof(C2<T>), nv = rows * S;
  int64_t off = 256;                                      // [0, 256): the window scale
  p.off_tw = off;
  off += al256(M * cs);
  p.off_chirp = p.off_bhat = off;
  if (!pow2) {
    off += al256(n * cs);
    p.off_bhat = off;
    off += al256(M * cs);
  }
  const int64_t want = rows > 0 ? ceil_div(kTargetWgs, rows) : 1;   // fused: chunks of G segments per row
  int64_t chunks = S < want ? S : want;
  if (chunks < 1) chunks = 1;
  p.G = S > 0 ? ceil_div(S, chunks) : 1;
  p.chunks = S > 0 ? ceil_div(S, p.G) : 1;
  int64_t GL = kLargeWs / (2 * M * cs);                   // through the workspace: GL vectors per batch
  if (GL < 1) GL = 1;
  if (GL > nv) GL = nv > 0 ? nv : 1;
  if (GL > 65535) GL = 65535;
  p.GL = GL;
  p.off_buf = off;
  p.off_tmp = off + al256(GL * M * cs);
  const int64_t after = p.off_tmp + al256(GL * M * cs);
  p.off_part = p.fwd_fused ? off : after;
  p.fwd_bytes = p.off_part + al256(rows * (p.fwd_fused ? p.chunks : 1) * n * (int64_t)sizeof(T));
  p.off_D = p.bwd_fused ? off : after;
  p.bwd_bytes = p.off_D + al256(nv * n * cs);
  return 0;
}

template <typename T> inline int lds_bytes(int logL) { return (2 * (pad(1 << logL) + 1)) * (int)sizeof(T); }

// f(std::integral_constant<int, l>) for the runtime l in [LO, HI]: the engine is compiled per transform length
template <int LO, int HI, typename F>
inline int with_log(int l, F&& f) {
  if constexpr (LO > HI) {
    return CPLXAMD_EINVAL;
  } else {
    if (l == LO) return f(std::integral_constant<int, LO>{});
    return with_log<LO + 1, HI>(l, f);
  }
}
// the largest fused workgroups: 16384 float32 / 8192 float64 points, 136 KiB
constexpr int kMaxLds = 2 * (pad(1 << 13) + 1) * 8;            // = 2 * (pad(1 << 14) + 1) * 4 + 8
template <typename K>
int lds_attr(PerDeviceOnce& once, K kernel) {
  return set_max_dyn_lds(once, kernel, kMaxLds);
}

inline int ew_grid(int64_t work) { return stream_grid(work, kET); }

// one batched pass of fft_pass<T, logL> (Bluestein filters need M >= 8; four-step halves are >= 2^7)
template <typename T>
int launch_pass(int logL, dim3 grid, const C2<T>* in, C2<T>* out, int64_t vs, int64_t in_u, int64_t in_e, int64_t out_u,
                int64_t out_e, const C2<T>* tw, int ltw, bool twiddle, T sg, hipStream_t st) {
  return with_log<3, kLogLMax<T>>(logL, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    static PerDeviceOnce once;
    if (const int e = lds_attr(once, fft_pass<T, LG>)) return e;
    fft_pass<T, LG><<<grid, kNT<LG>, lds_bytes<T>(LG), st>>>(in, out, vs, in_u, in_e, out_u, out_e, tw, ltw, twiddle, sg);
    CPLXAMD_CHECK_LAUNCH();
    return 0;
  });
}

// one FFT of length M (a power of two) over nv vectors of buf, natural order in and out (tmp: four-step scratch)
template <typename T>
int fft_vectors(const Plan& p, const C2<T>* tw, C2<T>* buf, C2<T>* tmp, int64_t nv, T sg, hipStream_t st) {
  if (p.logM <= kLogLMax<T>)
    return launch_pass<T>(p.logM, dim3(1, nv), buf, buf, p.M, 0, 1, 0, 1, tw, p.logM, false, sg, st);
  const int64_t N1 = 1ll << p.logN1, N2 = 1ll << p.logN2;
  // columns: FFT over n1 of buf[n1 N2 + n2], twiddle, to tmp[k1 N2 + n2]
  if (const int e = launch_pass<T>(p.logN1, dim3(N2, nv), buf, tmp, p.M, 1, N2, 1, N2, tw, p.logM, true, sg, st)) return e;
  // rows: FFT over n2 of tmp[k1 N2 + n2], to buf[k1 + N1 k2]
  return launch_pass<T>(p.logN2, dim3(N1, nv), tmp, buf, p.M, N2, 1, 1, N1, tw, p.logM, false, sg, st);
}

// the per-call tables: window scale, twiddles, and for Bluestein the chirp and the transformed filter B
template <typename T>
int build_tables(const Plan& p, const T* w, int64_t n, int scaling, double fs, bool blue, char* ws, hipStream_t st) {
  win_scale<T><<<1, kET, 0, st>>>(w, n, scaling, fs, (T*)ws);
  CPLXAMD_CHECK_LAUNCH();
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  tables<T><<<ew_grid(p.M), kET, 0, st>>>(tw, p.M, blue ? (C2<T>*)(ws + p.off_chirp) : nullptr, n);
  CPLXAMD_CHECK_LAUNCH();
  if (!blue) return 0;
  C2<T>* bh = (C2<T>*)(ws + p.off_bhat);
  chirp_filter<T><<<ew_grid(p.M), kET, 0, st>>>(bh, n, p.M);
  CPLXAMD_CHECK_LAUNCH();
  // four-step scratch: the (not yet used) batch buffer; fused sizes need none
  return fft_vectors<T>(p, tw, bh, (C2<T>*)(ws + p.off_buf), 1, (T)-1, st);
}

template <typename TI, typename T>
int welch_fwd_t(const void* xr, const void* xi, int64_t xrs, int64_t xes, int64_t rows, int64_t S, const void* window,
                int64_t n, int64_t step, int scaling, double fs, void* pxx, char* ws, const Plan& p, hipStream_t st) {
  const bool blue = p.path == CPLXAMD_WELCH_BLUESTEIN || p.path == CPLXAMD_WELCH_BLUESTEIN_FOURSTEP;
  const T* w = (const T*)window;
  const T* sc = (const T*)ws;
  if (const int e = build_tables<T>(p, w, n, scaling, fs, blue, ws, st)) return e;
  const C2<T>* tw = (const C2<T>*)(ws + p.off_tw);
  const C2<T>* bhat = (const C2<T>*)(ws + p.off_bhat);
  const C2<T>* chirp = blue ? (const C2<T>*)(ws + p.off_chirp) : nullptr;
  Seg<TI, T> src{(const TI*)xr, (const TI*)xi, xes, w, n, chirp};
  T* part = (T*)(ws + p.off_part);
  const T f = (T)1 / (T)S;
  if (p.path == CPLXAMD_WELCH_DIRECT || p.path == CPLXAMD_WELCH_BLUESTEIN) {
    const int e = blue ? with_log<3, kLogFusedMax>(p.logM, [&](auto c) -> int {
                           constexpr int LG = decltype(c)::value;
                           static PerDeviceOnce once;
                           if (const int r = lds_attr(once, welch_lds<TI, T, true, LG>)) return r;
                           welch_lds<TI, T, true, LG><<<rows * p.chunks, kNT<LG>, lds_bytes<T>(LG), st>>>(
                               src, xrs, step, S, p.G, p.chunks, tw, bhat, part);
                           CPLXAMD_CHECK_LAUNCH();
                           return 0;
                         })
                       : with_log<0, kLogLMax<T>>(p.logM, [&](auto c) -> int {
                           constexpr int LG = decltype(c)::value;
                           static PerDeviceOnce once;
                           if (const int r = lds_attr(once, welch_lds<TI, T, false, LG>)) return r;
                           welch_lds<TI, T, false, LG><<<rows * p.chunks, kNT<LG>, lds_bytes<T>(LG), st>>>(
                               src, xrs, step, S, p.G, p.chunks, tw, bhat, part);
                           CPLXAMD_CHECK_LAUNCH();
                           return 0;
                         });
    if (e) return e;
  } else {
    C2<T>* buf = (C2<T>*)(ws + p.off_buf);
    C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
    const hipError_t me = hipMemsetAsync(part, 0, rows * n * sizeof(T), st);
    if (me != hipSuccess) return (int)me;
    const int64_t nv_all = rows * S;
    for (int64_t v0 = 0; v0 < nv_all; v0 += p.GL) {
      const int64_t nv = nv_all - v0 < p.GL ? nv_all - v0 : p.GL;
      seg_load<TI, T><<<ew_grid(nv * p.M), kET, 0, st>>>(src, xrs, step, S, v0, nv, p.M, buf);
      CPLXAMD_CHECK_LAUNCH();
      if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)-1, st)) return e;
      if (blue) {
        vec_scale<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, bhat, false, nullptr, n, S, v0);
        CPLXAMD_CHECK_LAUNCH();
        if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)1, st)) return e;
      }
      pow_accum<T><<<ew_grid(((v0 + nv - 1) / S - v0 / S + 1) * n), kET, 0, st>>>(buf, v0, nv, S, p.M, n, part);
      CPLXAMD_CHECK_LAUNCH();
    }
  }
  combine<T><<<ew_grid(rows * n), kET, 0, st>>>(part, rows, p.fwd_fused ? p.chunks : 1, n, f, sc, (T*)pxx);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename T>
int welch_bwd_t(const void* xr, const void* xi, int64_t xrs, int64_t xes, int64_t rows, int64_t T_len, int64_t S,
                const void* window, int64_t n, int64_t step, int scaling, double fs, const void* gp, void* dxr, void* dxi,
                int64_t drs, int64_t des, char* ws, const Plan& p, hipStream_t st) {
  const bool blue = p.path == CPLXAMD_WELCH_BLUESTEIN || p.path == CPLXAMD_WELCH_BLUESTEIN_FOURSTEP;
  const T* w = (const T*)window;
  const T* g = (const T*)gp;
  const T* sc = (const T*)ws;
  if (const int e = build_tables<T>(p, w, n, scaling, fs, blue, ws, st)) return e;
  const C2<T>* tw = (const C2<T>*)(ws + p.off_tw);
  const C2<T>* bhat = (const C2<T>*)(ws + p.off_bhat);
  const C2<T>* chirp = blue ? (const C2<T>*)(ws + p.off_chirp) : nullptr;
  Seg<TI, T> src{(const TI*)xr, (const TI*)xi, xes, w, n, chirp};
  C2<T>* D = (C2<T>*)(ws + p.off_D);
  const T f = (T)2 / (T)S;                               // 2 c = 2 / (S scale)
  if (S > 0) {
    if (p.bwd_fused) {
      const int e = blue ? with_log<3, kLogFusedMax>(p.logM, [&](auto c) -> int {
                             constexpr int LG = decltype(c)::value;
                             static PerDeviceOnce once;
                             if (const int r = lds_attr(once, welch_bwd_lds<TI, T, true, LG>)) return r;
                             welch_bwd_lds<TI, T, true, LG><<<rows * p.chunks, kNT<LG>, lds_bytes<T>(LG), st>>>(
                                 src, xrs, step, S, p.G, p.chunks, tw, bhat, g, D);
                             CPLXAMD_CHECK_LAUNCH();
                             return 0;
                           })
                         : with_log<0, kLogFusedMax>(p.logM, [&](auto c) -> int {
                             constexpr int LG = decltype(c)::value;
                             static PerDeviceOnce once;
                             if (const int r = lds_attr(once, welch_bwd_lds<TI, T, false, LG>)) return r;
                             welch_bwd_lds<TI, T, false, LG><<<rows * p.chunks, kNT<LG>, lds_bytes<T>(LG), st>>>(
                                 src, xrs, step, S, p.G, p.chunks, tw, bhat, g, D);
                             CPLXAMD_CHECK_LAUNCH();
                             return 0;
                           });
      if (e) return e;
    } else {
      C2<T>* buf = (C2<T>*)(ws + p.off_buf);
      C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
      const int64_t nv_all = rows * S;
      for (int64_t v0 = 0; v0 < nv_all; v0 += p.GL) {
        const int64_t nv = nv_all - v0 < p.GL ? nv_all - v0 : p.GL;
        const int eg = ew_grid(nv * p.M);
        seg_load<TI, T><<<eg, kET, 0, st>>>(src, xrs, step, S, v0, nv, p.M, buf);
        CPLXAMD_CHECK_LAUNCH();
        if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)-1, st)) return e;
        if (blue) {
          vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, bhat, false, nullptr, n, S, v0);
          CPLXAMD_CHECK_LAUNCH();
          if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)1, st)) return e;
        }
        vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, nullptr, false, g, n, S, v0);
        CPLXAMD_CHECK_LAUNCH();
        if (blue) {
          if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)-1, st)) return e;
          vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, bhat, true, nullptr, n, S, v0);
          CPLXAMD_CHECK_LAUNCH();
        }
        if (const int e = fft_vectors<T>(p, tw, buf, tmp, nv, (T)1, st)) return e;
        seg_store<T><<<ew_grid(nv * n), kET, 0, st>>>(buf, v0, nv, p.M, n, w, chirp, D);
        CPLXAMD_CHECK_LAUNCH();
      }
    }
  }
  gather<TI, T><<<ew_grid(rows * T_len), kET, 0, st>>>(D, rows, T_len, n, step, S, f, sc, (TI*)dxr, (TI*)dxi, drs, des);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

inline bool dtype_ok(int dtype) { return dtype == CPLXAMD_F32 || dtype == CPLXAMD_BF16 || dtype == CPLXAMD_F64; }

inline int plan_for(int64_t n, int64_t rows, int64_t S, int dtype, Plan& p) {
  if (!dtype_ok(dtype)) return CPLXAMD_EINVAL;
  return dtype == CPLXAMD_F64 ? make_plan<double>(n, rows, S, p) : make_plan<float>(n, rows, S, p);
}

// shared argument checks; -> segments
inline int check_args(const void* xr, const void* xi, int64_t xes, int64_t rows, int64_t T_len, const void* window,
                      int64_t n, int64_t step, int scaling, double fs, const void* ws, int dtype, int64_t& S) {
  if (!dtype_ok(dtype) || n < 1 || n > CPLXAMD_WELCH_MAX_N || rows < 0 || T_len < n || step < 1 || xes < 1 ||
      (scaling != CPLXAMD_WELCH_DENSITY && scaling != CPLXAMD_WELCH_SPECTRUM) || !(fs == fs))
    return CPLXAMD_EINVAL;
  if (!xr || !xi || !window || !ws) return CPLXAMD_EINVAL;
  S = (T_len - n) / step + 1;
  return 0;
}

// the fused launches index workgroups by rows * chunks in one grid dimension
inline bool grid_ok(bool fused, const Plan& p, int64_t rows) { return !fused || rows * p.chunks <= 0x7fffffff; }

}  // namespace sp
}  // namespace cplxamd

using namespace cplxamd;
using namespace cplxamd::sp;

extern "C" {

int cplxamd_welch_plan(int64_t n, int64_t rows, int64_t segments, int dtype, int64_t* ws_fwd, int64_t* ws_bwd) {
  Plan p;
  if (const int e = plan_for(n, rows, segments, dtype, p)) return e;
  if (ws_fwd) *ws_fwd = p.fwd_bytes;
  if (ws_bwd) *ws_bwd = p.bwd_bytes;
  return p.path;
}

int cplxamd_welch_fwd(const void* x_r, const void* x_i, int64_t x_row_stride, int64_t x_stride, int64_t rows, int64_t t,
                      const void* window, int64_t n, int64_t step, int scaling, double fs, void* pxx, void* ws,
                      int64_t ws_bytes, int dtype, void* stream) {
  int64_t S = 0;
  if (const int e = check_args(x_r, x_i, x_stride, rows, t, window, n, step, scaling, fs, ws, dtype, S)) return e;
  if (!pxx) return CPLXAMD_EINVAL;
  Plan p;
  if (const int e = plan_for(n, rows, S, dtype, p); e < 0) return e;
  if (!grid_ok(p.fwd_fused, p, rows)) return CPLXAMD_ESHAPE;
  if (ws_bytes < p.fwd_bytes) return CPLXAMD_EWS;
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (dtype == CPLXAMD_F64)
    return welch_fwd_t<double, double>(x_r, x_i, x_row_stride, x_stride, rows, S, window, n, step, scaling, fs, pxx, w, p, st);
  if (dtype == CPLXAMD_BF16)
    return welch_fwd_t<bf16_t, float>(x_r, x_i, x_row_stride, x_stride, rows, S, window, n, step, scaling, fs, pxx, w, p, st);
  return welch_fwd_t<float, float>(x_r, x_i, x_row_stride, x_stride, rows, S, window, n, step, scaling, fs, pxx, w, p, st);
}

int cplxamd_welch_bwd(const void* x_r, const void* x_i, int64_t x_row_stride, int64_t x_stride, int64_t rows, int64_t t,
                      const void* window, int64_t n, int64_t step, int scaling, double fs, const void* g, void* dx_r,
                      void* dx_i, int64_t dx_row_stride, int64_t dx_stride, void* ws, int64_t ws_bytes, int dtype,
                      void* stream) {
  int64_t S = 0;
  if (const int e = check_args(x_r, x_i, x_stride, rows, t, window, n, step, scaling, fs, ws, dtype, S)) return e;
  if (!g || !dx_r || !dx_i || dx_stride < 1) return CPLXAMD_EINVAL;
  Plan p;
  if (const int e = plan_for(n, rows, S, dtype, p); e < 0) return e;
  if (!grid_ok(p.bwd_fused, p, rows)) return CPLXAMD_ESHAPE;
  if (ws_bytes < p.bwd_bytes) return CPLXAMD_EWS;
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (dtype == CPLXAMD_F64)
    return welch_bwd_t<double, double>(x_r, x_i, x_row_stride, x_stride, rows, t, S, window, n, step, scaling, fs, g, dx_r,
                                       dx_i, dx_row_stride, dx_stride, w, p, st);
  if (dtype == CPLXAMD_BF16)
    return welch_bwd_t<bf16_t, float>(x_r, x_i, x_row_stride, x_stride, rows, t, S, window, n, step, scaling, fs, g, dx_r,
                                      dx_i, dx_row_stride, dx_stride, w, p, st);
  return welch_bwd_t<float, float>(x_r, x_i, x_row_stride, x_stride, rows, t, S, window, n, step, scaling, fs, g, dx_r,
                                   dx_i, dx_row_stride, dx_stride, w, p, st);
}

}  // extern "C"
