// The package's FFT engine: a Stockham FFT of a power-of-two length held by one workgroup (or one slice of one), the
// batched pass kernel and the four-step driver built on it, and the per-call tables.  Shared by the Welch spectra
// (spectrum.hip, which describes the engine and the size classes at its top) and the transforms themselves (fft.hip,
// rfft.hip), whose batch, plan and packing constants stand at the end.
//
// Engine (fft_run): compiled per length 2^LOGL <= 2^kLogLMax: every stage, stride and thread count is a compile-time
// constant.  kNT<LOGL> threads hold kEOf<LOGL> values each; radix-8 butterflies (one leading radix-2 / 4 stage when 3 does
// not divide LOGL) run in registers; between stages the values make one LDS round trip, planes padded by one word per 16
// (pad()).  The barriers of a stage (`stage`) lie OUTSIDE its `j < NB` guards: every thread of the workgroup must reach
// every stage, whether or not it holds data.  Twiddles come from a table in the caller's workspace (tables): every entry
// is sincospi of an exactly reduced argument.  No state in the library, no atomics.
#pragma once
#include "common.h"
#include "launch.h"
#include "runs.h"

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

// ---- the per-call tables ---------------------------------------------------------------------------------------------
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

// ---- host side -------------------------------------------------------------------------------------------------------
inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

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

// one FFT of length M = 2^logM over nv (<= 65535) vectors of buf, natural order in and out (tmp: four-step scratch, not
// read when logM <= kLogLMax<T>).  Above the LDS limit, four steps with N = N1 N2: a column pass (FFT over n1 of
// buf[n1 N2 + n2], twiddle e^{sg 2 pi i n2 k1 / N}) and a row pass (FFT over n2) that writes X[k1 + N1 k2].
template <typename T>
int fft_vectors(int logM, const C2<T>* tw, C2<T>* buf, C2<T>* tmp, int64_t nv, T sg, hipStream_t st) {
  const int64_t M = 1ll << logM;
  if (logM <= kLogLMax<T>) return launch_pass<T>(logM, dim3(1, nv), buf, buf, M, 0, 1, 0, 1, tw, logM, false, sg, st);
  const int logN1 = (logM + 1) / 2, logN2 = logM - logN1;
  const int64_t N1 = 1ll << logN1, N2 = 1ll << logN2;
  // columns: FFT over n1 of buf[n1 N2 + n2], twiddle, to tmp[k1 N2 + n2]
  if (const int e = launch_pass<T>(logN1, dim3(N2, nv), buf, tmp, M, 1, N2, 1, N2, tw, logM, true, sg, st)) return e;
  // rows: FFT over n2 of tmp[k1 N2 + n2], to buf[k1 + N1 k2]
  return launch_pass<T>(logN2, dim3(N1, nv), tmp, buf, M, N2, 1, 1, N1, tw, logM, false, sg, st);
}

// ---- shared by the transforms of fft.hip and rfft.hip: the packed workgroup, the batch, the plan ---------------------------
constexpr int kPackT = 256;                               // threads of a packed workgroup
constexpr int kLogPackMax = 10;                           // packed up to 1024 points
template <int LOGM> constexpr int kVecs = kPackT / kNT<LOGM>;
// words of one vector's LDS slice in a packed workgroup: odd
template <int LOGM> constexpr int kSlice = 2 * (pad(1 << LOGM) + 1) + 1;

// The default loader / store policy of Io (fft_impl.h) and RIo (rfft_impl.h): nothing framed, nothing windowed, no
// storage.  The short-time transforms (stft_impl.h) bring their own.
struct NoStft {
  static constexpr bool kFramed = false, kWindowed = false;
};

// the batch of a call: three runs (unused ones have size 1), run 2 innermost
struct Batch {
  int64_t total, s1, s2, xs[3], ys[3];
};
__device__ __forceinline__ void batch_offsets(const Batch& b, int64_t v, int64_t& xo, int64_t& yo) {
  const int64_t i2 = v % b.s2, q = v / b.s2, i1 = q % b.s1, i0 = q / b.s1;
  xo = i0 * b.xs[0] + i1 * b.xs[1] + i2 * b.xs[2];
  yo = i0 * b.ys[0] + i1 * b.ys[1] + i2 * b.ys[2];
}

// the batch of a descriptor: its runs right-aligned (the innermost run is run 2), strides of any sign, an empty inner
// run as one of size 1 (total is 0: nothing is launched)
inline int batch_of(const cplxamd_fft_desc& d, Batch& b) {
  using D = cplxamd_fft_desc;
  int64_t size[3];
  const RunStride<D> f[] = {{&D::x_stride, b.xs}, {&D::y_stride, b.ys}};
  if (const int e = decode_runs(d, f, size, b.total, true)) return e;
  b.s1 = size[1] > 0 ? size[1] : 1;
  b.s2 = size[2] > 0 ? size[2] : 1;
  return 0;
}

// buf[v][k] *= h[k] (conj: conj(h[k]))
template <typename T>
__global__ __launch_bounds__(kET) void fft_mul(C2<T>* buf, int64_t nv, int64_t M, const C2<T>* h, bool conj) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * M; i += (int64_t)gridDim.x * kET)
    buf[i] = conj ? cmulc(buf[i], h[i % M]) : cmul(buf[i], h[i % M]);
}

// ---- plan --------------------------------------------------------------------------------------------------------------
struct FftPlan {
  int path, logM, vpw;                  // vpw: vectors per workgroup (1 unless packed)
  bool blue, lds;                       // lds: the whole transform inside one workgroup's LDS
  int64_t M, GL;                        // through the workspace: GL vectors per batch
  int64_t off_tw, off_chirp, off_bhat, off_buf, off_tmp, bytes;
};

template <typename T>
int fft_plan_t(int64_t n, int64_t vectors, FftPlan& p) {
  if (n < 1 || n > CPLXAMD_WELCH_MAX_N || vectors < 0) return CPLXAMD_EINVAL;
  const bool pow2 = (n & (n - 1)) == 0;
  int64_t M = 1;
  if (pow2) M = n;
  else while (M < 2 * n - 1) M <<= 1;
  p.M = M;
  p.logM = 63 - __builtin_clzll((unsigned long long)M);
  p.blue = !pow2;
  p.lds = pow2 ? p.logM <= kLogLMax<T> : p.logM <= kLogFusedMax;
  p.path = (pow2 ? CPLXAMD_WELCH_DIRECT : CPLXAMD_WELCH_BLUESTEIN) + (p.lds ? 0 : 1);
  const int64_t nt = M / 8 > 0 ? M / 8 : 1;               // kNT of a packed length
  p.vpw = p.lds && p.logM <= kLogPackMax ? (int)(kPackT / nt) : 1;
  const int64_t cs = sizeof(C2<T>);
  int64_t off = 0;
  p.off_tw = off;
  off += al256(M * cs);
  p.off_chirp = p.off_bhat = off;
  if (p.blue) {
    off += al256(n * cs);
    p.off_bhat = off;
    off += al256(M * cs);
  }
  p.off_buf = p.off_tmp = off;
  p.GL = 1;
  if (!p.lds) {                                           // batches bounded as Welch's
    int64_t GL = kLargeWs / (2 * M * cs);
    if (GL < 1) GL = 1;
    if (GL > vectors) GL = vectors > 0 ? vectors : 1;
    if (GL > 65535) GL = 65535;
    p.GL = GL;
    p.off_tmp = off + al256(GL * M * cs);
    off = p.off_tmp + al256(GL * M * cs);
  }
  p.bytes = off;
  return 0;
}

inline int fft_plan_for(int64_t n, int64_t vectors, int dtype, FftPlan& p) {
  if (dtype == CPLXAMD_F64) return fft_plan_t<double>(n, vectors, p);
  if (dtype == CPLXAMD_F32 || dtype == CPLXAMD_BF16) return fft_plan_t<float>(n, vectors, p);
  return CPLXAMD_EINVAL;
}

}  // namespace sp
}  // namespace cplxamd
