// Welch power spectra (cplxmodule/utils/spectrum.py:7-82 pwelch) on one power-of-two FFT engine, forward and gradient.
//
// The reference spells Welch's method as window_view -> * window -> torch.fft.fft -> abs^2 -> mean: the whole
// [rows, segments, n] windowed block and its spectrum go through memory several times.  Here one launch reads every
// segment straight from x (two plane pointers + element strides: interleaved complex and planar Cplx alike), windows,
// transforms and accumulates |X_k|^2 over a chunk of segments in registers; a second small launch adds the chunks in a
// fixed order, scales and writes [rows, n].  No atomics anywhere: repeated runs give the same bits.
//
// Engine (fft_run; in fft_engine.h, which fft.hip shares): a Stockham FFT of a power-of-two length L <= 2^kLogLMax (16384 float32 / 8192 float64 points, 136
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
#include "fft_engine.h"

#include <type_traits>

namespace cplxamd {
namespace sp {

constexpr int kTargetWgs = 2048;                          // workgroups of a fused launch (segments split to reach it)

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

// ---- elementwise helpers ---------------------------------------------------------------------------------------------
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
  return fft_vectors<T>(p.logM, tw, bh, (C2<T>*)(ws + p.off_buf), 1, (T)-1, st);
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
      if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)-1, st)) return e;
      if (blue) {
        vec_scale<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, bhat, false, nullptr, n, S, v0);
        CPLXAMD_CHECK_LAUNCH();
        if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
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
        if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)-1, st)) return e;
        if (blue) {
          vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, bhat, false, nullptr, n, S, v0);
          CPLXAMD_CHECK_LAUNCH();
          if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
        }
        vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, nullptr, false, g, n, S, v0);
        CPLXAMD_CHECK_LAUNCH();
        if (blue) {
          if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)-1, st)) return e;
          vec_scale<T><<<eg, kET, 0, st>>>(buf, nv, p.M, bhat, true, nullptr, n, S, v0);
          CPLXAMD_CHECK_LAUNCH();
        }
        if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
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
