// Chirp-z transforms of planar complex tensors (cplx.czt / zoom_fft: cplxmodule_amd/czt.py) on the engine of fft_engine.h.
// One call transforms every vector of a strided batch along one dim, with host scalars w and a:
//     y[v][k] = scale * sum_{j < n} x[v][j] a^{-j} w^{jk},   k in [0, m)
// Through jk = (j^2 + k^2 - (k - j)^2) / 2 this is Bluestein's sequence with the pins taken out (cplxamd_fft's Bluestein
// branch is the case w = e^{-2 pi i / n}, a = 1, m = n):
//     y_k = close_k IFFT_M(FFT_M(x . open) . B-hat)_k,  open_j = a^{-j} w^{j^2/2},  close_k = w^{k^2/2},
//     B-hat = FFT_M(b),  b_i = w^{-i^2/2} / M at index i mod M for -n < i < m, 0 elsewhere,
// a linear convolution of length n + m - 1 run cyclically at M = 2^ceil(log2(n + m - 1)) >= 8.  With CPLXAMD_CZT_A_OUT
// the power of a moves from the opening to the closing table (close_k = a^{-k} w^{k^2/2}): the adjoint of a transform
// (n, m, w, a) is the transform (m, n, conj w, conj a) with that flag, which is all the backward needs.
// x and y are plane pairs (x_i may be NULL: a plane of zeros that is never read) with an element stride along the
// transformed dim and up to three batch runs, as cplxamd_fft's.  bf16 planes are widened on load, the arithmetic is
// float32 (float64 for float64 planes), and every output is rounded once, on store.
//
// Paths (czt_plan_t below; the kernels are fft_lds's Bluestein branch with two tables, a general filter and n != m):
//   packed      M <= 1024: a 256-thread workgroup transforms V = 2048 / M vectors (256 for M = 8), vector threadIdx.x / kNT
//               in its own LDS slice; the threads of a partly filled last workgroup load zeros, run every stage and skip
//               the stores.
//   one vector  per workgroup for M = 2^11 .. 2^13 (kLogFusedMax): the same kernel with V = 1.
//               In both the transform is ONE launch after the table launches: it reads n inputs and writes m outputs per
//               vector, nothing of length M touches memory.
//   workspace   M up to 2^22: batches of at most GL vectors are gathered into C2 buffers (with the opening table), run
//               through fft_vectors (four-step above the LDS limit), multiplied by B-hat, run back and scattered with the
//               closing table, the scale and the one rounding.
// The per-call tables (twiddles, open, close, B-hat) are built in the caller's workspace by czt_tables and one FFT_M; the
// library keeps no state.  Every table entry is computed in float64 from the log-modulus and the turn fraction of w and a
// and rounded once: the phase theta i^2 / 2 mod 1 is formed from the product's fma residual (i^2 is exact up to 2^44),
// so it keeps its accuracy as i grows, and goes through sincospi.  No atomics: the same input gives the same bits.  No
// kernel uses scratch (-Rpass-analysis=kernel-resource-usage).
#include "fft_engine.h"

#include <cmath>

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

// theta * q mod 1 in [-1/2, 1/2] (+ the residual), q an integer that a double holds exactly: the rounded product and
// its exact fma residual are reduced separately, so the error is that of theta alone; `half` halves both first (exact).
// No contraction here: fused into p - rint(p), the product would carry its residual already and r would count twice.
__device__ __forceinline__ double turns(double theta, double q, bool half) {
#pragma clang fp contract(off)
  double p = __dmul_rn(theta, q);
  double r = fma(theta, q, -p);
  if (half) {
    p *= 0.5;
    r *= 0.5;
  }
  return (p - rint(p)) + r;
}

// w^{s i^2 / 2} [a^{-i}] from log-moduli and turn fractions, in float64
struct Contour {
  double w_log, w_turn, a_log, a_turn;
  __device__ __forceinline__ C2<double> at(int64_t i, double s, bool with_a) const {
    const double q = (double)(i * i);                     // exact: |i| < 2^22
    double ph = s * turns(w_turn, q, true), lg = s * w_log * q * 0.5;
    if (with_a) {
      ph -= turns(a_turn, (double)i, false);
      lg -= a_log * (double)i;
    }
    double sn, cs;
    sincospi(2.0 * ph, &sn, &cs);
    const double mod = lg == 0.0 ? 1.0 : exp(lg);
    return {mod * cs, mod * sn};
  }
};

// tw[q] = e^{-2 pi i q / M};  open[j], j < n;  close[k], k < m;  b[i mod M] = w^{-i^2/2} / M for -n < i < m, else 0
template <typename T>
__global__ __launch_bounds__(kET) void czt_tables(C2<T>* tw, C2<T>* open, C2<T>* close, C2<T>* b, int64_t n, int64_t m,
                                                  int64_t M, Contour c, bool a_out) {
  const double inv = 1.0 / (double)M;
  for (int64_t q = (int64_t)blockIdx.x * kET + threadIdx.x; q < M; q += (int64_t)gridDim.x * kET) {
    tw[q] = cis<T>((T)-1, q, M);
    if (q < n) {
      const C2<double> v = c.at(q, 1.0, !a_out);
      open[q] = {(T)v.re, (T)v.im};
    }
    if (q < m) {
      const C2<double> v = c.at(q, 1.0, a_out);
      close[q] = {(T)v.re, (T)v.im};
    }
    const int64_t i = q < m ? q : (M - q < n ? M - q : -1);   // the ranges are disjoint: M >= n + m - 1
    C2<double> v{0, 0};
    if (i >= 0) v = c.at(i, -1.0, false);
    b[q] = {(T)(v.re * inv), (T)(v.im * inv)};
  }
}

template <typename TI, typename TO, typename T>
struct CztIo {
  const TI* xr; const TI* xi; TO* yr; TO* yi;            // xi may be null: zeros that are never read
  int64_t xes, yes, n, m;
  const C2<T>* open; const C2<T>* close; const C2<T>* bhat;
  T scale;
  // element p < n of the vector at offset xo, with the opening table
  __device__ __forceinline__ C2<T> in(int64_t xo, int64_t p) const {
    const int64_t o = xo + p * xes;
    const C2<T> c = open[p];
    const T re = (T)ld<TI>::at(xr + o);
    if (!xi) return {re * c.re, re * c.im};
    return cmul(C2<T>{re, (T)ld<TI>::at(xi + o)}, c);
  }
  // output k < m of the vector at offset yo: closing table, scale, one rounding
  __device__ __forceinline__ void out(int64_t yo, int64_t k, C2<T> y) const {
    y = cmul(y, close[k]);
    const int64_t o = yo + k * yes;
    st_t(yr + o, y.re * scale);
    st_t(yi + o, y.im * scale);
  }
};

// ---- V vectors per workgroup of V kNT<LOGM> threads, each in its own LDS slice: load, FFT_M, B-hat, inverse FFT_M, store
template <typename TI, typename TO, typename T, int LOGM, int V>
__global__ __launch_bounds__(V * kNT<LOGM>) void czt_lds(CztIo<TI, TO, T> io, Batch b, const C2<T>* tw) {
  constexpr int E = kEOf<LOGM>, M = 1 << LOGM, NT = kNT<LOGM>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int u = V == 1 ? 0 : threadIdx.x / NT;
  int t = V == 1 ? threadIdx.x : threadIdx.x % NT;
  T* sre = (T*)smem + (V == 1 ? 0 : u * kSlice<LOGM>);
  T* sim = sre + pad(M) + 1;
  const int64_t vec = (int64_t)blockIdx.x * V + u;
  const bool ok = vec < b.total;                          // a partly filled last workgroup: zeros in, no stores
  int64_t xo = 0, yo = 0;
  if (ok) batch_offsets(b, vec, xo, yo);
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = {0, 0};
  auto from_lds = [&](int p) { return C2<T>{sre[pad(p)], sim[pad(p)]}; };
  auto load = [&](int p) -> C2<T> {
    if (!ok || p >= io.n) return {0, 0};
    return io.in(xo, p);
  };
  if constexpr (LOGM >= 13) {
    // the second transform takes its lane index through a volatile LDS read, as fft_lds does: the compiler may not keep
    // the addresses of every stage of both transforms live at once
    __shared__ int zero;
    if (threadIdx.x == 0) zero = 0;
    __syncthreads();
    fft_run<T, LOGM>(v, sre, sim, t, (T)-1, tw, LOGM, load);
    t += *(const volatile int*)&zero;
  } else {
    fft_run<T, LOGM>(v, sre, sim, t, (T)-1, tw, LOGM, load);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGM>(e, t, k)) v[e] = cmul(v[e], io.bhat[k]);
  }
  to_lds<T, LOGM>(v, sre, sim, t);
  fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGM>(e, t, k) && k < io.m && ok) io.out(yo, k, v[e]);
  }
}

// ---- through the workspace, one grid row (blockIdx.y) per vector of the batch (at most 65535): its offsets are formed once
// buf[v][p] = element p of vector v0 + v with the opening table, 0 for p >= n; p in [0, M)
template <typename TI, typename TO, typename T>
__global__ __launch_bounds__(kET) void czt_gather(CztIo<TI, TO, T> io, Batch b, int64_t v0, int logM, C2<T>* buf) {
  const int64_t v = blockIdx.y, M = (int64_t)1 << logM;
  int64_t xo, yo;
  batch_offsets(b, v0 + v, xo, yo);
  C2<T>* row = buf + (v << logM);
  for (int64_t p = (int64_t)blockIdx.x * kET + threadIdx.x; p < M; p += (int64_t)gridDim.x * kET)
    row[p] = p < io.n ? io.in(xo, p) : C2<T>{0, 0};
}

// y[v0 + v][k] = buf[v][k] (closing table, scale, one rounding), k in [0, m)
template <typename TI, typename TO, typename T>
__global__ __launch_bounds__(kET) void czt_scatter(CztIo<TI, TO, T> io, Batch b, int64_t v0, int logM, const C2<T>* buf) {
  const int64_t v = blockIdx.y;
  int64_t xo, yo;
  batch_offsets(b, v0 + v, xo, yo);
  const C2<T>* row = buf + (v << logM);
  for (int64_t k = (int64_t)blockIdx.x * kET + threadIdx.x; k < io.m; k += (int64_t)gridDim.x * kET) io.out(yo, k, row[k]);
}

// ---- plan --------------------------------------------------------------------------------------------------------------
struct CztPlan {
  int path, logM, vpw;
  int64_t M, GL;                        // through the workspace: GL vectors per batch
  int64_t off_tw, off_open, off_close, off_bhat, off_buf, off_tmp, bytes;
};

template <typename T>
int czt_plan_t(int64_t n, int64_t m, int64_t vectors, CztPlan& p) {
  if (n < 1 || m < 1 || vectors < 0) return CPLXAMD_EINVAL;
  if (n > CPLXAMD_WELCH_MAX_N || m > CPLXAMD_WELCH_MAX_N || n + m - 1 > CPLXAMD_WELCH_MAX_N) return CPLXAMD_ESHAPE;
  int64_t M = 8;
  while (M < n + m - 1) M <<= 1;
  p.M = M;
  p.logM = 63 - __builtin_clzll((unsigned long long)M);
  p.path = p.logM <= kLogPackMax ? CPLXAMD_CZT_PACKED : p.logM <= kLogFusedMax ? CPLXAMD_CZT_FUSED : CPLXAMD_CZT_WORKSPACE;
  p.vpw = p.path == CPLXAMD_CZT_PACKED ? (int)(kPackT / (M / 8)) : 1;
  const int64_t cs = sizeof(C2<T>);
  int64_t off = 0;
  p.off_tw = off;
  off += al256(M * cs);
  p.off_open = off;
  off += al256(n * cs);
  p.off_close = off;
  off += al256(m * cs);
  p.off_bhat = off;
  off += al256(M * cs);
  p.off_buf = p.off_tmp = off;
  p.GL = 1;
  if (p.path == CPLXAMD_CZT_WORKSPACE) {                  // batches bounded as cplxamd_fft's
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

int czt_plan_for(int64_t n, int64_t m, int64_t vectors, int dtype, CztPlan& p) {
  if (dtype == CPLXAMD_F64) return czt_plan_t<double>(n, m, vectors, p);
  if (dtype == CPLXAMD_F32 || dtype == CPLXAMD_BF16) return czt_plan_t<float>(n, m, vectors, p);
  return CPLXAMD_EINVAL;
}

template <typename TI, typename TO, typename T, int LOGM, int V>
int launch_czt(const CztIo<TI, TO, T>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = lds_attr(once, czt_lds<TI, TO, T, LOGM, V>)) return e;
  const int64_t wgs = ceil_div(b.total, V);
  const int lds = V == 1 ? lds_bytes<T>(LOGM) : V * kSlice<LOGM> * (int)sizeof(T);
  czt_lds<TI, TO, T, LOGM, V><<<(unsigned)wgs, V * kNT<LOGM>, lds, st>>>(io, b, tw);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO, typename T>
int czt_t(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_czt_desc& d, const Batch& b, const CztPlan& p,
          char* ws, hipStream_t st) {
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  C2<T>* open = (C2<T>*)(ws + p.off_open);
  C2<T>* close = (C2<T>*)(ws + p.off_close);
  C2<T>* bhat = (C2<T>*)(ws + p.off_bhat);
  C2<T>* buf = (C2<T>*)(ws + p.off_buf);
  C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
  const Contour c{d.w_log, d.w_turn, d.a_log, d.a_turn};
  czt_tables<T><<<ew_grid(p.M), kET, 0, st>>>(tw, open, close, bhat, d.n, d.m, p.M, c, (d.flags & CPLXAMD_CZT_A_OUT) != 0);
  CPLXAMD_CHECK_LAUNCH();
  // four-step scratch: the (not yet used) batch buffer; the packed and fused paths have none (buf is the workspace's
  // end) and need none, their M fits the LDS pass of either compute type
  static_assert(kLogFusedMax <= kLogLMax<double> && kLogFusedMax <= kLogLMax<float>, "a fused M must not take four steps");
  if (const int e = fft_vectors<T>(p.logM, tw, bhat, buf, 1, (T)-1, st)) return e;
  const CztIo<TI, TO, T> io{(const TI*)xr, (const TI*)xi, (TO*)yr, (TO*)yi, d.x_es, d.y_es, d.n, d.m, open, close, bhat,
                            (T)d.scale};
  if (p.path == CPLXAMD_CZT_PACKED)
    return with_log<3, kLogPackMax>(p.logM, [&](auto lg) -> int {
      constexpr int LG = decltype(lg)::value;
      return launch_czt<TI, TO, T, LG, kVecs<LG>>(io, b, tw, st);
    });
  if (p.path == CPLXAMD_CZT_FUSED)
    return with_log<kLogPackMax + 1, kLogFusedMax>(p.logM, [&](auto lg) -> int {
      constexpr int LG = decltype(lg)::value;
      return launch_czt<TI, TO, T, LG, 1>(io, b, tw, st);
    });
  for (int64_t v0 = 0; v0 < b.total; v0 += p.GL) {
    const int64_t nv = b.total - v0 < p.GL ? b.total - v0 : p.GL;
    czt_gather<TI, TO, T><<<dim3((unsigned)ceil_div(p.M, kET), (unsigned)nv), kET, 0, st>>>(io, b, v0, p.logM, buf);
    CPLXAMD_CHECK_LAUNCH();
    if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)-1, st)) return e;
    fft_mul<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, bhat, false);
    CPLXAMD_CHECK_LAUNCH();
    if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
    czt_scatter<TI, TO, T><<<dim3((unsigned)ceil_div(d.m, kET), (unsigned)nv), kET, 0, st>>>(io, b, v0, p.logM, buf);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

// the batch of a descriptor, as batch_of does for cplxamd_fft_desc
int czt_batch(const cplxamd_czt_desc& d, Batch& b) {
  using D = cplxamd_czt_desc;
  int64_t size[3];
  const RunStride<D> f[] = {{&D::x_stride, b.xs}, {&D::y_stride, b.ys}};
  if (const int e = decode_runs(d, f, size, b.total, true)) return e;
  b.s1 = size[1] > 0 ? size[1] : 1;
  b.s2 = size[2] > 0 ? size[2] : 1;
  return 0;
}

inline bool is_finite(double v) { return v - v == 0; }

}  // namespace

extern "C" {

int cplxamd_czt_plan(int64_t n, int64_t m, int64_t vectors, int dtype, int* vectors_per_workgroup, int64_t* ws_bytes) {
  CztPlan p;
  if (const int e = czt_plan_for(n, m, vectors, dtype, p)) return e;
  if (vectors_per_workgroup) *vectors_per_workgroup = p.vpw;
  if (ws_bytes) *ws_bytes = p.bytes;
  return p.path;
}

int cplxamd_czt(const void* x_r, const void* x_i, void* y_r, void* y_i, const cplxamd_czt_desc* d, int in_dtype,
                int out_dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_r || !y_r || !y_i || !d || !ws) return CPLXAMD_EINVAL;
  const bool f32ish_in = in_dtype == CPLXAMD_F32 || in_dtype == CPLXAMD_BF16;
  const bool f32ish_out = out_dtype == CPLXAMD_F32 || out_dtype == CPLXAMD_BF16;
  if (!((f32ish_in && f32ish_out) || (in_dtype == CPLXAMD_F64 && out_dtype == CPLXAMD_F64))) return CPLXAMD_EINVAL;
  if (d->n < 1 || d->m < 1 || d->x_es < 0 || d->y_es < 1 || d->runs < 0 || d->runs > 3 || (d->flags & ~CPLXAMD_CZT_A_OUT) ||
      !is_finite(d->w_log) || !is_finite(d->w_turn) || !is_finite(d->a_log) || !is_finite(d->a_turn) || !is_finite(d->scale))
    return CPLXAMD_EINVAL;
  Batch b;
  if (const int e = czt_batch(*d, b)) return e;
  CztPlan p;
  if (const int e = czt_plan_for(d->n, d->m, b.total, in_dtype, p)) return e;
  if (b.total > 0x7fffffffll) return CPLXAMD_ESHAPE;     // workgroups are indexed by one grid dimension
  if (ws_bytes < p.bytes) return CPLXAMD_EWS;
  if (b.total == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (in_dtype == CPLXAMD_F64) return czt_t<double, double, double>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
  if (in_dtype == CPLXAMD_BF16)
    return out_dtype == CPLXAMD_BF16 ? czt_t<bf16_t, bf16_t, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st)
                                     : czt_t<bf16_t, float, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
  return out_dtype == CPLXAMD_BF16 ? czt_t<float, bf16_t, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st)
                                   : czt_t<float, float, float>(x_r, x_i, y_r, y_i, *d, b, p, w, st);
}

}  // extern "C"
