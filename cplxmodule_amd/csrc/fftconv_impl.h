// Overlap-save convolution on the FFT engine: the plan, the kernels and the launch templates of
// fftconv.hip (which describes them) and fftconv_wgrad.hip, as a header so that the two build side by side.
#pragma once
#include "fft_impl.h"
#include "runs.h"

namespace cplxamd {
namespace sp {

constexpr int kLogConvMax = kLogFusedMax;                 // two transforms in one workgroup: up to 8192 points
constexpr int64_t kConvFusedK = 4096;                     // longer filters: composed from cplxamd_fft launches
constexpr int64_t kConvWsMax = 1ll << 40;                 // spectra or partials beyond 1 TiB: CPLXAMD_ESHAPE
constexpr int64_t kConvLenMax = 1ll << 48;                // operand lengths and |start|: every offset stays in 64 bits
constexpr int kLogConvFloor = 9;                          // the plan's shortest block (measured)
constexpr int kLogWgradFloor = 11;                        // and the weight gradient's: one block per 256-thread workgroup
constexpr int64_t kConvWgs = 768;                         // weight gradient: about three workgroups per CU

struct ConvPlan {
  int path, logL, vpw, wlogL;
  int64_t L, S, blocks, in_shift, out_lo, n_valid;        // cplxamd_fftconv
  int64_t off_tw, off_h, bytes;
  int64_t Lw, Sw, wblocks, pairs, chunks, per_chunk;      // cplxamd_fftconv_wgrad
  int64_t woff_tw, woff_part, wbytes;
};

inline int ceil_log2(int64_t v) {
  int l = 0;
  while ((1ll << l) < v) ++l;
  return l;
}

// A: entries of a, K: filter taps, (start, C): the window of the result (P1) / start and the entries of c (P2)
inline int conv_plan_for(int64_t A, int64_t K, int64_t start, int64_t C, int64_t rows, int64_t filters, int dtype, int conj,
                         int log_l, ConvPlan& p) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (A < 1 || K < 1 || C < 1 || A > kConvLenMax || K > kConvLenMax || C > kConvLenMax || start > kConvLenMax ||
      start < -kConvLenMax || rows < 0 || filters < 0 || (conj != 0 && conj != 1))
    return CPLXAMD_EINVAL;
  if (log_l < 0 || log_l > kLogConvMax || (log_l > 0 && (1ll << log_l) < K)) return CPLXAMD_EINVAL;
  p = ConvPlan{};
  if (K > kConvFusedK) {
    if (A + K - 1 > CPLXAMD_WELCH_MAX_N) return CPLXAMD_ESHAPE;
    p.path = CPLXAMD_FFTCONV_COMPOSED;
    p.logL = ceil_log2(A + K - 1);
    p.L = 1ll << p.logL;
    return 0;
  }
  p.path = CPLXAMD_FFTCONV_FUSED;
  const int64_t cs = dtype == CPLXAMD_F64 ? 16 : 8;       // bytes of a C2 of the compute type
  // ---- P1: at least three quarters of a block are outputs (L >= 4 K), never shorter than the floor, never longer than
  // the block that holds the whole window
  int l = log_l;
  if (!l) {
    l = ceil_log2(4 * K);
    if (l < kLogConvFloor) l = kLogConvFloor;
    const int cap = ceil_log2((A < C ? A : C) + K - 1);
    if (l > cap) l = cap;
    if (l > kLogConvMax) l = kLogConvMax;
  }
  p.logL = l;
  p.L = 1ll << l;
  p.S = p.L - K + 1;
  p.vpw = l <= kLogPackMax ? (int)(kPackT / (p.L / 8 > 0 ? p.L / 8 : 1)) : 1;
  // one block holds every product when L >= A + K - 1: the cyclic result IS the linear one, lag q at entry q mod L, for
  // q in [0, L) (convolution) or [-(K - 1), L - K + 1) (correlation)
  const bool single = p.L >= A + K - 1 && (conj ? start >= -(K - 1) && start + C <= p.L - K + 1 : start >= 0 && start + C <= p.L);
  if (single) {
    p.blocks = 1;
    p.in_shift = 0;
    p.out_lo = ((start % p.L) + p.L) % p.L;
    p.n_valid = C;
  } else {
    p.blocks = ceil_div(C, p.S);
    p.in_shift = conj ? start : start - (K - 1);
    p.out_lo = conj ? 0 : K - 1;
    p.n_valid = p.S;
  }
  p.off_tw = 0;
  p.off_h = al256(p.L * cs);
  int64_t hbytes;                                         // one spectrum per distinct filter: grows with the filters, unbounded
  if (__builtin_mul_overflow(filters > 0 ? filters : 1, p.L * cs, &hbytes) || hbytes > kConvWsMax) return CPLXAMD_ESHAPE;
  p.bytes = p.off_h + al256(hbytes);
  // ---- P2: blocks of a (S samples, zero tail) against blocks of c (L samples)
  int lw = log_l;
  if (!lw) {
    lw = ceil_log2(4 * K);
    if (lw < kLogWgradFloor) lw = kLogWgradFloor;
    const int cap = ceil_log2(A + K - 1);
    if (lw > cap) lw = cap;
    if (lw > kLogConvMax) lw = kLogConvMax;
  }
  p.wlogL = lw;
  p.Lw = 1ll << lw;
  p.Sw = p.Lw - K + 1;
  p.wblocks = ceil_div(A, p.Sw);
  const int64_t nf = filters > 0 ? filters : 1;
  if (__builtin_mul_overflow(rows / nf, p.wblocks, &p.pairs)) return CPLXAMD_ESHAPE;
  int64_t chunks = ceil_div(kConvWgs, nf);
  const int64_t slabs = dtype == CPLXAMD_F64 && lw >= 13 ? 2 : 1;   // fftconv_wgrad_lds: the accumulator's stash
  int64_t one;                                            // bytes of one partial per result: the least the call needs
  if (__builtin_mul_overflow(nf, p.Lw * cs * slabs, &one) || one > kConvWsMax) return CPLXAMD_ESHAPE;
  // further chunks only while the partials stay within the engine's batch buffers; one partial per result is the floor,
  // so with many results the workspace exceeds kLargeWs (up to kConvWsMax)
  const int64_t most = kLargeWs / one;
  if (chunks > most) chunks = most;
  if (chunks > p.pairs) chunks = p.pairs;
  if (chunks < 1) chunks = 1;
  p.per_chunk = ceil_div(p.pairs > 0 ? p.pairs : 1, chunks);
  p.chunks = ceil_div(p.pairs > 0 ? p.pairs : 1, p.per_chunk);
  p.woff_tw = 0;
  p.woff_part = al256(p.Lw * cs);
  p.wbytes = p.woff_part + al256(one * p.chunks);
  return 0;
}

// a null imaginary plane is a plane of zeros that is never read
template <typename TI, typename T>
__device__ __forceinline__ C2<T> ld2(const TI* xr, const TI* xi, int64_t o) {
  return {(T)ld<TI>::at(xr + o), xi ? (T)ld<TI>::at(xi + o) : (T)0};
}

// the filter's loader for the transform kernel: taps at their own element stride
template <typename TI, typename T>
struct FilterIn {
  static constexpr bool kFramed = true, kWindowed = false;
  int64_t es;
  __device__ __forceinline__ C2<T> load2(const TI* xr, const TI* xi, int64_t xo, int64_t p) const {
    return ld2<TI, T>(xr, xi, xo + p * es);
  }
};

// ---- P1 ---------------------------------------------------------------------------------------------------------------
template <typename TI, typename TO, typename T>
struct ConvIo {
  const TI* ar; const TI* ai; TO* yr; TO* yi;
  const C2<T>* H;                                         // [filter][L], 1 / L folded in
  int64_t A, C, S, in_shift, bpr, total, a_es;
  Sub ay, h;                                              // (a, y) strides; h.p: filter index strides
  int out_lo, n_valid;
  bool conj;
};

template <typename TI, typename TO, typename T, int LOGL, int V>
__global__ __launch_bounds__(V * kNT<LOGL>) void fftconv_lds(ConvIo<TI, TO, T> g, const C2<T>* tw) {
  constexpr int E = kEOf<LOGL>, L = 1 << LOGL, NT = kNT<LOGL>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int u = V == 1 ? 0 : threadIdx.x / NT;
  int t = V == 1 ? threadIdx.x : threadIdx.x % NT;
  T* sre = (T*)smem + (V == 1 ? 0 : u * kSlice<LOGL>);
  T* sim = sre + pad(L) + 1;
  const int64_t vec = (int64_t)blockIdx.x * V + u;
  const bool ok = vec < g.total;                          // a partly filled last workgroup: zeros in, no stores
  int64_t ao = 0, yo = 0, ho = 0, base = 0, left = 0;
  if (ok) {
    const int64_t row = vec / g.bpr, j = vec - row * g.bpr;   // one division per block
    int64_t unused;
    sub_offsets(g.ay, row, ao, yo);
    sub_offsets(g.h, row, ho, unused);
    ho *= L;
    yo += j * g.S;
    base = j * g.S + g.in_shift;
    left = g.C - j * g.S < g.n_valid ? g.C - j * g.S : g.n_valid;
  }
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = {0, 0};
  auto load = [&](int p) -> C2<T> {
    const int64_t i = base + p;
    if (!ok || i < 0 || i >= g.A) return {0, 0};          // zeros are never read
    return ld2<TI, T>(g.ar, g.ai, ao + i * g.a_es);
  };
  auto from_lds = [&](int p) { return C2<T>{sre[pad(p)], sim[pad(p)]}; };
  if constexpr (LOGL >= 13) {
    // as fft_lds's Bluestein branch: the second transform takes its lane index through a volatile LDS read, so that the
    // addresses of both transforms' stages are not all live at once
    __shared__ int zero;
    if (threadIdx.x == 0) zero = 0;
    __syncthreads();
    fft_run<T, LOGL>(v, sre, sim, t, (T)-1, tw, LOGL, load);
    t += *(const volatile int*)&zero;
  } else {
    fft_run<T, LOGL>(v, sre, sim, t, (T)-1, tw, LOGL, load);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGL>(e, t, k)) v[e] = g.conj ? cmulc(v[e], g.H[ho + k]) : cmul(v[e], g.H[ho + k]);
  }
  to_lds<T, LOGL>(v, sre, sim, t);
  fft_run<T, LOGL>(v, sre, sim, t, (T)1, tw, LOGL, from_lds);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGL>(e, t, k)) {
      const int64_t n = (k - g.out_lo) & (L - 1);
      if (n < left) {
        st_t(g.yr + yo + n, v[e].re);
        if (g.yi) st_t(g.yi + yo + n, v[e].im);          // a null plane is not stored
      }
    }
  }
}

template <typename TI, typename TO, typename T, int LOGL, int V>
int launch_conv(const ConvIo<TI, TO, T>& g, const C2<T>* tw, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = lds_attr(once, fftconv_lds<TI, TO, T, LOGL, V>)) return e;
  const int lds = V == 1 ? lds_bytes<T>(LOGL) : V * kSlice<LOGL> * (int)sizeof(T);
  fftconv_lds<TI, TO, T, LOGL, V><<<(unsigned)ceil_div(g.total, V), V * kNT<LOGL>, lds, st>>>(g, tw);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

// ---- P2 ---------------------------------------------------------------------------------------------------------------
template <typename TI, typename T>
struct WgradIo {
  const TI* ar; const TI* ai; const TI* cr; const TI* ci;
  int64_t A, C, S, start, wblocks, pairs, per_chunk, chunks, a_es, c_es;
  Sub kept, red;                                          // (a, c) strides of the result's runs and of the reduced runs
};

// workgroup (f, chunk): part[f][chunk][.] = sum over the chunk's (reduced row, block) pairs, ascending, of
// conj(FFT(a block, S samples and a zero tail)) FFT(c block, L samples)
// The accumulator lives in registers, except for 8192 float64 points: there three arrays of 16 complex doubles exceed the
// 256 registers of a 512-thread workgroup (two still spill), so the workgroup's own partial spectrum in the workspace is
// the accumulator and A-hat waits in a second slab of it while the c block is transformed (the plan doubles the buffer; each entry is
// read and written by the one thread that owns it, in the same ascending order: the same sums).
// The launch bound is at least one wave: with the one-thread workgroups of up to 8 points declared as such the compiler
// proves every value uniform, moves the whole transform to scalar registers and runs out of them.
template <typename TI, typename T, int LOGL>
__global__ __launch_bounds__(kNT<LOGL> < 64 ? 64 : kNT<LOGL>) void fftconv_wgrad_lds(WgradIo<TI, T> g, const C2<T>* tw, C2<T>* part) {
  constexpr int E = kEOf<LOGL>, L = 1 << LOGL;
  constexpr bool kAccInRegs = !(LOGL >= 13 && sizeof(T) == 8);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int zero;
  T* sre = (T*)smem;
  T* sim = sre + pad(L) + 1;
  if (threadIdx.x == 0) zero = 0;
  __syncthreads();
  const int64_t f = blockIdx.x / g.chunks, ch = blockIdx.x - f * g.chunks;
  int64_t a0, c0;
  sub_offsets(g.kept, f, a0, c0);
  C2<T> acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = {0, 0};
  C2<T>* dst = part + (int64_t)blockIdx.x * L;
  C2<T>* stash = part + ((int64_t)gridDim.x + blockIdx.x) * L;     // !kAccInRegs: behind every workgroup's partial
  const int64_t q0 = ch * g.per_chunk, q1 = q0 + g.per_chunk < g.pairs ? q0 + g.per_chunk : g.pairs;
  for (int64_t q = q0; q < q1; ++q) {       // the same range for every thread: the barriers are uniform
    const int64_t rr = q / g.wblocks, j = q - rr * g.wblocks;
    int64_t ao, co;
    sub_offsets(g.red, rr, ao, co);
    ao += a0;
    co += c0;
    // the lane index through a volatile LDS read per pair, as the Welch kernels do per segment: the compiler may not
    // keep the addresses of every stage of both transforms live across the loop
    const int t = threadIdx.x + *(const volatile int*)&zero;
    C2<T> va[E];
#pragma unroll
    for (int e = 0; e < E; ++e) va[e] = {0, 0};
    auto load_a = [&](int p) -> C2<T> {
      const int64_t i = j * g.S + p;
      if (p >= g.S || i >= g.A) return {0, 0};
      return ld2<TI, T>(g.ar, g.ai, ao + i * g.a_es);
    };
    auto load_c = [&](int p) -> C2<T> {
      const int64_t i = j * g.S + g.start + p;
      if (i < 0 || i >= g.C) return {0, 0};
      return ld2<TI, T>(g.cr, g.ci, co + i * g.c_es);
    };
    fft_run<T, LOGL>(va, sre, sim, t, (T)-1, tw, LOGL, load_a);
    if constexpr (kAccInRegs) {
      C2<T> vc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) vc[e] = {0, 0};
      fft_run<T, LOGL>(vc, sre, sim, t, (T)-1, tw, LOGL, load_c);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const C2<T> m = cmulc(vc[e], va[e]);
        acc[e] = {acc[e].re + m.re, acc[e].im + m.im};
      }
    } else {
      // every entry is written and read back by the one thread that owns it
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGL>(e, t, k)) stash[k] = va[e];
      }
#pragma unroll
      for (int e = 0; e < E; ++e) va[e] = {0, 0};
      fft_run<T, LOGL>(va, sre, sim, t, (T)-1, tw, LOGL, load_c);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGL>(e, t, k)) {
          const C2<T> m = cmulc(va[e], stash[k]);
          const C2<T> s = q == q0 ? C2<T>{0, 0} : dst[k];
          dst[k] = {s.re + m.re, s.im + m.im};
        }
      }
    }
  }
  if constexpr (kAccInRegs) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      int k;
      if (out_k<LOGL>(e, (int)threadIdx.x, k)) dst[k] = acc[e];
    }
  }
}

// part[f][0][p] = sum over chunks, ascending, of part[f][chunk][p]: one thread per entry, so that a result shared by the
// whole batch (one filter, hundreds of chunks) is not summed by the one workgroup that transforms it back
template <typename T>
__global__ __launch_bounds__(kET) void fftconv_wgrad_sum(C2<T>* part, int64_t filters, int64_t chunks, int64_t L) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < filters * L; i += (int64_t)gridDim.x * kET) {
    const int64_t f = i / L, p = i - f * L;
    C2<T>* src = part + f * chunks * L + p;
    C2<T> s = src[0];
    for (int64_t c = 1; c < chunks; ++c) s = {s.re + src[c * L].re, s.im + src[c * L].im};
    src[0] = s;
  }
}

// y[f][m] = scale * IFFT_L(part[f][0])[m], m < K, rounded once (`chunks`: the partials per result, summed into the first)
template <typename TO, typename T, int LOGL>
__global__ __launch_bounds__(kNT<LOGL>) void fftconv_wgrad_finish(const C2<T>* part, int64_t chunks, TO* yr, TO* yi, int64_t K,
                                                                   T scale, Sub ys, const C2<T>* tw) {
  constexpr int E = kEOf<LOGL>, L = 1 << LOGL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sre = (T*)smem;
  T* sim = sre + pad(L) + 1;
  const int t = threadIdx.x;
  const C2<T>* src = part + (int64_t)blockIdx.x * chunks * L;
  int64_t yo, unused;
  sub_offsets(ys, blockIdx.x, yo, unused);
  C2<T> v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = {0, 0};
  auto load = [&](int p) { return src[p]; };
  fft_run<T, LOGL>(v, sre, sim, t, (T)1, tw, LOGL, load);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int k;
    if (out_k<LOGL>(e, t, k) && k < K) {
      st_t(yr + yo + k, v[e].re * scale);
      if (yi) st_t(yi + yo + k, v[e].im * scale);
    }
  }
}

// the checks both launchers share; the plan of the call
inline int conv_check(const void* a_r, const void* b_r, const void* y_r, const cplxamd_fftconv_desc* d, const void* ws,
                      int dtype, bool wgrad, ConvRuns& r, int64_t& filters, int (&kept)[3], ConvPlan& p) {
  if (!a_r || !b_r || !y_r || !d || !ws) return CPLXAMD_EINVAL;
  if (d->a_es < 0 || d->b_es < 0 || d->reserved != 0 || (wgrad && d->conj != 0)) return CPLXAMD_EINVAL;
  using D = cplxamd_fftconv_desc;
  const RunStride<D> f[] = {{&D::a_stride, r.as}, {&D::b_stride, r.bs}, {&D::y_stride, r.ys}};
  if (const int e = decode_runs(*d, f, r.size, r.rows)) return e;
  filters = select_runs(r, wgrad ? r.ys : r.bs, true, kept);
  if (const int e = conv_plan_for(d->a_len, d->k, d->start, d->c_len, r.rows, filters, dtype, d->conj, d->log_l, p)) return e;
  if (p.path != CPLXAMD_FFTCONV_FUSED) return CPLXAMD_EINVAL;
  return 0;
}

}  // namespace sp
}  // namespace cplxamd
