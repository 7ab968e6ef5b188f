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
#include "fft_engine.h"

namespace cplxamd {
namespace sp {

template <typename TI, typename TO, typename T>
struct Io {
  const TI* xr; const TI* xi; TO* yr; TO* yi;
  int64_t xes, yes, n, n_in;
  const C2<T>* chirp; const C2<T>* bhat;                  // Bluestein only
  bool inv;
  T scale;
  // element p of the vector at offset xo, with the opening chirp for Bluestein
  template <bool BLUE> __device__ __forceinline__ C2<T> in(int64_t xo, int64_t p) const {
    const int64_t o = xo + p * xes;
    C2<T> a{(T)ld<TI>::at(xr + o), (T)ld<TI>::at(xi + o)};
    if constexpr (BLUE) a = inv ? cmulc(a, chirp[p]) : cmul(a, chirp[p]);
    return a;
  }
  // output k of the vector at offset yo: closing chirp, scale, one rounding
  template <bool BLUE> __device__ __forceinline__ void out(int64_t yo, int64_t k, C2<T> y) const {
    if constexpr (BLUE) y = inv ? cmulc(y, chirp[k]) : cmul(y, chirp[k]);
    const int64_t o = yo + k * yes;
    st_t(yr + o, y.re * scale);
    st_t(yi + o, y.im * scale);
  }
};

// ---- V vectors of 2^LOGM points per workgroup of V kNT<LOGM> threads, each in its own LDS slice ------------------------
// STAGED (packed only; the launcher picks it when the vectors lie closer together than their elements, i.e. along a
// non-last dim): the V x M tile moves between memory and LDS with the VECTOR index fastest across lanes, so that a wave's
// load covers 64 / V rows of V neighbouring elements.  The engine's own lane order (threadIdx.x / kNT = vector) would
// give a wave kNT rows of 64 / kNT elements: at 256 points, 32 rows of 8 bytes.  The arithmetic is the same either way,
// and so are the bits.
template <typename TI, typename TO, typename T, bool BLUE, int LOGM, int V, bool STAGED>
__global__ __launch_bounds__(V * kNT<LOGM>) void fft_lds(Io<TI, TO, T> io, Batch b, const C2<T>* tw) {
  static_assert(!STAGED || V > 1, "staging is for packed workgroups");
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
  // the tile's lane order: vector tv of the workgroup, rows tp, tp + 256 / V, ...
  const int tv = threadIdx.x % V, tp = threadIdx.x / V;
  T* tre = (T*)smem + tv * kSlice<LOGM>;
  T* tim = tre + pad(M) + 1;
  const bool tok = (int64_t)blockIdx.x * V + tv < b.total;
  int64_t txo = 0, tyo = 0;
  if constexpr (STAGED) {
    if (tok) batch_offsets(b, (int64_t)blockIdx.x * V + tv, txo, tyo);
    for (int p = tp; p < M; p += kPackT / V) {
      C2<T> a{0, 0};
      if (tok && p < io.n_in) a = io.template in<BLUE>(txo, p);
      tre[pad(p)] = a.re;
      tim[pad(p)] = a.im;
    }
    __syncthreads();
  }
  auto load = [&](int p) -> C2<T> {
    if constexpr (STAGED) return from_lds(p);
    if (!ok || p >= io.n_in) return {0, 0};
    return io.template in<BLUE>(xo, p);
  };
  if constexpr (!BLUE) {
    fft_run<T, LOGM>(v, sre, sim, t, io.inv ? (T)1 : (T)-1, tw, LOGM, load);
  } else {
    if constexpr (LOGM >= 13) {
      // the second transform takes its lane index through a volatile LDS read, as the Welch kernels do per segment: the
      // compiler may not keep the addresses of every stage of both transforms live at once (at 8192 float64 points they
      // overflowed the register file into scratch)
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
      if (out_k<LOGM>(e, t, k)) v[e] = io.inv ? cmulc(v[e], io.bhat[k]) : cmul(v[e], io.bhat[k]);
    }
    to_lds<T, LOGM>(v, sre, sim, t);
    fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
  }
  if constexpr (STAGED) {
    to_lds<T, LOGM>(v, sre, sim, t);
    for (int k = tp; k < M; k += kPackT / V)
      if (tok && k < io.n) io.template out<BLUE>(tyo, k, C2<T>{tre[pad(k)], tim[pad(k)]});
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      int k;
      if (out_k<LOGM>(e, t, k) && k < io.n && ok) io.template out<BLUE>(yo, k, v[e]);
    }
  }
}

// ---- through the workspace ---------------------------------------------------------------------------------------------
// buf[v][p] = element p of vector v0 + v (with the opening chirp), 0 for p >= n_in; p in [0, M)
template <typename TI, typename TO, typename T, bool BLUE>
__global__ __launch_bounds__(kET) void fft_gather(Io<TI, TO, T> io, Batch b, int64_t v0, int64_t nv, int64_t M, C2<T>* buf) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * M; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / M, p = i % M;
    C2<T> a{0, 0};
    if (p < io.n_in) {
      int64_t xo, yo;
      batch_offsets(b, v0 + v, xo, yo);
      a = io.template in<BLUE>(xo, p);
    }
    buf[i] = a;
  }
}

// y[v0 + v][k] = buf[v][k] (closing chirp, scale, one rounding), k in [0, n)
template <typename TI, typename TO, typename T, bool BLUE>
__global__ __launch_bounds__(kET) void fft_scatter(Io<TI, TO, T> io, Batch b, int64_t v0, int64_t nv, int64_t M,
                                                  const C2<T>* buf) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * io.n; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / io.n, k = i % io.n;
    int64_t xo, yo;
    batch_offsets(b, v0 + v, xo, yo);
    io.template out<BLUE>(yo, k, buf[v * M + k]);
  }
}

template <typename TI, typename TO, typename T, bool BLUE, int LOGM, int V, bool STAGED>
int launch_lds(const Io<TI, TO, T>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = lds_attr(once, fft_lds<TI, TO, T, BLUE, LOGM, V, STAGED>)) return e;
  const int64_t wgs = ceil_div(b.total, V);
  const int lds = V == 1 ? lds_bytes<T>(LOGM) : V * kSlice<LOGM> * (int)sizeof(T);
  fft_lds<TI, TO, T, BLUE, LOGM, V, STAGED><<<(unsigned)wgs, V * kNT<LOGM>, lds, st>>>(io, b, tw);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO, typename T, bool BLUE>
int fft_lds_any(const FftPlan& p, bool packed, const Io<TI, TO, T>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  constexpr int LO = BLUE ? 3 : 0;                        // a Bluestein M is at least 8 (n = 3)
  if (packed) {
    // vectors closer together than their elements, on both sides (a transform along a non-last dim): move tiles
    const bool staged = b.s2 > 1 && b.xs[2] < io.xes && b.ys[2] < io.yes;
    return with_log<LO, kLogPackMax>(p.logM, [&](auto c) -> int {
      constexpr int LG = decltype(c)::value;
      return staged ? launch_lds<TI, TO, T, BLUE, LG, kVecs<LG>, true>(io, b, tw, st)
                    : launch_lds<TI, TO, T, BLUE, LG, kVecs<LG>, false>(io, b, tw, st);
    });
  }
  return with_log<LO, BLUE ? kLogFusedMax : kLogLMax<T>>(p.logM, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    return launch_lds<TI, TO, T, BLUE, LG, 1, false>(io, b, tw, st);
  });
}

template <typename TI, typename TO, typename T, bool BLUE>
int fft_ws(const FftPlan& p, const Io<TI, TO, T>& io, const Batch& b, const C2<T>* tw, char* ws, hipStream_t st) {
  C2<T>* buf = (C2<T>*)(ws + p.off_buf);
  C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
  for (int64_t v0 = 0; v0 < b.total; v0 += p.GL) {
    const int64_t nv = b.total - v0 < p.GL ? b.total - v0 : p.GL;
    fft_gather<TI, TO, T, BLUE><<<ew_grid(nv * p.M), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
    CPLXAMD_CHECK_LAUNCH();
    if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, BLUE || !io.inv ? (T)-1 : (T)1, st)) return e;
    if constexpr (BLUE) {
      fft_mul<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, io.bhat, io.inv);
      CPLXAMD_CHECK_LAUNCH();
      if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
    }
    fft_scatter<TI, TO, T, BLUE><<<ew_grid(nv * io.n), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

template <typename TI, typename TO, typename T>
int fft_t(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_fft_desc& d, const Batch& b, const FftPlan& p,
          char* ws, hipStream_t st) {
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  C2<T>* chirp = (C2<T>*)(ws + p.off_chirp);
  C2<T>* bhat = (C2<T>*)(ws + p.off_bhat);
  if (p.blue || p.logM > 3) {                             // up to 8 points: one register stage, no twiddle is read
    tables<T><<<ew_grid(p.M), kET, 0, st>>>(tw, p.M, p.blue ? chirp : nullptr, d.n);
    CPLXAMD_CHECK_LAUNCH();
  }
  if (p.blue) {
    chirp_filter<T><<<ew_grid(p.M), kET, 0, st>>>(bhat, d.n, p.M);
    CPLXAMD_CHECK_LAUNCH();
    // four-step scratch: the (not yet used) batch buffer; the sizes held in LDS need none
    if (const int e = fft_vectors<T>(p.logM, tw, bhat, (C2<T>*)(ws + p.off_buf), 1, (T)-1, st)) return e;
  }
  const bool inv = (d.inverse & CPLXAMD_FFT_INVERSE) != 0;
  const Io<TI, TO, T> io{(const TI*)xr, (const TI*)xi, (TO*)yr, (TO*)yi, d.x_es, d.y_es, d.n, d.n_in, chirp, bhat, inv,
                         (T)d.scale};
  if (p.lds) {
    const bool packed = p.vpw > 1 && !(d.inverse & CPLXAMD_FFT_ONE_PER_WORKGROUP);
    return p.blue ? fft_lds_any<TI, TO, T, true>(p, packed, io, b, tw, st)
                  : fft_lds_any<TI, TO, T, false>(p, packed, io, b, tw, st);
  }
  return p.blue ? fft_ws<TI, TO, T, true>(p, io, b, tw, ws, st) : fft_ws<TI, TO, T, false>(p, io, b, tw, ws, st);
}

}  // namespace sp
}  // namespace cplxamd

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
