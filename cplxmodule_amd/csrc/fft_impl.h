// The kernels, plan users and launch templates of fft.hip (which describes them), as a header: fft.hip instantiates them for
// cplx.fft, the short-time transforms (stft_c2c*.hip) for framed, windowed input and windowed output.
#pragma once
#include "fft_engine.h"

namespace cplxamd {
namespace sp {

// P: the loader / store policy of the short-time transforms (NoStft of fft_engine.h adds nothing and takes no storage).
//   kFramed    in(xo, p) is pol.load2(xr, xi, xo, p): xo is a VIRTUAL offset that names row and frame, the policy maps it
//              (padding index map, window; a null xi is a plane of zeros that is never read) to a sample or to zero
//   kWindowed  the outputs are multiplied by pol.win(k) in the store
template <typename TI, typename TO, typename T, typename P = NoStft>
struct Io {
  const TI* xr; const TI* xi; TO* yr; TO* yi;
  int64_t xes, yes, n, n_in;
  const C2<T>* chirp; const C2<T>* bhat;                  // Bluestein only
  bool inv;
  T scale;
  [[no_unique_address]] P pol;                            // the default takes no storage: the kernel arguments are what they were
  // element p of the vector at offset xo, with the opening chirp for Bluestein
  template <bool BLUE> __device__ __forceinline__ C2<T> in(int64_t xo, int64_t p) const {
    C2<T> a;
    if constexpr (P::kFramed) {
      a = pol.load2(xr, xi, xo, p);
    } else {
      const int64_t o = xo + p * xes;
      a = C2<T>{(T)ld<TI>::at(xr + o), (T)ld<TI>::at(xi + o)};
    }
    if constexpr (BLUE) a = inv ? cmulc(a, chirp[p]) : cmul(a, chirp[p]);
    return a;
  }
  // output k of the vector at offset yo: closing chirp, scale, one rounding
  template <bool BLUE> __device__ __forceinline__ void out(int64_t yo, int64_t k, C2<T> y) const {
    if constexpr (BLUE) y = inv ? cmulc(y, chirp[k]) : cmul(y, chirp[k]);
    const int64_t o = yo + k * yes;
    if constexpr (P::kWindowed) {
      st_t(yr + o, y.re * scale * pol.win(k));
      st_t(yi + o, y.im * scale * pol.win(k));
    } else {
      st_t(yr + o, y.re * scale);
      st_t(yi + o, y.im * scale);
    }
  }
};

// ---- V vectors of 2^LOGM points per workgroup of V kNT<LOGM> threads, each in its own LDS slice ------------------------
// STAGED (packed only; the launcher picks it when the vectors lie closer together than their elements, i.e. along a
// non-last dim): the V x M tile moves between memory and LDS with the VECTOR index fastest across lanes, so that a wave's
// load covers 64 / V rows of V neighbouring elements.  The engine's own lane order (threadIdx.x / kNT = vector) would
// give a wave kNT rows of 64 / kNT elements: at 256 points, 32 rows of 8 bytes.  The arithmetic is the same either way,
// and so are the bits.
template <typename TI, typename TO, typename T, bool BLUE, int LOGM, int V, bool STAGED, typename P = NoStft>
__global__ __launch_bounds__(V * kNT<LOGM>) void fft_lds(Io<TI, TO, T, P> io, Batch b, const C2<T>* tw) {
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
template <typename TI, typename TO, typename T, bool BLUE, typename P = NoStft>
__global__ __launch_bounds__(kET) void fft_gather(Io<TI, TO, T, P> io, Batch b, int64_t v0, int64_t nv, int64_t M, C2<T>* buf) {
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
template <typename TI, typename TO, typename T, bool BLUE, typename P = NoStft>
__global__ __launch_bounds__(kET) void fft_scatter(Io<TI, TO, T, P> io, Batch b, int64_t v0, int64_t nv, int64_t M,
                                                  const C2<T>* buf) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * io.n; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / io.n, k = i % io.n;
    int64_t xo, yo;
    batch_offsets(b, v0 + v, xo, yo);
    io.template out<BLUE>(yo, k, buf[v * M + k]);
  }
}

template <typename TI, typename TO, typename T, bool BLUE, int LOGM, int V, bool STAGED, typename P>
int launch_lds(const Io<TI, TO, T, P>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = lds_attr(once, fft_lds<TI, TO, T, BLUE, LOGM, V, STAGED, P>)) return e;
  const int64_t wgs = ceil_div(b.total, V);
  const int lds = V == 1 ? lds_bytes<T>(LOGM) : V * kSlice<LOGM> * (int)sizeof(T);
  fft_lds<TI, TO, T, BLUE, LOGM, V, STAGED, P><<<(unsigned)wgs, V * kNT<LOGM>, lds, st>>>(io, b, tw);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO, typename T, bool BLUE, typename P>
int fft_lds_any(const FftPlan& p, bool packed, const Io<TI, TO, T, P>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  constexpr int LO = BLUE ? 3 : 0;                        // a Bluestein M is at least 8 (n = 3)
  if (packed) {
    // vectors closer together than their elements, on both sides (a transform along a non-last dim): move tiles
    // (a frame axis never is: its side of the frame workspace is dense along the vector)
    const bool staged = !P::kFramed && !P::kWindowed && b.s2 > 1 && b.xs[2] < io.xes && b.ys[2] < io.yes;
    return with_log<LO, kLogPackMax>(p.logM, [&](auto c) -> int {
      constexpr int LG = decltype(c)::value;
      if constexpr (P::kFramed || P::kWindowed) return launch_lds<TI, TO, T, BLUE, LG, kVecs<LG>, false>(io, b, tw, st);
      else return staged ? launch_lds<TI, TO, T, BLUE, LG, kVecs<LG>, true>(io, b, tw, st)
                    : launch_lds<TI, TO, T, BLUE, LG, kVecs<LG>, false>(io, b, tw, st);
    });
  }
  return with_log<LO, BLUE ? kLogFusedMax : kLogLMax<T>>(p.logM, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    return launch_lds<TI, TO, T, BLUE, LG, 1, false>(io, b, tw, st);
  });
}

template <typename TI, typename TO, typename T, bool BLUE, typename P>
int fft_ws(const FftPlan& p, const Io<TI, TO, T, P>& io, const Batch& b, const C2<T>* tw, char* ws, hipStream_t st) {
  C2<T>* buf = (C2<T>*)(ws + p.off_buf);
  C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
  for (int64_t v0 = 0; v0 < b.total; v0 += p.GL) {
    const int64_t nv = b.total - v0 < p.GL ? b.total - v0 : p.GL;
    fft_gather<TI, TO, T, BLUE, P><<<ew_grid(nv * p.M), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
    CPLXAMD_CHECK_LAUNCH();
    if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, BLUE || !io.inv ? (T)-1 : (T)1, st)) return e;
    if constexpr (BLUE) {
      fft_mul<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, io.bhat, io.inv);
      CPLXAMD_CHECK_LAUNCH();
      if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
    }
    fft_scatter<TI, TO, T, BLUE, P><<<ew_grid(nv * io.n), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

// `build`: write the per-call tables first (false: an earlier call with the same n and dtype left them in ws)
template <typename TI, typename TO, typename T, typename P = NoStft>
int fft_t(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_fft_desc& d, const Batch& b, const FftPlan& p,
          char* ws, hipStream_t st, const P& pol = P{}, bool build = true) {
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  C2<T>* chirp = (C2<T>*)(ws + p.off_chirp);
  C2<T>* bhat = (C2<T>*)(ws + p.off_bhat);
  if (build && (p.blue || p.logM > 3)) {                           // up to 8 points: one register stage, no twiddle is read
    tables<T><<<ew_grid(p.M), kET, 0, st>>>(tw, p.M, p.blue ? chirp : nullptr, d.n);
    CPLXAMD_CHECK_LAUNCH();
  }
  if (build && p.blue) {
    chirp_filter<T><<<ew_grid(p.M), kET, 0, st>>>(bhat, d.n, p.M);
    CPLXAMD_CHECK_LAUNCH();
    // four-step scratch: the (not yet used) batch buffer; the sizes held in LDS need none
    if (const int e = fft_vectors<T>(p.logM, tw, bhat, (C2<T>*)(ws + p.off_buf), 1, (T)-1, st)) return e;
  }
  const bool inv = (d.inverse & CPLXAMD_FFT_INVERSE) != 0;
  const Io<TI, TO, T, P> io{(const TI*)xr, (const TI*)xi, (TO*)yr, (TO*)yi, d.x_es, d.y_es, d.n, d.n_in, chirp, bhat, inv,
                         (T)d.scale, pol};
  if (p.lds) {
    const bool packed = p.vpw > 1 && !(d.inverse & CPLXAMD_FFT_ONE_PER_WORKGROUP);
    return p.blue ? fft_lds_any<TI, TO, T, true, P>(p, packed, io, b, tw, st)
                  : fft_lds_any<TI, TO, T, false, P>(p, packed, io, b, tw, st);
  }
  return p.blue ? fft_ws<TI, TO, T, true, P>(p, io, b, tw, ws, st) : fft_ws<TI, TO, T, false, P>(p, io, b, tw, ws, st);
}

}  // namespace sp
}  // namespace cplxamd
