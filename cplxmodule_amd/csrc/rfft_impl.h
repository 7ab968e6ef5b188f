// The kernels, the plan and the launchers of the real transforms: see rfft.hip, which describes them.  Compiled in two
// translation units, one per direction (rfft.hip: real -> half spectrum; rfft_c2r.hip: half spectrum -> real).
#pragma once
#include "fft_engine.h"

namespace cplxamd {
namespace sp {

// P: the loader / store policy of the short-time transforms (NoStft of fft_engine.h adds nothing):
//   kFramed    real_in(xo, j) is pol.load(xr, xo, j): xo is a VIRTUAL offset that names row and frame, the policy maps
//              it (padding index map, window) to a sample or to zero
//   kWindowed  the real outputs of C2R are multiplied by pol.win(j) in the store
template <typename TI, typename TO, typename T, typename P = NoStft>
struct RIo {
  const TI* xr; const TI* xi; TO* yr; TO* yi;             // R2C reads xr alone, C2R writes yr alone
  int64_t xes, yes, n, h, n_in, L;                        // L: points of the complex transform, h (HALF) or n
  const C2<T>* chirp; const C2<T>* bhat;                  // Bluestein only (of L points)
  const C2<T>* rt;                                        // HALF only: rt[k] = e^{-2 pi i k/n}, k < h
  T sg;
  bool weighted;
  T scale;
  [[no_unique_address]] P pol;                            // the default takes no storage: the kernel arguments are what they were

  __device__ __forceinline__ bool edge(int64_t k) const { return k == 0 || 2 * k == n; }   // DC, Nyquist
  __device__ __forceinline__ T real_in(int64_t xo, int64_t j) const {
    if constexpr (P::kFramed) return j < n_in ? pol.load(xr, xo, j) : (T)0;
    else return j < n_in ? (T)ld<TI>::at(xr + xo + j * xes) : (T)0;
  }
  // c_k X_k / w_k of the half spectrum, k in [0, h]: what the Hermitian extension is formed from
  __device__ __forceinline__ C2<T> half_in(int64_t xo, int64_t k) const {
    if (k >= n_in) return {0, 0};
    const int64_t o = xo + k * xes;
    if (edge(k)) return {(T)ld<TI>::at(xr + o), 0};
    const T c = weighted ? (T)1 : (T)0.5;
    return {c * (T)ld<TI>::at(xr + o), c * (T)ld<TI>::at(xi + o)};
  }
  // element p in [0, L) of the complex transform's input of the vector at offset xo, with Bluestein's opening chirp
  template <bool C2R, bool HALF, bool BLUE> __device__ __forceinline__ C2<T> in(int64_t xo, int64_t p) const {
    C2<T> a;
    if constexpr (!C2R) {
      if constexpr (HALF) a = {real_in(xo, 2 * p), real_in(xo, 2 * p + 1)};
      else a = {real_in(xo, p), 0};
    } else if constexpr (HALF) {
      const C2<T> xk = half_in(xo, p), xc = half_in(xo, h - p);          // conj X_h-p = (xc.re, -xc.im)
      const C2<T> d = cmul(twid(rt, p, sg), C2<T>{xk.re - xc.re, xk.im + xc.im});
      a = {xk.re + xc.re - d.im, xk.im - xc.im + d.re};
    } else {
      a = half_in(xo, p <= h ? p : n - p);
      if (p > h) a.im = -a.im;
    }
    if constexpr (BLUE) a = sg > 0 ? cmulc(a, chirp[p]) : cmul(a, chirp[p]);
    return a;
  }
  // Bluestein's closing chirp on output k < L of the complex transform
  template <bool BLUE> __device__ __forceinline__ C2<T> closed(C2<T> y, int64_t k) const {
    if constexpr (BLUE) return sg > 0 ? cmulc(y, chirp[k]) : cmul(y, chirp[k]);
    return y;
  }
  // outputs stored per vector: half spectrum entries, or elements of the complex result that hold the reals
  template <bool C2R> __host__ __device__ __forceinline__ int64_t count() const { return C2R ? L : h + 1; }
  __device__ __forceinline__ void half_out(int64_t yo, int64_t k, C2<T> y) const {
    const T s = weighted && !edge(k) ? 2 * scale : scale;
    const int64_t o = yo + k * yes;
    st_t(yr + o, y.re * s);
    st_t(yi + o, edge(k) ? (T)0 : y.im * s);
  }
  // output k < count() from the complex result z(q), q in [0, L), closing chirp applied: scale, one rounding
  template <bool C2R, bool HALF, typename Z> __device__ __forceinline__ void out(int64_t yo, int64_t k, Z&& z) const {
    if constexpr (C2R) {
      const C2<T> y = z(k);
      if constexpr (HALF) {
        if constexpr (P::kWindowed) {
          st_t(yr + yo + 2 * k * yes, y.re * scale * pol.win(2 * k));
          st_t(yr + yo + (2 * k + 1) * yes, y.im * scale * pol.win(2 * k + 1));
        } else {
          st_t(yr + yo + 2 * k * yes, y.re * scale);
          st_t(yr + yo + (2 * k + 1) * yes, y.im * scale);
        }
      } else {
        if constexpr (P::kWindowed) st_t(yr + yo + k * yes, y.re * scale * pol.win(k));
        else st_t(yr + yo + k * yes, y.re * scale);
      }
    } else if constexpr (HALF) {
      const C2<T> a = z(k == h ? 0 : k), b = z(k == 0 || k == h ? 0 : h - k);   // indices mod h
      const C2<T> t = k == h ? C2<T>{-1, 0} : twid(rt, k, sg);
      const C2<T> d = cmul(t, C2<T>{a.re - b.re, a.im + b.im});         // t_k (Z_k - conj Z_h-k)
      half_out(yo, k, C2<T>{(T)0.5 * (a.re + b.re + d.im), (T)0.5 * (a.im - b.im - d.re)});
    } else {
      half_out(yo, k, z(k));
    }
  }
};

// ---- V vectors per workgroup, the complex transform of 2^LOGM points in the vector's LDS slice (fft_lds of fft.hip
// with the real loaders and stores) -----------------------------------------------------------------------------------
template <typename TI, typename TO, typename T, bool C2R, bool HALF, bool BLUE, int LOGM, int V, bool STAGED, typename P = NoStft>
__global__ __launch_bounds__(V * kNT<LOGM>) void rfft_lds(RIo<TI, TO, T, P> io, Batch b, const C2<T>* tw) {
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
      if (tok && p < io.L) a = io.template in<C2R, HALF, BLUE>(txo, p);
      tre[pad(p)] = a.re;
      tim[pad(p)] = a.im;
    }
    __syncthreads();
  }
  auto load = [&](int p) -> C2<T> {
    if constexpr (STAGED) return from_lds(p);
    if (!ok || p >= io.L) return {0, 0};
    return io.template in<C2R, HALF, BLUE>(xo, p);
  };
  if constexpr (!BLUE) {
    fft_run<T, LOGM>(v, sre, sim, t, io.sg, tw, LOGM, load);
  } else {
    if constexpr (LOGM >= 13) {
      // the second transform takes its lane index through a volatile LDS read, as fft_lds does
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
      if (out_k<LOGM>(e, t, k)) v[e] = io.sg > 0 ? cmulc(v[e], io.bhat[k]) : cmul(v[e], io.bhat[k]);
    }
    to_lds<T, LOGM>(v, sre, sim, t);
    fft_run<T, LOGM>(v, sre, sim, t, (T)1, tw, LOGM, from_lds);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      int k;
      if (out_k<LOGM>(e, t, k) && k < io.L) v[e] = io.template closed<true>(v[e], k);
    }
  }
  const int64_t count = io.template count<C2R>();
  if constexpr (STAGED) {
    to_lds<T, LOGM>(v, sre, sim, t);
    auto z = [&](int64_t q) { return C2<T>{tre[pad((int)q)], tim[pad((int)q)]}; };
    for (int k = tp; k < count; k += kPackT / V)
      if (tok) io.template out<C2R, HALF>(tyo, k, z);
  } else if constexpr (!C2R && HALF) {
    to_lds<T, LOGM>(v, sre, sim, t);                      // the pair (k, h - k) lies on different lanes
    auto z = [&](int64_t q) { return from_lds((int)q); };
    for (int k = t; k < count; k += NT)
      if (ok) io.template out<C2R, HALF>(yo, k, z);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      int k;
      auto z = [&](int64_t) { return v[e]; };
      if (out_k<LOGM>(e, t, k) && k < count && ok) io.template out<C2R, HALF>(yo, k, z);
    }
  }
}

// ---- through the workspace ---------------------------------------------------------------------------------------------
template <typename TI, typename TO, typename T, bool C2R, bool HALF, bool BLUE, typename P = NoStft>
__global__ __launch_bounds__(kET) void rfft_gather(RIo<TI, TO, T, P> io, Batch b, int64_t v0, int64_t nv, int64_t M, C2<T>* buf) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * M; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / M, p = i % M;
    C2<T> a{0, 0};
    if (p < io.L) {
      int64_t xo, yo;
      batch_offsets(b, v0 + v, xo, yo);
      a = io.template in<C2R, HALF, BLUE>(xo, p);
    }
    buf[i] = a;
  }
}

template <typename TI, typename TO, typename T, bool C2R, bool HALF, bool BLUE, typename P = NoStft>
__global__ __launch_bounds__(kET) void rfft_scatter(RIo<TI, TO, T, P> io, Batch b, int64_t v0, int64_t nv, int64_t M,
                                                   const C2<T>* buf) {
  const int64_t count = io.template count<C2R>();
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < nv * count; i += (int64_t)gridDim.x * kET) {
    const int64_t v = i / count, k = i % count;
    int64_t xo, yo;
    batch_offsets(b, v0 + v, xo, yo);
    auto z = [&](int64_t q) { return io.template closed<BLUE>(buf[v * M + q], q); };
    io.template out<C2R, HALF>(yo, k, z);
  }
}

// rt[k] = e^{-2 pi i k / n}, k < h
template <typename T>
__global__ __launch_bounds__(kET) void rfft_twiddles(C2<T>* rt, int64_t h, int64_t n) {
  for (int64_t k = (int64_t)blockIdx.x * kET + threadIdx.x; k < h; k += (int64_t)gridDim.x * kET) rt[k] = cis<T>((T)-1, k, n);
}

// ---- plan: fft.hip's plan of the complex transform, plus the table t_k --------------------------------------------------
struct RfftPlan {
  FftPlan c;
  bool half;
  int64_t L, off_rt, bytes;
};

inline int rfft_plan_for(int64_t n, int64_t vectors, int dtype, RfftPlan& p) {
  if (n < 1 || n > CPLXAMD_WELCH_MAX_N) return CPLXAMD_EINVAL;
  p.half = n % 2 == 0;
  p.L = p.half ? n / 2 : n;
  if (const int e = fft_plan_for(p.L, vectors, dtype, p.c)) return e;
  p.off_rt = p.c.bytes;
  p.bytes = p.c.bytes + (p.half ? al256(p.L * (dtype == CPLXAMD_F64 ? 16 : 8)) : 0);
  return 0;
}

template <typename TI, typename TO, typename T, bool C2R, bool HALF, bool BLUE, int LOGM, int V, bool STAGED, typename P>
int launch_rlds(const RIo<TI, TO, T, P>& io, const Batch& b, const C2<T>* tw, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = lds_attr(once, rfft_lds<TI, TO, T, C2R, HALF, BLUE, LOGM, V, STAGED, P>)) return e;
  const int64_t wgs = ceil_div(b.total, V);
  const int lds = V == 1 ? lds_bytes<T>(LOGM) : V * kSlice<LOGM> * (int)sizeof(T);
  rfft_lds<TI, TO, T, C2R, HALF, BLUE, LOGM, V, STAGED, P><<<(unsigned)wgs, V * kNT<LOGM>, lds, st>>>(io, b, tw);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO, typename T, bool C2R, bool HALF, bool BLUE, typename P>
int rfft_run(const FftPlan& p, const RIo<TI, TO, T, P>& io, const Batch& b, const C2<T>* tw, char* ws, hipStream_t st) {
  constexpr int LO = BLUE ? 3 : 0;                        // a Bluestein M is at least 8
  // a direct transform of an odd length has one point (n = 1)
  constexpr int PACK_HI = !BLUE && !HALF ? 0 : kLogPackMax;
  if (p.lds && p.vpw > 1) {
    const bool staged = b.s2 > 1 && b.xs[2] < io.xes && b.ys[2] < io.yes;
    return with_log<LO, PACK_HI>(p.logM, [&](auto c) -> int {
      constexpr int LG = decltype(c)::value;
      return staged ? launch_rlds<TI, TO, T, C2R, HALF, BLUE, LG, kVecs<LG>, true>(io, b, tw, st)
                    : launch_rlds<TI, TO, T, C2R, HALF, BLUE, LG, kVecs<LG>, false>(io, b, tw, st);
    });
  }
  if constexpr (BLUE || HALF) {
    if (p.lds)
      return with_log<kLogPackMax + 1, BLUE ? kLogFusedMax : kLogLMax<T>>(p.logM, [&](auto c) -> int {
        constexpr int LG = decltype(c)::value;
        return launch_rlds<TI, TO, T, C2R, HALF, BLUE, LG, 1, false>(io, b, tw, st);
      });
    C2<T>* buf = (C2<T>*)(ws + p.off_buf);
    C2<T>* tmp = (C2<T>*)(ws + p.off_tmp);
    const int64_t count = io.template count<C2R>();
    for (int64_t v0 = 0; v0 < b.total; v0 += p.GL) {
      const int64_t nv = b.total - v0 < p.GL ? b.total - v0 : p.GL;
      rfft_gather<TI, TO, T, C2R, HALF, BLUE, P><<<ew_grid(nv * p.M), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
      CPLXAMD_CHECK_LAUNCH();
      if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, BLUE ? (T)-1 : io.sg, st)) return e;
      if constexpr (BLUE) {
        fft_mul<T><<<ew_grid(nv * p.M), kET, 0, st>>>(buf, nv, p.M, io.bhat, io.sg > 0);
        CPLXAMD_CHECK_LAUNCH();
        if (const int e = fft_vectors<T>(p.logM, tw, buf, tmp, nv, (T)1, st)) return e;
      }
      rfft_scatter<TI, TO, T, C2R, HALF, BLUE, P><<<ew_grid(nv * count), kET, 0, st>>>(io, b, v0, nv, p.M, buf);
      CPLXAMD_CHECK_LAUNCH();
    }
    return 0;
  }
  return CPLXAMD_EINVAL;
}

// `build`: write the per-call tables first (false: an earlier call with the same n and dtype left them in ws)
template <typename TI, typename TO, typename T, bool C2R, typename P = NoStft>
int rfft_t(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_fft_desc& d, const Batch& b, const RfftPlan& rp,
           char* ws, hipStream_t st, const P& pol = P{}, bool build = true) {
  const FftPlan& p = rp.c;
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  C2<T>* chirp = (C2<T>*)(ws + p.off_chirp);
  C2<T>* bhat = (C2<T>*)(ws + p.off_bhat);
  C2<T>* rt = (C2<T>*)(ws + rp.off_rt);
  if (build && (p.blue || p.logM > 3)) {                  // up to 8 points: one register stage, no twiddle is read
    tables<T><<<ew_grid(p.M), kET, 0, st>>>(tw, p.M, p.blue ? chirp : nullptr, rp.L);
    CPLXAMD_CHECK_LAUNCH();
  }
  if (build && rp.half) {
    rfft_twiddles<T><<<ew_grid(rp.L), kET, 0, st>>>(rt, rp.L, d.n);
    CPLXAMD_CHECK_LAUNCH();
  }
  if (build && p.blue) {
    chirp_filter<T><<<ew_grid(p.M), kET, 0, st>>>(bhat, rp.L, p.M);
    CPLXAMD_CHECK_LAUNCH();
    if (const int e = fft_vectors<T>(p.logM, tw, bhat, (C2<T>*)(ws + p.off_buf), 1, (T)-1, st)) return e;
  }
  const RIo<TI, TO, T, P> io{(const TI*)xr, (const TI*)xi, (TO*)yr, (TO*)yi, d.x_es, d.y_es, d.n, d.n / 2, d.n_in, rp.L, chirp,
                          bhat, rt, (d.inverse & CPLXAMD_FFT_INVERSE) ? (T)1 : (T)-1, (d.inverse & CPLXAMD_RFFT_WEIGHTED) != 0,
                          (T)d.scale, pol};
  if (rp.half)
    return p.blue ? rfft_run<TI, TO, T, C2R, true, true>(p, io, b, tw, ws, st)
                  : rfft_run<TI, TO, T, C2R, true, false>(p, io, b, tw, ws, st);
  return p.blue ? rfft_run<TI, TO, T, C2R, false, true>(p, io, b, tw, ws, st)
                : rfft_run<TI, TO, T, C2R, false, false>(p, io, b, tw, ws, st);
}

template <bool C2R>
int rfft_any(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_fft_desc& d, int in_dtype, int out_dtype,
             const Batch& b, const RfftPlan& p, char* w, hipStream_t st) {
  if (in_dtype == CPLXAMD_F64) return rfft_t<double, double, double, C2R>(xr, xi, yr, yi, d, b, p, w, st);
  if (in_dtype == CPLXAMD_BF16)
    return out_dtype == CPLXAMD_BF16 ? rfft_t<bf16_t, bf16_t, float, C2R>(xr, xi, yr, yi, d, b, p, w, st)
                                     : rfft_t<bf16_t, float, float, C2R>(xr, xi, yr, yi, d, b, p, w, st);
  return out_dtype == CPLXAMD_BF16 ? rfft_t<float, bf16_t, float, C2R>(xr, xi, yr, yi, d, b, p, w, st)
                                   : rfft_t<float, float, float, C2R>(xr, xi, yr, yi, d, b, p, w, st);
}

}  // namespace sp
}  // namespace cplxamd
