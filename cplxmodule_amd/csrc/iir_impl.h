// Recursive filtering on a chunk-parallel kernel: the plan, the kernels and the checks of iir.hip (which describes
// them).  The batch runs are runs.h's.
#pragma once
#include "fft_engine.h"
#include "runs.h"

namespace cplxamd {
namespace sp {

constexpr int64_t kIirLdsBudget = 76 << 10;               // bytes per workgroup: two workgroups in a CU's 160 KiB
constexpr int kIirLanes = 64;                             // chunks per tile: one per thread, one wave per workgroup
constexpr int kIirMaxOrder = 8;
constexpr int kIirMaxSections = 16;                       // per launch; the caller chains longer cascades
constexpr int64_t kIirLenMax = 1ll << 40;
constexpr int64_t kIirFill = 1024;                        // one-wave workgroups that fill the chip: four per CU
constexpr int kIirScanWidth = 32;                         // sections * order of the split path's state

template <typename T> struct IirChunk { static constexpr int kLog = sizeof(T) == 8 ? 5 : 6; };

struct IirPlan {
  int path;
  int64_t chunk, lanes, tile, tiles, segments, seg_len, bucket, lds, threads, grid, ws;
};

// words of one workgroup: the padded tile, the lanes' states, the carried states and the per-section tables
// (coefficients, `bucket` zero-input responses of `chunk` samples, the chunk transition)
inline int64_t iir_table_words(int64_t bucket, int64_t chunk) {
  return 2 * (bucket + 1) + bucket * chunk + bucket * bucket;
}
inline int64_t iir_lds_words(int64_t bucket, int64_t chunk, int64_t sections, int planes) {
  const int64_t tile = chunk * kIirLanes;
  return planes * (tile + kIirLanes + 1 + bucket * kIirLanes + sections * bucket + sections * iir_table_words(bucket, chunk));
}

inline int iir_plan_for(int64_t n, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype, int cplx,
                        int64_t force, IirPlan& p) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (n < 1 || rows < 0 || filters < 0 || force < 0 || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (sections < 1 || sections > kIirMaxSections || order < 1 || order > (sections == 1 ? kIirMaxOrder : 2))
    return CPLXAMD_EINVAL;
  if (n > kIirLenMax) return CPLXAMD_ESHAPE;
  p = IirPlan{};
  const int64_t word = dtype == CPLXAMD_F64 ? 8 : 4;
  p.chunk = dtype == CPLXAMD_F64 ? 32 : 64;
  p.lanes = kIirLanes;
  p.tile = p.chunk * p.lanes;
  p.bucket = order > 2 ? 8 : 2;
  p.threads = kIirLanes;
  p.lds = iir_lds_words(p.bucket, p.chunk, sections, cplx ? 2 : 1) * word;
  if (p.lds > kIirLdsBudget) return CPLXAMD_ESHAPE;
  int64_t segs = 1;
  p.seg_len = n;
  if (force > 0) {
    segs = force < n ? force : n;
    p.seg_len = ceil_div(n, segs);
  } else if (rows > 0 && rows * (p.bucket == 8 ? 8 : 2) <= kIirFill && sections * order <= kIirScanWidth) {
    // few rows (the split path reads x twice: it has to win more than that): segments of whole tiles, at least two tiles
    // each, up to kIirFill workgroups.  Measured (profiles/iir_bench.txt): at 256 rows of 65536 samples the split wins by
    // 1.3-1.7 x with two states per section and LOSES by 1.25 x with eight, so the wider kernel splits below 129 rows only
    // (between 129 and 256 rows it was not measured)
    segs = ceil_div(kIirFill, rows);
    if (segs > n / (2 * p.tile)) segs = n / (2 * p.tile);
    if (segs < 2) segs = 1;
    p.seg_len = ceil_div(ceil_div(n, segs), p.tile) * p.tile;
  }
  p.segments = ceil_div(n, p.seg_len);
  p.path = p.segments > 1 ? CPLXAMD_IIR_SPLIT : CPLXAMD_IIR_ROW;
  p.tiles = ceil_div(p.seg_len, p.tile);
  if (__builtin_mul_overflow(rows, p.segments, &p.grid) || p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  const int64_t w = sections * order;
  p.ws = p.path == CPLXAMD_IIR_SPLIT ? (cplx ? 2 : 1) * word * (3 * p.grid * w + 2 * filters * w * w) : 0;
  return 0;
}

// TO, TC: the element types of y and of the coefficients (the extended pass of filtfilt.hip: they differ from x's)
template <typename TI, typename T, typename TO = TI, typename TC = TI>
struct IirIo {
  const TI* xr; const TI* xi; const TC* cr; const TC* ci; const T* zr; const T* zi; TO* yr; TO* yi; T* fr; T* fi;
  int64_t n, segs, seg_len, x_es;
  Sub xy, c;                                              // (x, y) strides; c.p: the coefficients', c.q: the unit state's
  int D, S;
  bool rev, conj;
  // the extended pass only (EXT): the row has n + 2 edge logical samples, [y_lo, y_lo + y_n) of them are stored
  int64_t edge, y_lo, y_n;
  int mode;
  bool scale;
};

// ---- the edge extension's index map: the same code on the host (cplxamd_filtfilt_src, the host tests) and in the kernel
// Logical sample m of a row of n samples extended by e < n samples on each side is
//   k < 0: x[j];   j < 0: x[k];   else 2 x[k] - x[j]
// with k an anchor (0 or n - 1).  ODD: the row reflected through its end points, EVEN: mirrored about them, CONSTANT:
// the end points repeated.  m outside [0, n + 2 e): j = k = -1.
struct IirSrc { int64_t j, k; };
__host__ __device__ __forceinline__ IirSrc iir_ext_src(int64_t m, int64_t n, int64_t e, int mode) {
  if (m < 0 || m >= n + 2 * e) return {-1, -1};
  const int64_t i = m - e;
  if (i >= 0 && i < n) return {i, -1};
  const int64_t k = i < 0 ? 0 : n - 1, j = i < 0 ? -i : 2 * (n - 1) - i;
  if (mode == CPLXAMD_FILTFILT_CONSTANT) return {-1, k};
  return {j, mode == CPLXAMD_FILTFILT_ODD ? k : -1};
}

// lane `lane`'s value in every lane (lane is uniform; every lane of the wave is active)
__device__ __forceinline__ float wave_bcast(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ double wave_bcast(double v, int lane) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <bool CX, typename T>
__device__ __forceinline__ void iir_mac(T& re, T& im, T ar, T ai, T br, T bi) {   // += a b
  if constexpr (CX) {
    re += ar * br - ai * bi;
    im += ar * bi + ai * br;
  } else {
    re += ar * br;
  }
}
template <bool CX, typename T>
__device__ __forceinline__ void iir_msub(T& re, T& im, T ar, T ai, T br, T bi) {  // -= a b
  if constexpr (CX) {
    re -= ar * br - ai * bi;
    im -= ar * bi + ai * br;
  } else {
    re -= ar * br;
  }
}

// Workgroup (row, segment); thread c owns chunk c of every tile: samples [c L, c L + L) of the tile, L = 2^kLog.
// LDS, per plane (im follows re at a distance of `plane` words): the tile at i + (i >> kLog) (one word per chunk: lanes
// step L + 1 words, no two lanes of the wave share a bank), the lanes' states [d][lane], the carried states [s][d], then
// per section the coefficients b0..b_DK a0..a_DK, the zero-input responses [d][j] and M = A^L [i][k].
// EXT (filtfilt.hip) adds, as compile-time policy of the one body: the loader that forms the edge extension from x where it
// lies (the two anchors x[0], x[n - 1] are fetched once per workgroup into two words per plane behind the tables), the
// entering state as a unit state [S][D] per filter times the first sample in processing order, and the windowed store.
template <typename TI, typename T, bool CX, int DK, typename TO = TI, typename TC = TI, bool EXT = false>
__global__ __launch_bounds__(kIirLanes) void iir_chunks(IirIo<TI, T, TO, TC> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int kLog = IirChunk<T>::kLog, L = 1 << kLog, TL = L * kIirLanes;
  constexpr int kCo = 2 * (DK + 1), kTab = kCo + DK * L + DK * DK;
  const int tid = threadIdx.x, S = g.S, D = g.D;
  const int plane = TL + kIirLanes + 1 + DK * kIirLanes + S * DK + S * kTab + (EXT ? 2 : 0);
  T* tile = (T*)smem;
  T* st = tile + TL + kIirLanes + 1;
  T* carry = st + DK * kIirLanes;
  T* tab = carry + S * DK;
  auto IM = [&](T* p) { return p + plane; };
  const int64_t row = blockIdx.x / g.segs, seg = blockIdx.x - row * g.segs;
  int64_t xo, yo, co, zo;
  sub_offsets(g.xy, row, xo, yo);
  sub_offsets(g.c, row, co, zo);
  const int64_t nlog = EXT ? g.n + 2 * g.edge : g.n;      // samples of the row as the recurrence sees it
  T* anc = tab + S * kTab;                                // EXT: x[0], x[n - 1]
  // EXT: logical sample m through the index map (after the barrier that publishes the anchors)
  auto ext_at = [&](int64_t m, T& re, T& im) {
    const IirSrc s = iir_ext_src(m, g.n, g.edge, g.mode);
    T vr = 0, vi = 0;
    if (s.j >= 0) {
      vr = g.xr ? (T)ld<TI>::at(g.xr + xo + s.j * g.x_es) : (T)0;
      if constexpr (CX) vi = g.xi ? (T)ld<TI>::at(g.xi + xo + s.j * g.x_es) : (T)0;
    }
    if (s.k >= 0) {
      const int w = s.k != 0;
      const T ar = anc[w], ai = CX ? *IM(anc + w) : (T)0;
      vr = s.j >= 0 ? 2 * ar - vr : ar;
      vi = s.j >= 0 ? 2 * ai - vi : ai;
    }
    re = vr, im = vi;
  };
  if constexpr (EXT) {
    if (tid < 2) {
      const int64_t at = xo + (tid ? g.n - 1 : 0) * g.x_es;
      anc[tid] = g.xr ? (T)ld<TI>::at(g.xr + at) : (T)0;
      if constexpr (CX) *IM(anc + tid) = g.xi ? (T)ld<TI>::at(g.xi + at) : (T)0;
    }
  }
  // ---- the coefficients, zero-padded to DK states
  for (int e = tid; e < S * kCo; e += kIirLanes) {
    const int s = e / kCo, k = e - s * kCo, which = k / (DK + 1), kk = k - which * (DK + 1);
    const bool in = kk <= D;
    const int64_t at = co + (int64_t)s * 2 * (D + 1) + which * (D + 1) + kk;
    T* dst = tab + s * kTab + k;
    *dst = in ? (T)ld<TC>::at(g.cr + at) : (T)0;
    if constexpr (CX) *IM(dst) = in && g.ci ? (g.conj ? -(T)ld<TC>::at(g.ci + at) : (T)ld<TC>::at(g.ci + at)) : (T)0;
  }
  __syncthreads();
  // ---- zero-input response j of section s over one chunk; its final state is column j of M
  if (tid < S * DK) {
    const int s = tid / DK, j = tid - s * DK;
    const T* a = tab + s * kTab + DK + 1;
    T* zir = tab + s * kTab + kCo + j * L;
    T* pw = tab + s * kTab + kCo + DK * L;
    T zr[DK], zi[DK];
#pragma unroll
    for (int i = 0; i < DK; ++i) zr[i] = i == j ? (T)1 : (T)0, zi[i] = 0;
    for (int q = 0; q < L; ++q) {
      const T yr = zr[0], yi = zi[0];
      zir[q] = yr;
      if constexpr (CX) *IM(zir + q) = yi;
#pragma unroll
      for (int i = 0; i < DK; ++i) {
        T nr = i + 1 < DK ? zr[i + 1] : (T)0, ni = i + 1 < DK ? zi[i + 1] : (T)0;
        iir_msub<CX>(nr, ni, a[i + 1], CX ? *IM(const_cast<T*>(a) + i + 1) : (T)0, yr, yi);
        zr[i] = nr, zi[i] = ni;
      }
    }
#pragma unroll
    for (int i = 0; i < DK; ++i) {
      pw[i * DK + j] = zr[i];
      if constexpr (CX) *IM(pw + i * DK + j) = zi[i];
    }
    // the carried state of (row, segment)
    const bool has = j < D && g.zr;
    const bool in = has && !(EXT && g.scale);             // (a scaled state is not laid out per row: see below)
    const int64_t at = ((row * g.segs + seg) * S + s) * D + j;
    carry[tid] = in ? g.zr[at] : (T)0;
    if constexpr (CX) *IM(carry + tid) = in && g.zi ? g.zi[at] : (T)0;
    if constexpr (EXT) {
      if (g.scale) {                                      // the unit state of the row's filter times the first sample
        const int64_t ua = zo + (int64_t)s * D + j;
        const T ur = has ? g.zr[ua] : (T)0, ui = CX && has && g.zi ? g.zi[ua] : (T)0;
        T fr, fi, pr = 0, pi = 0;
        ext_at(g.rev ? nlog - 1 : 0, fr, fi);
        iir_mac<CX>(pr, pi, ur, ui, fr, fi);
        carry[tid] = pr;
        if constexpr (CX) *IM(carry + tid) = pi;
      }
    }
  }
  __syncthreads();
  // ---- the segment's tiles, in order
  const int64_t t_begin = seg * g.seg_len, t_end = t_begin + g.seg_len < nlog ? t_begin + g.seg_len : nlog;
  const int base = tid * (L + 1);                         // tid L + q + ((tid L + q) >> kLog) = base + q for q < L
  for (int64_t t0 = t_begin; t0 < t_end; t0 += TL) {
    const int cnt = t_end - t0 < TL ? (int)(t_end - t0) : TL;
    for (int p = tid; p < cnt; p += kIirLanes) {
      const int64_t m = g.rev ? nlog - 1 - (t0 + p) : t0 + p;
      const int at = p + (p >> kLog);
      if constexpr (EXT) {
        T vr, vi;
        ext_at(m, vr, vi);
        tile[at] = vr;
        if constexpr (CX) *IM(tile + at) = vi;
      } else {
        tile[at] = g.xr ? (T)ld<TI>::at(g.xr + xo + m * g.x_es) : (T)0;
        if constexpr (CX) *IM(tile + at) = g.xi ? (T)ld<TI>::at(g.xi + xo + m * g.x_es) : (T)0;
      }
    }
    __syncthreads();
    const int nl = (cnt + L - 1) >> kLog;                 // lanes with samples
    int nv = cnt - tid * L;
    nv = nv < 0 ? 0 : (nv > L ? L : nv);
    for (int s = 0; s < S; ++s) {
      const T* co_s = tab + s * kTab;
      const T* zir = co_s + kCo;
      const T* pw = zir + DK * L;
      T br[DK + 1], bi[DK + 1], ar[DK + 1], ai[DK + 1];
#pragma unroll
      for (int i = 0; i <= DK; ++i) {
        br[i] = co_s[i], ar[i] = co_s[DK + 1 + i];
        bi[i] = CX ? *IM(const_cast<T*>(co_s) + i) : (T)0;
        ai[i] = CX ? *IM(const_cast<T*>(co_s) + DK + 1 + i) : (T)0;
      }
      T zr[DK], zi[DK], lr[DK], li[DK];
#pragma unroll
      for (int i = 0; i < DK; ++i) {
        zr[i] = tid == 0 ? carry[s * DK + i] : (T)0;
        zi[i] = CX && tid == 0 ? *IM(carry + s * DK + i) : (T)0;
      }
      // the chunk from zero state (lane 0: from the carried state)
      for (int q = 0; q < nv; ++q) {
        const T xr = tile[base + q], xi = CX ? *IM(tile + base + q) : (T)0;
        T yr = zr[0], yi = zi[0];
        iir_mac<CX>(yr, yi, br[0], bi[0], xr, xi);
#pragma unroll
        for (int i = 0; i < DK; ++i) {
          T nr = i + 1 < DK ? zr[i + 1] : (T)0, ni = i + 1 < DK ? zi[i + 1] : (T)0;
          iir_mac<CX>(nr, ni, br[i + 1], bi[i + 1], xr, xi);
          iir_msub<CX>(nr, ni, ar[i + 1], ai[i + 1], yr, yi);
          zr[i] = nr, zi[i] = ni;
        }
        tile[base + q] = yr;
        if constexpr (CX) *IM(tile + base + q) = yi;
      }
#pragma unroll
      for (int i = 0; i < DK; ++i) {
        lr[i] = zr[i], li[i] = zi[i];
        st[i * kIirLanes + tid] = zr[i];
        if constexpr (CX) *IM(st + i * kIirLanes + tid) = zi[i];
      }
      __syncthreads();
      // the states at the chunk ends, P_c = M P_{c-1} + s_c, in order: lane i < DK carries component i, the components
      // travel between the lanes through scalar registers (the workgroup is one wave), s_{c+1} is fetched a step ahead
      {
        const int ii = tid < DK ? tid : 0;
        T mr[DK], mi[DK];
#pragma unroll
        for (int k = 0; k < DK; ++k) mr[k] = pw[ii * DK + k], mi[k] = CX ? *IM(const_cast<T*>(pw) + ii * DK + k) : (T)0;
        T cr = st[ii * kIirLanes], ci = CX ? *IM(st + ii * kIirLanes) : (T)0;
        T nr = nl > 1 ? st[ii * kIirLanes + 1] : (T)0, ni = CX && nl > 1 ? *IM(st + ii * kIirLanes + 1) : (T)0;
        for (int c = 1; c < nl; ++c) {
          T ar_ = nr, ai_ = ni;
          if (c + 1 < nl) {
            nr = st[ii * kIirLanes + c + 1];
            if constexpr (CX) ni = *IM(st + ii * kIirLanes + c + 1);
          }
#pragma unroll
          for (int k = 0; k < DK; ++k) iir_mac<CX>(ar_, ai_, mr[k], mi[k], wave_bcast(cr, k), CX ? wave_bcast(ci, k) : (T)0);
          cr = ar_, ci = ai_;
          if (tid < DK) {
            st[tid * kIirLanes + c] = cr;
            if constexpr (CX) *IM(st + tid * kIirLanes + c) = ci;
          }
        }
      }
      __syncthreads();
      if (tid == nl - 1 && nv == L) {                     // a full last chunk: its scanned state is the tile's
#pragma unroll
        for (int i = 0; i < DK; ++i) {
          zr[i] = st[i * kIirLanes + tid];
          zi[i] = CX ? *IM(st + i * kIirLanes + tid) : (T)0;
        }
      }
      // the entering state of the chunk: the scanned state of the lane before; its zero-input response corrects the chunk
      if (tid > 0 && nv > 0) {
        T er[DK], ei[DK];
#pragma unroll
        for (int i = 0; i < DK; ++i) {
          er[i] = st[i * kIirLanes + tid - 1];
          ei[i] = CX ? *IM(st + i * kIirLanes + tid - 1) : (T)0;
        }
        for (int q = 0; q < nv; ++q) {
          T yr = tile[base + q], yi = CX ? *IM(tile + base + q) : (T)0;
#pragma unroll
          for (int i = 0; i < DK; ++i)
            iir_mac<CX>(yr, yi, zir[i * L + q], CX ? *IM(const_cast<T*>(zir) + i * L + q) : (T)0, er[i], ei[i]);
          tile[base + q] = yr;
          if constexpr (CX) *IM(tile + base + q) = yi;
        }
        if (tid == nl - 1 && nv < L) {                    // a part chunk ends the tile: its own final state
          for (int q = 0; q < nv; ++q) {
            const T yr = er[0], yi = ei[0];
#pragma unroll
            for (int i = 0; i < DK; ++i) {
              T nr = i + 1 < DK ? er[i + 1] : (T)0, ni = i + 1 < DK ? ei[i + 1] : (T)0;
              iir_msub<CX>(nr, ni, ar[i + 1], ai[i + 1], yr, yi);
              er[i] = nr, ei[i] = ni;
            }
          }
#pragma unroll
          for (int i = 0; i < DK; ++i) zr[i] = lr[i] + er[i], zi[i] = li[i] + ei[i];
        }
      }
      if (tid == nl - 1) {                                // (lane 0's chunk ran from the carried state itself)
#pragma unroll
        for (int i = 0; i < DK; ++i) {
          carry[s * DK + i] = zr[i];
          if constexpr (CX) *IM(carry + s * DK + i) = zi[i];
        }
      }
      __syncthreads();
    }
    if (g.yr) {
      for (int p = tid; p < cnt; p += kIirLanes) {
        const int64_t m = g.rev ? nlog - 1 - (t0 + p) : t0 + p;
        const int at = p + (p >> kLog);
        if constexpr (EXT) {
          if (m < g.y_lo || m >= g.y_lo + g.y_n) continue;   // only the window is kept
          st_t(g.yr + yo + (m - g.y_lo), tile[at]);
          if constexpr (CX) st_t(g.yi + yo + (m - g.y_lo), *IM(tile + at));
        } else {
          st_t(g.yr + yo + m, tile[at]);
          if constexpr (CX) st_t(g.yi + yo + m, *IM(tile + at));
        }
      }
    }
    __syncthreads();
  }
  if (g.fr && tid < S * DK) {
    const int s = tid / DK, j = tid - s * DK;
    if (j < D) {
      const int64_t at = ((row * g.segs + seg) * S + s) * D + j;
      g.fr[at] = carry[tid];
      if constexpr (CX) g.fi[at] = *IM(carry + tid);
    }
  }
}

// the split path's scan: thread r walks the segments of row r
template <typename T, bool CX>
__global__ __launch_bounds__(kET) void iir_scan(const T* zr, const T* zi, const T* mr, const T* mi, const T* ir, const T* ii,
                                                T* er, T* ei, int64_t rows, int64_t rpf, int64_t segs, int w) {
  const int64_t r = (int64_t)blockIdx.x * kET + threadIdx.x;
  if (r >= rows) return;
  const T* Mr = mr + (r / rpf) * w * w;
  const T* Mi = mi ? mi + (r / rpf) * w * w : nullptr;
  T cr[kIirScanWidth], ci[kIirScanWidth], nr[kIirScanWidth], ni[kIirScanWidth];
  for (int i = 0; i < w; ++i) {
    cr[i] = ir ? ir[r * w + i] : (T)0;
    ci[i] = CX && ii ? ii[r * w + i] : (T)0;
  }
  for (int64_t k = 0; k < segs; ++k) {
    const int64_t at = (r * segs + k) * w;
    for (int i = 0; i < w; ++i) {
      er[at + i] = cr[i];
      if constexpr (CX) ei[at + i] = ci[i];
    }
    if (k + 1 == segs) break;
    for (int i = 0; i < w; ++i) {
      T re = zr[at + i], im = CX ? zi[at + i] : (T)0;
      for (int j = 0; j < w; ++j) iir_mac<CX>(re, im, Mr[j * w + i], CX && Mi ? Mi[j * w + i] : (T)0, cr[j], ci[j]);
      nr[i] = re, ni[i] = im;
    }
    for (int i = 0; i < w; ++i) cr[i] = nr[i], ci[i] = ni[i];
  }
}

}  // namespace sp
}  // namespace cplxamd
