// The first-order recurrence with a coefficient per step on a time-parallel scan kernel: the plan, the chunk loader and
// the kernel of scan.hip (which describes them).  The batch runs are runs.h's.
#pragma once
#include "fft_engine.h"
#include "runs.h"

namespace cplxamd {
namespace sp {

constexpr int kScanThreads = 256;                          // four waves per workgroup
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int64_t kScanLenMax = 1ll << 40;
constexpr int64_t kScanFill = 256;                         // workgroups below which the chip counts as not filled
constexpr int64_t kScanSplitGrid = 1024;                   // workgroups the split path aims at (DESIGN 22's figure)
constexpr int64_t kScanSplitTiles = 4;                     // a row is cut only when it has that many tiles

// steps per chunk: a and x of a chunk stay in VGPRs (complex float32: 4 x 16 = 64 registers; complex float64: 4 x 8 x 2)
template <typename T> struct ScanChunk { static constexpr int L = sizeof(T) == 8 ? 8 : 16; };

struct ScanPlan {
  int column;
  int64_t chunk, tile, tiles, segments, seg_len, window, lds, threads, grid, ws, units, channels, cblocks;
};

// the runs of a scan descriptor: a, x, y in ConvRuns' three columns, h0's strides next to them
struct ScanRuns {
  ConvRuns r;
  int64_t hs[3];
};

inline int scan_decode(const cplxamd_scan_desc& d, ScanRuns& s) {
  using D = cplxamd_scan_desc;
  const RunStride<D> f[] = {{&D::a_stride, s.r.as}, {&D::x_stride, s.r.bs}, {&D::h_stride, s.hs}, {&D::y_stride, s.r.ys}};
  return decode_runs(d, f, s.r.size, s.r.rows);
}

// The plan of one call, from the strides alone.  Column plan: time is strided in the result and the innermost run has
// stride 1 in x and the result and stride 1 or 0 in a -- lanes lie along that run.  Row plan: time has stride 1 in the
// result (x and a may step along time by any element stride: they are then read one element per load).
inline int scan_plan_for(const cplxamd_scan_desc& d, const ScanRuns& s, int dtype, int cplx, ScanPlan& p) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (d.n < 1 || d.force_segments < 0 || d.a_es < 0 || d.x_es < 0 || d.y_es < 1 || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (d.n > kScanLenMax) return CPLXAMD_ESHAPE;
  p = ScanPlan{};
  const int64_t word = dtype == CPLXAMD_F64 ? 8 : 4, nc = cplx ? 4 : 2;
  p.chunk = dtype == CPLXAMD_F64 ? 8 : 16;
  p.threads = kScanThreads;
  p.column = d.y_es != 1 && d.runs >= 1 && s.r.bs[2] == 1 && s.r.ys[2] == 1 && (s.r.as[2] == 0 || s.r.as[2] == 1);
  if (!p.column && d.y_es != 1) return CPLXAMD_EINVAL;
  p.channels = p.column ? s.r.size[2] : 1;
  p.cblocks = ceil_div(p.channels, kWave);
  p.tile = p.chunk * (p.column ? kScanWaves : kScanThreads);
  p.tiles = ceil_div(d.n, p.tile);
  if (p.column) {
    if (__builtin_mul_overflow(s.r.size[0] * s.r.size[1], p.cblocks, &p.units)) return CPLXAMD_ESHAPE;
  } else {
    p.units = s.r.rows;
  }
  p.seg_len = d.n;
  if (d.force_segments > 0) {
    const int64_t segs = d.force_segments < d.n ? d.force_segments : d.n;
    p.seg_len = ceil_div(d.n, segs);
  } else if (p.units > 0 && p.units < kScanFill && p.tiles >= kScanSplitTiles) {
    // few rows: segments of whole tiles, at least two tiles each, up to kScanSplitGrid workgroups (x and a are read twice)
    int64_t segs = ceil_div(kScanSplitGrid, p.units);
    if (segs > p.tiles / 2) segs = p.tiles / 2;
    p.seg_len = ceil_div(p.tiles, segs) * p.tile;
  }
  p.segments = ceil_div(d.n, p.seg_len);
  p.window = p.segments > 1 ? p.seg_len : (d.n < p.tile ? d.n : p.tile);
  if (__builtin_mul_overflow(p.units, p.segments, &p.grid) || p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  const int64_t lw = p.column ? kWave : 1;
  p.lds = 2 * kScanWaves * nc * lw * word;
  p.ws = p.units * (p.segments - 1) * nc * lw * word;
  return 0;
}

template <typename TI, typename T>
struct ScanIo {
  const TI* ar; const TI* ai; const TI* xr; const TI* xi; const TI* hr; const TI* hi; TI* yr; TI* yi; T* ws;
  int64_t n, segs, seg_len, a_es, x_es, y_es;
  Sub ax, hy;                                             // (a, x) and (h0, y) strides of the rows
  int64_t channels, cblocks, a_cs, h_cs;                  // column plan: the lanes' run
  bool rev, conj, lag, pairs;
};

template <typename TI, typename T> __device__ __forceinline__ TI scan_cvt(T v);
template <> __device__ __forceinline__ float scan_cvt<float, float>(float v) { return v; }
template <> __device__ __forceinline__ double scan_cvt<double, double>(double v) { return v; }
template <> __device__ __forceinline__ bf16_t scan_cvt<bf16_t, float>(float v) { return f32_to_bf16(v); }

// One chunk of a plane into registers, out[q] for processing step p0 + q (q < cnt; `pad` behind the chunk's end).  Step
// p lies at sample p, or n - 1 - p in reverse; with `shift` (the lag flag's coefficients) out[q] is the value of step
// p0 + q - 1, and zero for the step before the row's first: no address outside the plane is formed.  A full chunk of
// stride 1 is read as 16-byte vectors when its first byte allows it (the same answer for every lane of the row: chunks
// lie a multiple of 16 bytes apart), anything else one element per load, predicated.
template <typename TI, typename T, int L, bool COL>
__device__ __forceinline__ void scan_load(const TI* p, int64_t base, int64_t es, int64_t n, bool rev, int64_t p0, int cnt,
                                          bool shift, T pad, T (&out)[L]) {
  constexpr int V = 16 / (int)sizeof(TI);
  if constexpr (!COL) {
    const TI* blk = p + base + (rev ? n - p0 - L : p0);
    if (cnt == L && es == 1 && ((uintptr_t)blk & 15) == 0) {
      T mem[L];
#pragma unroll
      for (int v = 0; v < L / V; ++v) {
        const uint4 w = *reinterpret_cast<const uint4*>(blk + v * V);
        TI e[V];
        __builtin_memcpy(e, &w, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) mem[v * V + k] = (T)ld<TI>::at(&e[k]);
      }
      T first = 0;
      if (shift && p0 > 0) first = (T)ld<TI>::at(p + base + (rev ? n - p0 : p0 - 1));
#pragma unroll
      for (int q = 0; q < L; ++q) {
        const T here = rev ? mem[L - 1 - q] : mem[q];
        const T before = q == 0 ? first : (rev ? mem[L - q] : mem[q - 1]);
        out[q] = shift ? before : here;
      }
      return;
    }
  }
  T one = 0;
  if (es == 0 && cnt > 0) one = (T)ld<TI>::at(p + base);
#pragma unroll
  for (int q = 0; q < L; ++q) {
    const int64_t pp = p0 + q - (shift ? 1 : 0);
    T v = pad;
    if (q < cnt) {
      v = 0;
      if (pp >= 0) v = es == 0 ? one : (T)ld<TI>::at(p + base + (rev ? n - 1 - pp : pp) * es);
    }
    out[q] = v;
  }
}

template <typename TI, typename T, int L, bool COL>
__device__ __forceinline__ void scan_store(TI* p, int64_t base, int64_t es, int64_t n, bool rev, int64_t p0, int cnt,
                                           const T (&in)[L]) {
  constexpr int V = 16 / (int)sizeof(TI);
  if constexpr (!COL) {
    TI* blk = p + base + (rev ? n - p0 - L : p0);
    if (cnt == L && es == 1 && ((uintptr_t)blk & 15) == 0) {
#pragma unroll
      for (int v = 0; v < L / V; ++v) {
        TI e[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int j = v * V + k;
          e[k] = scan_cvt<TI, T>(rev ? in[L - 1 - j] : in[j]);
        }
        uint4 w;
        __builtin_memcpy(&w, e, 16);
        *reinterpret_cast<uint4*>(blk + v * V) = w;
      }
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < L; ++q)
    if (q < cnt) {
      const int64_t pp = p0 + q;
      st_t(p + base + (rev ? n - 1 - pp : pp) * es, in[q]);
    }
}

// (P, s): the map h -> P h + s of a run of steps.  `later` after `first`: (P2 P1, P2 s1 + s2).
template <typename T> struct ScanMap { T pr, pi, sr, si; };

template <bool CX, typename T>
__device__ __forceinline__ void scan_step(T& hr, T& hi, T ar, T ai, T xr, T xi) {   // h = a h + x
  if constexpr (CX) {
    const T nr = ar * hr - ai * hi + xr, ni = ar * hi + ai * hr + xi;
    hr = nr, hi = ni;
  } else {
    hr = ar * hr + xr;
  }
}
template <bool CX, typename T>
__device__ __forceinline__ void scan_mul(T& pr, T& pi, T ar, T ai) {                 // p = a p
  if constexpr (CX) {
    const T nr = ar * pr - ai * pi, ni = ar * pi + ai * pr;
    pr = nr, pi = ni;
  } else {
    pr = ar * pr;
  }
}
template <bool CX, typename T>
__device__ __forceinline__ ScanMap<T> scan_after(const ScanMap<T>& later, ScanMap<T> first) {
  scan_step<CX>(first.sr, first.si, later.pr, later.pi, later.sr, later.si);
  scan_mul<CX>(first.pr, first.pi, later.pr, later.pi);
  return first;
}
template <bool CX, typename T>
__device__ __forceinline__ ScanMap<T> scan_shfl_up(const ScanMap<T>& m, int by) {
  ScanMap<T> o{__shfl_up(m.pr, by, kWave), (T)0, __shfl_up(m.sr, by, kWave), (T)0};
  if constexpr (CX) o.pi = __shfl_up(m.pi, by, kWave), o.si = __shfl_up(m.si, by, kWave);
  return o;
}

// Workgroup (unit, segment); a unit is a row (row plan: thread c owns chunk c of every tile of 256 L steps) or 64
// channels of a row (column plan: lane l owns channel l, wave w chunk w of every tile of 4 L steps).  `pairs`: the
// split path's first launch -- phases 1 and 2 only, from zero state, and the segment's map (P, s) into ws; its grid
// leaves out the last segment of every unit, whose map nobody reads.
template <typename TI, typename T, bool CX, bool COL>
__global__ __launch_bounds__(kScanThreads) void scan_chunks(ScanIo<TI, T> g) {
  constexpr int L = ScanChunk<T>::L, NC = CX ? 4 : 2, LW = COL ? kWave : 1;
  constexpr int TL = L * (COL ? kScanWaves : kScanThreads);
  __shared__ T tot[2][kScanWaves][NC][LW];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, wl = COL ? lane : 0;
  const int64_t nseg = g.pairs ? g.segs - 1 : g.segs;
  const int64_t seg = blockIdx.x % nseg, unit = blockIdx.x / nseg;
  int64_t row = unit, ao, xo, ho, yo;
  bool live = true;
  if constexpr (COL) row = unit / g.cblocks;
  sub_offsets(g.ax, row, ao, xo);
  sub_offsets(g.hy, row, ho, yo);
  if constexpr (COL) {
    const int64_t ch = (unit - row * g.cblocks) * kWave + lane;
    live = ch < g.channels;
    const int64_t c = live ? ch : 0;
    ao += c * g.a_cs, xo += c, ho += c * g.h_cs, yo += c;
  }
  // ---- the state that enters the segment: h0 run through the maps of the segments before this one, in order
  ScanMap<T> carry{(T)1, (T)0, (T)0, (T)0};
  if (!g.pairs) {
    if (g.hr && live) {
      carry.sr = (T)ld<TI>::at(g.hr + ho);
      if constexpr (CX) carry.si = g.hi ? (T)ld<TI>::at(g.hi + ho) : (T)0;
    }
    const T* w = g.ws + (unit * (g.segs - 1) * NC) * LW + wl;
    for (int64_t j = 0; j < seg; ++j, w += NC * LW) {
      const T pr = w[0], sr = w[LW], pi = CX ? w[2 * LW] : (T)0, si = CX ? w[3 * LW] : (T)0;
      scan_step<CX>(carry.sr, carry.si, pr, pi, sr, si);
    }
  }
  // ---- the segment's tiles, in order
  const int64_t t_begin = seg * g.seg_len, t_end = t_begin + g.seg_len < g.n ? t_begin + g.seg_len : g.n;
  int par = 0;
  for (int64_t t0 = t_begin; t0 < t_end; t0 += TL, par ^= 1) {
    const int64_t p0 = t0 + (int64_t)(COL ? wave : tid) * L, left = t_end - p0;
    const int cnt = !live || left <= 0 ? 0 : (left > L ? L : (int)left);
    T Ar[L], Ai[L], Xr[L], Xi[L];
    scan_load<TI, T, L, COL>(g.ar, ao, g.a_es, g.n, g.rev, p0, cnt, g.lag, (T)1, Ar);
    if constexpr (CX) {
      if (g.ai) {
        scan_load<TI, T, L, COL>(g.ai, ao, g.a_es, g.n, g.rev, p0, cnt, g.lag, (T)0, Ai);
        if (g.conj) {
#pragma unroll
          for (int q = 0; q < L; ++q) Ai[q] = -Ai[q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < L; ++q) Ai[q] = 0;
      }
    }
    if (g.xr) {
      scan_load<TI, T, L, COL>(g.xr, xo, g.x_es, g.n, g.rev, p0, cnt, false, (T)0, Xr);
    } else {
#pragma unroll
      for (int q = 0; q < L; ++q) Xr[q] = 0;
    }
    if constexpr (CX) {
      if (g.xi) {
        scan_load<TI, T, L, COL>(g.xi, xo, g.x_es, g.n, g.rev, p0, cnt, false, (T)0, Xi);
      } else {
#pragma unroll
        for (int q = 0; q < L; ++q) Xi[q] = 0;
      }
    }
    // 1. the chunk from zero state: its coefficient product and its local final state (a step behind the chunk's end
    //    has a = 1, x = 0 and changes neither)
    ScanMap<T> m{(T)1, (T)0, (T)0, (T)0};
#pragma unroll
    for (int q = 0; q < L; ++q) {
      scan_step<CX>(m.sr, m.si, Ar[q], CX ? Ai[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
      scan_mul<CX>(m.pr, m.pi, Ar[q], CX ? Ai[q] : (T)0);
    }
    // 2. the maps in order.  Row plan: an inclusive scan over the lanes of the wave, log depth; then both plans: the
    //    waves' totals through LDS, taken in order by every thread (tot is double-buffered: one barrier per tile)
    if constexpr (!COL) {
#pragma unroll
      for (int by = 1; by < kWave; by <<= 1) {
        const ScanMap<T> prev = scan_shfl_up<CX>(m, by);
        if (lane >= by) m = scan_after<CX>(m, prev);
      }
    }
    if (COL || lane == kWave - 1) {
      tot[par][wave][0][wl] = m.pr, tot[par][wave][1][wl] = m.sr;
      if constexpr (CX) tot[par][wave][2][wl] = m.pi, tot[par][wave][3][wl] = m.si;
    }
    __syncthreads();
    ScanMap<T> enter = carry;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
      if (w == wave) enter = carry;
      const ScanMap<T> t{tot[par][w][0][wl], CX ? tot[par][w][2][wl] : (T)0, tot[par][w][1][wl], CX ? tot[par][w][3][wl] : (T)0};
      carry = scan_after<CX>(t, carry);
    }
    if (g.pairs) continue;
    // 3. the chunk again, from its true entering state, and the store
    T hr = enter.sr, hi = enter.si;
    if constexpr (!COL) {
      const ScanMap<T> prev = scan_shfl_up<CX>(m, 1);
      if (lane > 0) scan_step<CX>(hr, hi, prev.pr, prev.pi, prev.sr, prev.si);
    }
#pragma unroll
    for (int q = 0; q < L; ++q) {
      scan_step<CX>(hr, hi, Ar[q], CX ? Ai[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
      Xr[q] = hr;
      if constexpr (CX) Xi[q] = hi;
    }
    scan_store<TI, T, L, COL>(g.yr, yo, g.y_es, g.n, g.rev, p0, cnt, Xr);
    if constexpr (CX) scan_store<TI, T, L, COL>(g.yi, yo, g.y_es, g.n, g.rev, p0, cnt, Xi);
  }
  if (g.pairs && wave == 0 && (COL || lane == 0)) {
    T* w = g.ws + ((unit * (g.segs - 1) + seg) * NC) * LW + wl;
    w[0] = carry.pr, w[LW] = carry.sr;
    if constexpr (CX) w[2 * LW] = carry.pi, w[3 * LW] = carry.si;
  }
}

}  // namespace sp
}  // namespace cplxamd
