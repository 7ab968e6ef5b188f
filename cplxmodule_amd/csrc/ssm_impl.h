// The multi-state diagonal state-space scan: the plan, the chunk loader and the kernel of ssm.hip (which describes
// them).  The maps, their composition and the chunk store are scan_impl.h's; the batch runs are runs.h's.
#pragma once
#include "scan_impl.h"

namespace cplxamd {
#include "cexp.h"
namespace sp {

constexpr int kSsmStatesMax = 256;                         // one carried state per thread of the workgroup
constexpr int kSsmL = 16;                                  // steps per chunk
enum { kSsmConst = 0, kSsmVary = 1, kSsmDt = 2 };          // the coefficient: one value per state, a chunk, exp(dt a)
enum { kSsmA = 0, kSsmB, kSsmC, kSsmX, kSsmD, kSsmH, kSsmY, kSsmF, kSsmPlanes };

// states per group (one barrier each).  A coefficient that varies along time is held for the whole group between phases
// 1 and 3: 2 L registers per complex state, so those instances take two states where the others take four.
constexpr int ssm_group(bool cx, bool vary) { return cx && vary ? 2 : 4; }

struct SsmPlan {
  int64_t chunk, tile, tiles, group, lds, threads, grid, window;
};

inline int ssm_plan_for(int64_t n, int64_t states, int64_t rows, int dtype, int cplx, int vary, SsmPlan& p) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (states < 1 || states > kSsmStatesMax || n < 0 || rows < 0) return CPLXAMD_EINVAL;
  if ((cplx != 0 && cplx != 1) || (vary != 0 && vary != 1)) return CPLXAMD_EINVAL;
  if (n > kScanLenMax || rows > 0x7fffffffll) return CPLXAMD_ESHAPE;
  p.chunk = kSsmL;
  p.tile = kSsmL * kScanThreads;
  p.tiles = ceil_div(n, p.tile);
  p.group = ssm_group(cplx != 0, vary != 0);
  p.lds = (2 * kSsmStatesMax * (cplx ? 2 : 1) + 2 * kScanWaves * p.group * (cplx ? 4 : 2)) * 4;
  p.threads = kScanThreads;
  p.grid = n == 0 ? 0 : rows;
  p.window = n < p.tile ? n : p.tile;
  return 0;
}

template <typename TI>
struct SsmIo {
  const TI* ar; const TI* ai; const TI* br; const TI* bi; const TI* cr; const TI* ci; const TI* xr; const TI* xi;
  const TI* dt; TI* yr; TI* yi;
  const float* hr; const float* hi; float* fr; float* fi; // the state planes are float32 whatever the dtype
  int64_t n, a_es, b_es, c_es, a_ns, b_ns, c_ns, h_ns, f_ns;
  int64_t s1, s2, rs[kSsmPlanes][3];                       // the rows: sizes of runs 1 and 2, the strides of every operand
  int states;
  bool rev, conj, lag, dt_out;
};

template <bool CX>
__device__ __forceinline__ void ssm_mul(float& ur, float& ui, float br, float bi, float xr, float xi) {   // u = b x
  if constexpr (CX) {
    ur = br * xr - bi * xi, ui = br * xi + bi * xr;
  } else {
    ur = br * xr;
  }
}

// One chunk of a plane into registers, as scan_load reads it (out[q]: processing step p0 + q, or the step before it
// under `shift`, zero before the row; `pad` behind the chunk's end) for an element stride of 1 or 0 only: every element
// is addressed from ONE pointer per chunk with a constant offset, so that the state loop carries no address per element.
template <typename TI>
__device__ __forceinline__ void ssm_load(const TI* p, int64_t base, int64_t es, int64_t n, bool rev, int64_t p0, int cnt,
                                         bool shift, float pad, float (&out)[kSsmL]) {
  constexpr int L = kSsmL, V = 16 / (int)sizeof(TI);
  if (es == 0) {
    const float one = cnt > 0 ? (float)ld<TI>::at(p + base) : 0.0f;
#pragma unroll
    for (int q = 0; q < L; ++q) out[q] = q < cnt ? (shift && p0 + q == 0 ? 0.0f : one) : pad;
    return;
  }
  const TI* blk = p + base + (rev ? n - p0 - L : p0);       // the chunk's L samples in memory order (read where valid only)
  float mem[L];
  if (cnt == L && ((uintptr_t)blk & 15) == 0) {
#pragma unroll
    for (int v = 0; v < L / V; ++v) {
      const uint4 w = *reinterpret_cast<const uint4*>(blk + v * V);
      TI e[V];
      __builtin_memcpy(e, &w, 16);
#pragma unroll
      for (int k = 0; k < V; ++k) mem[v * V + k] = (float)ld<TI>::at(&e[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < L; ++k) mem[k] = (rev ? k >= L - cnt : k < cnt) ? (float)ld<TI>::at(blk + k) : 0.0f;
  }
  float first = 0;
  if (shift && p0 > 0 && cnt > 0) first = (float)ld<TI>::at(rev ? blk + L : blk - 1);
#pragma unroll
  for (int q = 0; q < L; ++q) {
    const float here = rev ? mem[L - 1 - q] : mem[q];
    const float before = q == 0 ? first : (rev ? mem[L - q] : mem[q - 1]);
    out[q] = q < cnt ? (shift ? before : here) : pad;
  }
}

// one chunk of an imaginary plane: zeros for a null plane and behind the row's end, negated under `neg`
template <typename TI>
__device__ __forceinline__ void ssm_plane(const TI* p, int64_t base, int64_t es, int64_t n, bool rev, int64_t p0, int cnt,
                                          bool shift, bool neg, float (&out)[kSsmL]) {
  if (p) {
    ssm_load<TI>(p, base, es, n, rev, p0, cnt, shift, 0.0f, out);
    if (neg) {
#pragma unroll
      for (int q = 0; q < kSsmL; ++q) out[q] = -out[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < kSsmL; ++q) out[q] = 0;
  }
}

// Workgroup = row; thread c owns chunk c (L steps) of every tile of 256 L steps.  The chunk's x (times dt), dt and the
// 2 L accumulators of y stay in registers while the states go by in groups of G; the N carried states live in LDS,
// double-buffered by the tile's parity, and thread 0 moves them on.
template <typename TI, bool CX, int AM>
__global__ __launch_bounds__(kScanThreads) void ssm_chunks(SsmIo<TI> g) {
  using T = float;
  constexpr int L = kSsmL, G = ssm_group(CX, AM != kSsmConst), NC = CX ? 4 : 2, NS = CX ? 2 : 1;
  constexpr int AL = AM == kSsmConst ? 1 : L, TL = L * kScanThreads;
  __shared__ T state[2][NS][kSsmStatesMax];
  __shared__ T tot[2][kScanWaves][G][NC];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, N = g.states;
  int64_t off[kSsmPlanes];
  {
    const int64_t v = blockIdx.x, i2 = v % g.s2, w = v / g.s2, i1 = w % g.s1, i0 = w / g.s1;
#pragma unroll
    for (int k = 0; k < kSsmPlanes; ++k) off[k] = i0 * g.rs[k][0] + i1 * g.rs[k][1] + i2 * g.rs[k][2];
  }
  if (tid < N) {
    state[0][0][tid] = g.hr ? g.hr[off[kSsmH] + tid * g.h_ns] : (T)0;
    if constexpr (CX) state[0][1][tid] = g.hi ? g.hi[off[kSsmH] + tid * g.h_ns] : (T)0;
  }
  int par = 0, tp = 0;
  for (int64_t t0 = 0; t0 < g.n; t0 += TL, par ^= 1) {
    const int64_t p0 = t0 + (int64_t)tid * L, left = g.n - p0;
    const int cnt = left <= 0 ? 0 : (left > L ? L : (int)left);
    const int lo = g.lag && p0 == 0 ? 1 : 0;                // under lag nothing scales what enters the row's step 0
    T Xr[L], Xi[L], Dt[L], Ds[L], Yr[L], Yi[L];
    ssm_load<TI>(g.xr, off[kSsmX], 1, g.n, g.rev, p0, cnt, false, (T)0, Xr);
    if constexpr (CX) ssm_plane<TI>(g.xi, off[kSsmX], 1, g.n, g.rev, p0, cnt, false, false, Xi);
    if (g.dt) {
      ssm_load<TI>(g.dt, off[kSsmD], 1, g.n, g.rev, p0, cnt, false, (T)0, Dt);
      if (!g.dt_out) {
#pragma unroll
        for (int q = 0; q < L; ++q) {
          Xr[q] *= Dt[q];
          if constexpr (CX) Xi[q] *= Dt[q];
        }
      }
    }
    if constexpr (AM == kSsmDt) {                           // the dt of the coefficient: that of step p - 1 under lag, and
      if (g.lag) {                                          // zero -- a coefficient of one -- before the row and behind it
        ssm_load<TI>(g.dt, off[kSsmD], 1, g.n, g.rev, p0, cnt, true, (T)0, Ds);
      } else {
#pragma unroll
        for (int q = 0; q < L; ++q) Ds[q] = Dt[q];
      }
    }
#pragma unroll
    for (int q = 0; q < L; ++q) Yr[q] = Yi[q] = 0;
    for (int n0 = 0; n0 < N; n0 += G, tp ^= 1) {
      T Ar[G][AL], Ai[G][AL];
      ScanMap<T> m[G];
      // 1. every state of the group: its coefficients, and the chunk from zero state for its map (P, s)
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int nn = n0 + j;
        m[j] = ScanMap<T>{(T)1, (T)0, (T)0, (T)0};
        if (nn >= N) continue;
        const int64_t ao = off[kSsmA] + nn * g.a_ns, bo = off[kSsmB] + nn * g.b_ns;
        if constexpr (AM == kSsmVary) {
          ssm_load<TI>(g.ar, ao, g.a_es, g.n, g.rev, p0, cnt, g.lag, (T)1, Ar[j]);
          if constexpr (CX) ssm_plane<TI>(g.ai, ao, g.a_es, g.n, g.rev, p0, cnt, g.lag, g.conj, Ai[j]);
          if (lo && cnt > 0) Ar[j][0] = 1;                  // (the shifted imaginary chunk is zero there already)
        } else {
          const T a0r = (T)ld<TI>::at(g.ar + ao);
          T a0i = 0;
          if constexpr (CX) {
            if (g.ai) a0i = (T)ld<TI>::at(g.ai + ao);
            if (g.conj) a0i = -a0i;
          }
          if constexpr (AM == kSsmConst) {
            Ar[j][0] = a0r;
            if constexpr (CX) Ai[j][0] = a0i;
          } else {
#pragma unroll
            for (int q = 0; q < L; ++q) {
              if constexpr (CX) {
                const CF e = f_exp(Ds[q] * a0r, Ds[q] * a0i);
                Ar[j][q] = e.re, Ai[j][q] = e.im;
              } else {
                Ar[j][q] = expf(Ds[q] * a0r);
              }
            }
          }
        }
        T Br[L], Bi[L];
        ssm_load<TI>(g.br, bo, g.b_es, g.n, g.rev, p0, cnt, false, (T)0, Br);
        if constexpr (CX) ssm_plane<TI>(g.bi, bo, g.b_es, g.n, g.rev, p0, cnt, false, g.conj, Bi);
#pragma unroll
        for (int q = 0; q < L; ++q) {
          const bool on = AM != kSsmConst || (q >= lo && q < cnt);
          const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
          T ur, ui = 0;
          ssm_mul<CX>(ur, ui, Br[q], CX ? Bi[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
          scan_step<CX>(m[j].sr, m[j].si, er, ei, ur, ui);
          scan_mul<CX>(m[j].pr, m[j].pi, er, ei);
        }
      }
      // 2. the maps in order: over the lanes of the wave, then the four waves' totals through LDS -- one barrier a group
#pragma unroll
      for (int j = 0; j < G; ++j) {
#pragma unroll
        for (int by = 1; by < kWave; by <<= 1) {
          const ScanMap<T> prev = scan_shfl_up<CX>(m[j], by);
          if (lane >= by) m[j] = scan_after<CX>(m[j], prev);
        }
        if (lane == kWave - 1) {
          tot[tp][wave][j][0] = m[j].pr, tot[tp][wave][j][1] = m[j].sr;
          if constexpr (CX) tot[tp][wave][j][2] = m[j].pi, tot[tp][wave][j][3] = m[j].si;
        }
      }
      __syncthreads();
      // 3. every state of the group again, from its true entering state, into the accumulators of y
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int nn = n0 + j;
        if (nn >= N) continue;
        T kr = state[par][0][nn], ki = CX ? state[par][NS - 1][nn] : (T)0, hr = kr, hi = ki;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
          if (w == wave) hr = kr, hi = ki;
          scan_step<CX>(kr, ki, tot[tp][w][j][0], CX ? tot[tp][w][j][2] : (T)0, tot[tp][w][j][1], CX ? tot[tp][w][j][3] : (T)0);
        }
        if (tid == 0) {
          state[par ^ 1][0][nn] = kr;
          if constexpr (CX) state[par ^ 1][1][nn] = ki;
        }
        const ScanMap<T> prev = scan_shfl_up<CX>(m[j], 1);
        if (lane > 0) scan_step<CX>(hr, hi, prev.pr, prev.pi, prev.sr, prev.si);
        const int64_t bo = off[kSsmB] + nn * g.b_ns, co = off[kSsmC] + nn * g.c_ns;
        T Br[L], Bi[L], Cr[L], Ci[L];
        ssm_load<TI>(g.br, bo, g.b_es, g.n, g.rev, p0, cnt, false, (T)0, Br);
        ssm_load<TI>(g.cr, co, g.c_es, g.n, g.rev, p0, cnt, false, (T)0, Cr);
        if constexpr (CX) {
          ssm_plane<TI>(g.bi, bo, g.b_es, g.n, g.rev, p0, cnt, false, g.conj, Bi);
          ssm_plane<TI>(g.ci, co, g.c_es, g.n, g.rev, p0, cnt, false, g.conj, Ci);
        }
#pragma unroll
        for (int q = 0; q < L; ++q) {
          const bool on = AM != kSsmConst || (q >= lo && q < cnt);
          const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
          T ur, ui = 0;
          ssm_mul<CX>(ur, ui, Br[q], CX ? Bi[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
          scan_step<CX>(hr, hi, er, ei, ur, ui);
          if constexpr (CX) {
            Yr[q] += Cr[q] * hr - Ci[q] * hi;
            Yi[q] += Cr[q] * hi + Ci[q] * hr;
          } else {
            Yr[q] += Cr[q] * hr;
          }
        }
      }
    }
    if (g.dt && g.dt_out) {
#pragma unroll
      for (int q = 0; q < L; ++q) {
        Yr[q] *= Dt[q];
        if constexpr (CX) Yi[q] *= Dt[q];
      }
    }
    scan_store<TI, T, L, false>(g.yr, off[kSsmY], 1, g.n, g.rev, p0, cnt, Yr);
    if constexpr (CX) scan_store<TI, T, L, false>(g.yi, off[kSsmY], 1, g.n, g.rev, p0, cnt, Yi);
  }
  // the state after the last step: what thread 0 wrote behind the last group's barrier
  __syncthreads();
  if (g.fr && tid < N) {
    g.fr[off[kSsmF] + tid * g.f_ns] = state[par][0][tid];
    if constexpr (CX) g.fi[off[kSsmF] + tid * g.f_ns] = state[par][1][tid];
  }
}

}  // namespace sp
}  // namespace cplxamd
