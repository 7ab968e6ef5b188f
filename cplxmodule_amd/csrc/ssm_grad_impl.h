// The parameter-gradient kernel of the diagonal state-space scan: the plan, the small complex helpers and the kernel of
// ssm_grad.hip (which describes them).  The chunk loader, the maps and the chunk store are ssm_impl.h's and scan_impl.h's.
#pragma once
#include "ssm_impl.h"

namespace cplxamd {
namespace sp {

enum { kPgA = 0, kPgB, kPgC, kPgX, kPgD, kPgH, kPgG, kPgF, kPgPlanes };
enum { kPgIn = 15, kPgOut = 12 };                          // the planes of cplxamd_ssm_pgrad's `in` and `out`

// states per group (one barrier each).  Between phases 1 and 3 a state keeps its two maps and, where the coefficient
// varies along time, its chunk of A; phase 3 adds the chunk of h.  The complex instances take one state: with two the
// one-coefficient instance spills 76 bytes a lane.
constexpr int ssm_pgrad_group(bool cx, bool vary) { return cx ? 1 : (vary ? 2 : 4); }

struct SsmGradPlan {
  int64_t chunk, tile, tiles, group, lds, ws, threads, grid;
};

inline int ssm_pgrad_plan_for(int64_t n, int64_t states, int64_t rows, int dtype, int cplx, int vary, SsmGradPlan& p) {
  SsmPlan f;
  if (const int e = ssm_plan_for(n, states, rows, dtype, cplx, vary, f)) return e;
  const int64_t ns = cplx ? 2 : 1;
  p.chunk = f.chunk, p.tile = f.tile, p.tiles = f.tiles, p.threads = f.threads, p.grid = f.grid;
  p.group = ssm_pgrad_group(cplx != 0, vary != 0);
  // the carried states, the two exchanges of the maps, the exchange of the waves' sums
  p.lds = (2 * kSsmStatesMax * ns + 2 * 2 * kScanWaves * p.group * 2 * ns + 2 * kScanWaves * p.group * 3 * ns) * 4;
  p.ws = 0;
  if (p.tiles > 1 && (__builtin_mul_overflow(rows * p.tiles, states * ns * 4, &p.ws))) return CPLXAMD_ESHAPE;
  return 0;
}

template <typename TI>
struct SsmGradIo {
  const TI* ar; const TI* ai; const TI* br; const TI* bi; const TI* cr; const TI* ci; const TI* xr; const TI* xi;
  const TI* dt; const TI* gr; const TI* gi;
  const float* hr; const float* hi; const float* fr; const float* fi;   // h0 and gf: float32 whatever the dtype
  TI* dxr; TI* dxi;
  float* dar; float* dai; float* dbr; float* dbi; float* dcr; float* dci; float* ddt; float* lr; float* li; float* ws;
  int64_t n, tiles, a_ns, b_ns, c_ns, h_ns, f_ns;
  int64_t s1, s2, rs[kPgPlanes][3];
  int states, need, b_es, c_es;
  bool rev;
};

template <bool CX>
__device__ __forceinline__ void pg_mulc(float& ur, float& ui, float ar, float ai, float br, float bi) {   // u = a conj(b)
  if constexpr (CX) {
    ur = ar * br + ai * bi, ui = ai * br - ar * bi;
  } else {
    ur = ar * br;
  }
}
template <bool CX, typename T>
__device__ __forceinline__ ScanMap<T> pg_shfl_down(const ScanMap<T>& m, int by) {
  ScanMap<T> o{__shfl_down(m.pr, by, kWave), (T)0, __shfl_down(m.sr, by, kWave), (T)0};
  if constexpr (CX) o.pi = __shfl_down(m.pi, by, kWave), o.si = __shfl_down(m.si, by, kWave);
  return o;
}
// the sum over the wave, in lane 0, in a fixed order
__device__ __forceinline__ float pg_wave_sum(float v) {
#pragma unroll
  for (int by = kWave / 2; by > 0; by >>= 1) v += __shfl_down(v, by, kWave);
  return v;
}

// The coefficient chunk of state `ao` (ssm_chunks' phase 1 without `conj` and `lag`) and the pole itself.
template <typename TI, bool CX, int AM, int AL>
__device__ __forceinline__ void pg_coef(const SsmGradIo<TI>& g, int64_t ao, int64_t p0, int cnt, const float (&Dt)[kSsmL],
                                        float (&Ar)[AL], float (&Ai)[AL], float& a0r, float& a0i) {
  a0r = a0i = 0;
  if constexpr (AM == kSsmVary) {
    ssm_load<TI>(g.ar, ao, 1, g.n, g.rev, p0, cnt, false, 1.0f, Ar);
    if constexpr (CX) ssm_plane<TI>(g.ai, ao, 1, g.n, g.rev, p0, cnt, false, false, Ai);
  } else {
    a0r = (float)ld<TI>::at(g.ar + ao);
    if constexpr (CX) {
      if (g.ai) a0i = (float)ld<TI>::at(g.ai + ao);
    }
    if constexpr (AM == kSsmConst) {
      Ar[0] = a0r;
      if constexpr (CX) Ai[0] = a0i;
    } else {
#pragma unroll
      for (int q = 0; q < kSsmL; ++q) {
        if constexpr (CX) {
          const CF e = f_exp(Dt[q] * a0r, Dt[q] * a0i);
          Ar[q] = e.re, Ai[q] = e.im;
        } else {
          Ar[q] = expf(Dt[q] * a0r);
        }
      }
    }
  }
}

// Workgroup = row; thread c owns chunk c (L steps) of every tile of 256 L steps.  Per tile the chunks of X (= dt x), g
// and dt and the accumulators of dX and ddt stay in registers while the states go by in groups of G.  The tiles are
// walked last to first (lambda's order: its carried states live in LDS); the states of h that enter the tiles come from
// the prologue's workspace.
template <typename TI, bool CX, int AM>
__global__ __launch_bounds__(kScanThreads) void ssm_pgrad(SsmGradIo<TI> g) {
  using T = float;
  constexpr int L = kSsmL, G = ssm_pgrad_group(CX, AM != kSsmConst), NC = CX ? 4 : 2, NS = CX ? 2 : 1;
  constexpr int AL = AM == kSsmConst ? 1 : L, TL = L * kScanThreads;
  constexpr bool HG = !(CX && AM == kSsmDt);               // g's chunk is held for the tile, or read again per state
  __shared__ T state[2][NS][kSsmStatesMax];
  __shared__ T tot[2][2][kScanWaves][G][NC];               // [parity][h, lambda]
  __shared__ T red[2][kScanWaves][G][3][NS];               // [parity][wave][state of the group][a, b, c]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, N = g.states;
  const int64_t row = blockIdx.x;
  int64_t off[kPgPlanes];
  {
    const int64_t i2 = row % g.s2, w = row / g.s2, i1 = w % g.s1, i0 = w / g.s1;
#pragma unroll
    for (int k = 0; k < kPgPlanes; ++k) off[k] = i0 * g.rs[k][0] + i1 * g.rs[k][1] + i2 * g.rs[k][2];
  }
  // `need` switches the stores and the reductions.  The products themselves are formed for every gradient: a branch
  // per gradient inside the chunk loops cost the complex instances up to 190 registers and their zero scratch.
  const bool wa = (g.need & CPLXAMD_SSM_NEED_A) != 0, wb = (g.need & CPLXAMD_SSM_NEED_B) != 0;
  const bool wc = (g.need & CPLXAMD_SSM_NEED_C) != 0, wx = (g.need & CPLXAMD_SSM_NEED_X) != 0;
  const bool wd = AM == kSsmDt && (g.need & CPLXAMD_SSM_NEED_DT) != 0;
  // what is summed over time: the gradient of an operand with one value per state
  const bool sum_a = wa && AM != kSsmVary, sum_b = wb && g.b_es == 0, sum_c = wc && g.c_es == 0;
  const bool sums = sum_a || sum_b || sum_c;
  T* ws = g.ws + row * g.tiles * N * NS;                    // [tiles][NS][N]: the state of h that enters each tile
  int tp = 0;

  // ---- the prologue: phases 1 and 2 for h alone, first tile to last but one, for the states that enter the tiles
  if (g.tiles > 1) {
    if (tid < N) {
      const T h0r = g.hr ? g.hr[off[kPgH] + tid * g.h_ns] : (T)0;
      state[0][0][tid] = ws[tid] = h0r;
      if constexpr (CX) state[0][1][tid] = ws[N + tid] = g.hi ? g.hi[off[kPgH] + tid * g.h_ns] : (T)0;
    }
    int par = 0;
    for (int64_t tile = 0; tile + 1 < g.tiles; ++tile, par ^= 1) {
      const int64_t p0 = tile * TL + (int64_t)tid * L;      // (every tile but the last is full)
      T Xr[L], Xi[L], Dt[L];
      ssm_load<TI>(g.xr, off[kPgX], 1, g.n, g.rev, p0, L, false, (T)0, Xr);
      if constexpr (CX) ssm_plane<TI>(g.xi, off[kPgX], 1, g.n, g.rev, p0, L, false, false, Xi);
      if constexpr (AM == kSsmDt) {
        ssm_load<TI>(g.dt, off[kPgD], 1, g.n, g.rev, p0, L, false, (T)0, Dt);
#pragma unroll
        for (int q = 0; q < L; ++q) {
          Xr[q] *= Dt[q];
          if constexpr (CX) Xi[q] *= Dt[q];
        }
      }
      T* next = ws + (tile + 1) * N * NS;
      for (int n0 = 0; n0 < N; n0 += G, tp ^= 1) {
        ScanMap<T> m[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const int nn = n0 + j;
          m[j] = ScanMap<T>{(T)1, (T)0, (T)0, (T)0};
          if (nn >= N) continue;
          T Ar[AL], Ai[AL], a0r, a0i, Br[L], Bi[L];
          pg_coef<TI, CX, AM, AL>(g, off[kPgA] + nn * g.a_ns, p0, L, Dt, Ar, Ai, a0r, a0i);
          const int64_t bo = off[kPgB] + nn * g.b_ns;
          ssm_load<TI>(g.br, bo, g.b_es, g.n, g.rev, p0, L, false, (T)0, Br);
          if constexpr (CX) ssm_plane<TI>(g.bi, bo, g.b_es, g.n, g.rev, p0, L, false, false, Bi);
#pragma unroll
          for (int q = 0; q < L; ++q) {
            const T er = Ar[q % AL], ei = CX ? Ai[q % AL] : (T)0;
            T ur, ui = 0;
            ssm_mul<CX>(ur, ui, Br[q], CX ? Bi[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
            scan_step<CX>(m[j].sr, m[j].si, er, ei, ur, ui);
            scan_mul<CX>(m[j].pr, m[j].pi, er, ei);
          }
#pragma unroll
          for (int by = 1; by < kWave; by <<= 1) {
            const ScanMap<T> prev = scan_shfl_up<CX>(m[j], by);
            if (lane >= by) m[j] = scan_after<CX>(m[j], prev);
          }
          if (lane == kWave - 1) {
            tot[tp][0][wave][j][0] = m[j].pr, tot[tp][0][wave][j][1] = m[j].sr;
            if constexpr (CX) tot[tp][0][wave][j][2] = m[j].pi, tot[tp][0][wave][j][3] = m[j].si;
          }
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
          for (int j = 0; j < G; ++j) {
            const int nn = n0 + j;
            if (nn >= N) continue;
            T kr = state[par][0][nn], ki = CX ? state[par][NS - 1][nn] : (T)0;
#pragma unroll
            for (int w = 0; w < kScanWaves; ++w)
              scan_step<CX>(kr, ki, tot[tp][0][w][j][0], CX ? tot[tp][0][w][j][2] : (T)0, tot[tp][0][w][j][1],
                            CX ? tot[tp][0][w][j][3] : (T)0);
            state[par ^ 1][0][nn] = next[nn] = kr;
            if constexpr (CX) state[par ^ 1][1][nn] = next[N + nn] = ki;
          }
        }
      }
    }
    __syncthreads();                                        // the workspace is this workgroup's own: visible behind the barrier
  }

  // ---- lambda's carried states: gf enters the last step unscaled
  if (tid < N) {
    state[0][0][tid] = g.fr ? g.fr[off[kPgF] + tid * g.f_ns] : (T)0;
    if constexpr (CX) state[0][1][tid] = g.fi ? g.fi[off[kPgF] + tid * g.f_ns] : (T)0;
  }
  T acc[3][NS];                                             // thread n: the sums over time of state n (a, b, c)
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[k][s] = 0;
  int par = 0, pend = -1;                                   // pend: the group whose waves' sums wait in red[tp ^ 1]
  const auto fold = [&](int buf) {
    if (sums && pend >= 0 && tid >= pend && tid < pend + G) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          T v = red[buf][0][tid - pend][k][s];
#pragma unroll
          for (int w = 1; w < kScanWaves; ++w) v += red[buf][w][tid - pend][k][s];
          acc[k][s] += v;
        }
    }
  };

  for (int64_t tile = g.tiles - 1; tile >= 0; --tile, par ^= 1) {
    const int64_t p0 = tile * TL + (int64_t)tid * L, left = g.n - p0;
    const int cnt = left <= 0 ? 0 : (left > L ? L : (int)left);
    const T* hin = ws + tile * N * NS;
    T Xr[L], Xi[L], Gr[L], Gi[L], Dt[L], DXr[L], DXi[L], DD[L];
    ssm_load<TI>(g.xr, off[kPgX], 1, g.n, g.rev, p0, cnt, false, (T)0, Xr);
    if constexpr (CX) ssm_plane<TI>(g.xi, off[kPgX], 1, g.n, g.rev, p0, cnt, false, false, Xi);
    const auto load_g = [&]() {
      ssm_load<TI>(g.gr, off[kPgG], 1, g.n, g.rev, p0, cnt, false, (T)0, Gr);
      if constexpr (CX) ssm_plane<TI>(g.gi, off[kPgG], 1, g.n, g.rev, p0, cnt, false, false, Gi);
    };
    if constexpr (HG) load_g();
    if constexpr (AM == kSsmDt) {                           // (zero behind the row's end: a coefficient of one)
      ssm_load<TI>(g.dt, off[kPgD], 1, g.n, g.rev, p0, cnt, false, (T)0, Dt);
#pragma unroll
      for (int q = 0; q < L; ++q) {
        Xr[q] *= Dt[q];
        if constexpr (CX) Xi[q] *= Dt[q];
      }
    }
#pragma unroll
    for (int q = 0; q < L; ++q) DXr[q] = DXi[q] = DD[q] = 0;

    for (int n0 = 0; n0 < N; n0 += G, tp ^= 1) {
      T Ar[G][AL], Ai[G][AL], a0r[G], a0i[G];
      ScanMap<T> mh[G], ml[G];
      // 1. every state of the group: its coefficients, and the chunk from zero state for both maps -- h's ascending,
      //    lambda's (mu[p] = conj(A[p]) lambda[p], what enters step p - 1) descending; their products are conjugates
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int nn = n0 + j;
        mh[j] = ml[j] = ScanMap<T>{(T)1, (T)0, (T)0, (T)0};
        if (nn >= N) continue;
        pg_coef<TI, CX, AM, AL>(g, off[kPgA] + nn * g.a_ns, p0, cnt, Dt, Ar[j], Ai[j], a0r[j], a0i[j]);
        const int64_t bo = off[kPgB] + nn * g.b_ns, co = off[kPgC] + nn * g.c_ns;
        T Pr[L], Pi[L];
        ssm_load<TI>(g.br, bo, g.b_es, g.n, g.rev, p0, cnt, false, (T)0, Pr);
        if constexpr (CX) ssm_plane<TI>(g.bi, bo, g.b_es, g.n, g.rev, p0, cnt, false, false, Pi);
#pragma unroll
        for (int q = 0; q < L; ++q) {
          const bool on = AM != kSsmConst || q < cnt;
          const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
          T ur, ui = 0;
          ssm_mul<CX>(ur, ui, Pr[q], CX ? Pi[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
          scan_step<CX>(mh[j].sr, mh[j].si, er, ei, ur, ui);
          scan_mul<CX>(mh[j].pr, mh[j].pi, er, ei);
        }
        ml[j].pr = mh[j].pr, ml[j].pi = -mh[j].pi;
        __builtin_amdgcn_sched_barrier(0);                  // (b's chunk is dead before c's is fetched)
        if constexpr (!HG) load_g();
        ssm_load<TI>(g.cr, co, g.c_es, g.n, g.rev, p0, cnt, false, (T)0, Pr);
        if constexpr (CX) ssm_plane<TI>(g.ci, co, g.c_es, g.n, g.rev, p0, cnt, false, false, Pi);
#pragma unroll
        for (int q = L - 1; q >= 0; --q) {
          const bool on = AM != kSsmConst || q < cnt;
          const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
          T vr, vi = 0;
          pg_mulc<CX>(vr, vi, Gr[q], CX ? Gi[q] : (T)0, Pr[q], CX ? Pi[q] : (T)0);
          vr += ml[j].sr, vi += ml[j].si;
          pg_mulc<CX>(ml[j].sr, ml[j].si, vr, vi, er, ei);
        }
      }
      // 2. the maps in order over the lanes, h's upwards and lambda's downwards, then the waves' totals through LDS: one
      //    barrier for both, and for the sums that the group before left in `red`
#pragma unroll
      for (int j = 0; j < G; ++j) {
#pragma unroll
        for (int by = 1; by < kWave; by <<= 1) {
          const ScanMap<T> prev = scan_shfl_up<CX>(mh[j], by), nxt = pg_shfl_down<CX>(ml[j], by);
          if (lane >= by) mh[j] = scan_after<CX>(mh[j], prev);
          if (lane + by < kWave) ml[j] = scan_after<CX>(ml[j], nxt);
        }
        if (lane == kWave - 1) {
          tot[tp][0][wave][j][0] = mh[j].pr, tot[tp][0][wave][j][1] = mh[j].sr;
          if constexpr (CX) tot[tp][0][wave][j][2] = mh[j].pi, tot[tp][0][wave][j][3] = mh[j].si;
        }
        if (lane == 0) {
          tot[tp][1][wave][j][0] = ml[j].pr, tot[tp][1][wave][j][1] = ml[j].sr;
          if constexpr (CX) tot[tp][1][wave][j][2] = ml[j].pi, tot[tp][1][wave][j][3] = ml[j].si;
        }
      }
      __syncthreads();
      fold(tp ^ 1);
      // 3. every state of the group again from its true entering states: h ascending and kept, then lambda descending,
      //    forming the gradients as it goes
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int nn = n0 + j;
        if (nn >= N) continue;
        T kr, ki = 0, h0r, h0i = 0;
        if (g.tiles > 1) {
          kr = hin[nn];
          if constexpr (CX) ki = hin[N + nn];
        } else {
          kr = g.hr ? g.hr[off[kPgH] + nn * g.h_ns] : (T)0;
          if constexpr (CX) ki = g.hi ? g.hi[off[kPgH] + nn * g.h_ns] : (T)0;
        }
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
          if (w == wave) h0r = kr, h0i = ki;
          scan_step<CX>(kr, ki, tot[tp][0][w][j][0], CX ? tot[tp][0][w][j][2] : (T)0, tot[tp][0][w][j][1],
                        CX ? tot[tp][0][w][j][3] : (T)0);
        }
        T mr, mi = 0;
        kr = state[par][0][nn], ki = CX ? state[par][NS - 1][nn] : (T)0;
#pragma unroll
        for (int w = kScanWaves - 1; w >= 0; --w) {
          if (w == wave) mr = kr, mi = ki;
          scan_step<CX>(kr, ki, tot[tp][1][w][j][0], CX ? tot[tp][1][w][j][2] : (T)0, tot[tp][1][w][j][1],
                        CX ? tot[tp][1][w][j][3] : (T)0);
        }
        if (tid == 0) {
          state[par ^ 1][0][nn] = kr;
          if constexpr (CX) state[par ^ 1][1][nn] = ki;
        }
        {
          const ScanMap<T> prev = scan_shfl_up<CX>(mh[j], 1), nxt = pg_shfl_down<CX>(ml[j], 1);
          if (lane > 0) scan_step<CX>(h0r, h0i, prev.pr, prev.pi, prev.sr, prev.si);
          if (lane < kWave - 1) scan_step<CX>(mr, mi, nxt.pr, nxt.pi, nxt.sr, nxt.si);
        }
        const int64_t bo = off[kPgB] + nn * g.b_ns, co = off[kPgC] + nn * g.c_ns;
        const int64_t wide = (row * N + nn) * g.n;           // this state's chunk row of a [rows, N, T] result
        T sa[NS], sb[NS], sc[NS], Hr[L], Hi[L], Pr[L], Pi[L];
#pragma unroll
        for (int s = 0; s < NS; ++s) sa[s] = sb[s] = sc[s] = 0;
        ssm_load<TI>(g.br, bo, g.b_es, g.n, g.rev, p0, cnt, false, (T)0, Pr);
        if constexpr (CX) ssm_plane<TI>(g.bi, bo, g.b_es, g.n, g.rev, p0, cnt, false, false, Pi);
        {
          T hr = h0r, hi = h0i;
#pragma unroll
          for (int q = 0; q < L; ++q) {
            const bool on = AM != kSsmConst || q < cnt;
            const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
            T ur, ui = 0;
            ssm_mul<CX>(ur, ui, Pr[q], CX ? Pi[q] : (T)0, Xr[q], CX ? Xi[q] : (T)0);
            scan_step<CX>(hr, hi, er, ei, ur, ui);
            Hr[q] = hr;
            if constexpr (CX) Hi[q] = hi;
          }
        }
        if constexpr (!HG) load_g();
        {                                                   // dc = g conj(h): zero behind the row's end, where g is
          T Er[L], Ei[L];
#pragma unroll
          for (int q = 0; q < L; ++q) {
            Ei[q] = 0;
            pg_mulc<CX>(Er[q], Ei[q], Gr[q], CX ? Gi[q] : (T)0, Hr[q], CX ? Hi[q] : (T)0);
            sc[0] += Er[q];
            if constexpr (CX) sc[1] += Ei[q];
          }
          if (wc && !sum_c) {
            scan_store<float, T, L, false>(g.dcr, wide, 1, g.n, g.rev, p0, cnt, Er);
            if constexpr (CX) scan_store<float, T, L, false>(g.dci, wide, 1, g.n, g.rev, p0, cnt, Ei);
          }
        }
        __builtin_amdgcn_sched_barrier(0);                  // (dc's chunk is stored before c's is fetched)
        T Cr[L], Ci[L];
        ssm_load<TI>(g.cr, co, g.c_es, g.n, g.rev, p0, cnt, false, (T)0, Cr);
        if constexpr (CX) ssm_plane<TI>(g.ci, co, g.c_es, g.n, g.rev, p0, cnt, false, false, Ci);
        T lr = 0, li = 0;
#pragma unroll
        for (int q = L - 1; q >= 0; --q) {
          const bool on = AM != kSsmConst || q < cnt;
          const T er = on ? Ar[j][q % AL] : (T)1, ei = CX && on ? Ai[j][q % AL] : (T)0;
          li = 0;
          pg_mulc<CX>(lr, li, Gr[q], CX ? Gi[q] : (T)0, Cr[q], CX ? Ci[q] : (T)0);
          lr += mr, li += mi;                               // lambda[p] = conj(c) g + mu[p + 1]
          {                                                 // dX += conj(b) lambda
            T ur, ui = 0;
            pg_mulc<CX>(ur, ui, lr, li, Pr[q], CX ? Pi[q] : (T)0);
            DXr[q] += ur;
            if constexpr (CX) DXi[q] += ui;
          }
          {                                                 // db = lambda conj(X): zero behind the row's end, where X is
            T ur, ui = 0;
            pg_mulc<CX>(ur, ui, lr, li, Xr[q], CX ? Xi[q] : (T)0);
            Pr[q] = ur, sb[0] += ur;
            if constexpr (CX) Pi[q] = ui, sb[1] += ui;
          }
          {                                                 // dA = lambda conj(h[p - 1]), nothing behind the row's end
            T ur, ui = 0;
            pg_mulc<CX>(ur, ui, lr, li, q == 0 ? h0r : Hr[q ? q - 1 : 0], CX ? (q == 0 ? h0i : Hi[q ? q - 1 : 0]) : (T)0);
            if (q >= cnt) ur = ui = 0;
            if constexpr (AM == kSsmDt) {                   // da += dA conj(dt A), ddt += Re(dA conj(a A))
              T tr, ti = 0;
              pg_mulc<CX>(tr, ti, ur, ui, er, ei);
              sa[0] += Dt[q] * tr;
              if constexpr (CX) sa[1] += Dt[q] * ti;
              DD[q] += tr * a0r[j] + (CX ? ti * a0i[j] : (T)0);
            } else {
              Hr[q] = ur, sa[0] += ur;
              if constexpr (CX) Hi[q] = ui, sa[1] += ui;
            }
          }
          pg_mulc<CX>(mr, mi, lr, li, er, ei);              // mu[p] = conj(A[p]) lambda[p]
        }
        if (tile == 0 && tid == 0 && g.lr) {                // lambda[n, 0]
          g.lr[row * N + nn] = lr;
          if constexpr (CX) g.li[row * N + nn] = li;
        }
        if (wb && !sum_b) {
          scan_store<float, T, L, false>(g.dbr, wide, 1, g.n, g.rev, p0, cnt, Pr);
          if constexpr (CX) scan_store<float, T, L, false>(g.dbi, wide, 1, g.n, g.rev, p0, cnt, Pi);
        }
        if constexpr (AM == kSsmVary) {
          if (wa) {
            scan_store<float, T, L, false>(g.dar, wide, 1, g.n, g.rev, p0, cnt, Hr);
            if constexpr (CX) scan_store<float, T, L, false>(g.dai, wide, 1, g.n, g.rev, p0, cnt, Hi);
          }
        }
        if (sums) {                                         // the chunk's sums over the wave, lane 0's into `red`
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const T va = sum_a ? pg_wave_sum(sa[s]) : (T)0, vb = sum_b ? pg_wave_sum(sb[s]) : (T)0;
            const T vc = sum_c ? pg_wave_sum(sc[s]) : (T)0;
            if (lane == 0) red[tp][wave][j][0][s] = va, red[tp][wave][j][1][s] = vb, red[tp][wave][j][2][s] = vc;
          }
        }
      }
      pend = n0;
    }
    // dX is complete: ddt takes Re(conj(x) dX), dx is dX (dt dX in the dt form), rounded once
    if constexpr (AM == kSsmDt) {
      if (wd) {
        T xr[L], xi[L];
        ssm_load<TI>(g.xr, off[kPgX], 1, g.n, g.rev, p0, cnt, false, (T)0, xr);
        if constexpr (CX) ssm_plane<TI>(g.xi, off[kPgX], 1, g.n, g.rev, p0, cnt, false, false, xi);
#pragma unroll
        for (int q = 0; q < L; ++q) DD[q] += xr[q] * DXr[q] + (CX ? xi[q] * DXi[q] : (T)0);
        scan_store<float, T, L, false>(g.ddt, row * g.n, 1, g.n, g.rev, p0, cnt, DD);
      }
#pragma unroll
      for (int q = 0; q < L; ++q) {
        DXr[q] *= Dt[q];
        if constexpr (CX) DXi[q] *= Dt[q];
      }
    }
    if (wx) {
      scan_store<TI, T, L, false>(g.dxr, row * g.n, 1, g.n, g.rev, p0, cnt, DXr);
      if constexpr (CX) scan_store<TI, T, L, false>(g.dxi, row * g.n, 1, g.n, g.rev, p0, cnt, DXi);
    }
  }
  // ---- the sums over time, once per row
  if (sums) {
    __syncthreads();
    fold(tp ^ 1);
    if (tid < N) {
      float* const out[3][2] = {{g.dar, g.dai}, {g.dbr, g.dbi}, {g.dcr, g.dci}};
      const bool on[3] = {sum_a, sum_b, sum_c};
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (on[k]) out[k][s][row * N + tid] = acc[k][s];
    }
  }
}

}  // namespace sp
}  // namespace cplxamd
