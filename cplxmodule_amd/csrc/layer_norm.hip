// Complex layer normalisation of planar tensors (cplx.layer_norm, nn.CplxLayerNorm): statistics per ROW of N complex
// features, taken while the row sits in registers.  DESIGN 26.
//
//   m = mean x,  c = x - m
//   whiten:   a = mean c_r^2 + eps, d = mean c_i^2 + eps, b = mean c_r c_i,  s = sqrt(a d - b^2),  t = s sqrt(a + d + 2 s)
//             p = (d + s) / t, q = -b / t, r = (a + s) / t;   y_r = p c_r + q c_i,  y_i = q c_r + r c_i
//   modulus:  v = mean |c|^2 + eps;   y = c / sqrt(v)      (p = r = rstd, q = 0)
//   out = W y + B per feature (W [2][2][N], B [2][N], float32), or y without them.
//
// One template serves three plans (cplxamd_ln_plan).  A GROUP of G threads owns a row and holds a TILE of G * C * V
// columns in registers (V = 16 bytes of the plane dtype; thread t of the group owns the V columns at (c G + t) V of every
// chunk c < C, so that a chunk is one 16-byte access per lane and consecutive lanes are consecutive in memory):
//   wave    N <= 512         G = 64: one wave per row, four rows per 256-thread workgroup, reductions by __shfl_xor only
//                            (no LDS, no barrier); the affine parameters of the lane's 8 columns live in registers and the
//                            waves walk rows (a persistent grid), so W and B are read once per wave, not once per row
//   block   N <= 8192        G = the workgroup (256 threads x 32 columns forward; backward 512 x 8, N <= 4096); a round is
//                            a wave reduction and ONE exchange through LDS (two alternating buffers: one barrier a round)
//   stream  above            the block template over tiles of 8192 (4096) columns: the statistics of a tile are taken from its
//                            registers (mean first, then centred moments) and merged into the row's by Chan's update --
//                            never E[x^2] - m^2 -- and the row is read a second time (from L2) to be normalised
// Forward: mean first, then the centred second moments of the registers, reduced together; (m_r, m_i, p, q, r) or
// (m_r, m_i, rstd) per row are saved.  Backward: with g^ = W^T g, six row sums (three for modulus) give
//   dx = P (g^ - mean g^ - Z y),   Z = sym(G) + (G01 - G10) / (2 (p + r)) [[-2q, p - r], [p - r, 2q]],   G = mean g^ y^T
// (modulus: Z = (G00 + G11) I); y is recomputed from x and the saved statistics.  Workgroups are persistent over rows and a
// thread owns fixed columns, so sum g y^T (4) and sum g (2) of its columns stay in registers while the workgroup walks
// rows; the waves of a wave-plan workgroup combine them once through LDS, per-workgroup partials go to the workspace and
// ln_finish_kernel sums them in workgroup order.  No atomics anywhere: the same input gives the same bits.
#include <cmath>

#include "common.h"
#include "prims.h"
#include "runs.h"

namespace cplxamd {
namespace ln {

constexpr int kWaveCols = 8;                     // columns a lane of the wave plan owns
constexpr int kWaveMax = 64 * kWaveCols;         // seam wave | block
constexpr int kTile = 8192;                      // forward: seam block | stream, and the stream plan's tile
constexpr int kBwdTile = 4096;                   // backward: the same (a thread also holds 6 partial sums per column)
constexpr int kFwdThreads = 256, kBwdThreads = 512;
constexpr int64_t kWsCap = 32ll << 20;           // bytes of parameter-gradient partials at most
constexpr int kFwdGridWave = 2048, kFwdGridBlock = 1 << 20, kBwdGridWave = 1024, kBwdGridBlock = 256;

struct Args {
  const void *x_r, *x_i, *g_r, *g_i;
  void *o_r, *o_i;        // forward: the result; backward: dx (both NULL: not wanted)
  float* stats;           // [rows][5 or 3]: written by the forward, read by the backward
  const float *w, *b;     // NULL: no affine step
  float* part;            // backward: [grid][6][N] partial parameter gradients (NULL: not wanted)
  int64_t rows, size1, size2;
  int64_t xs[3], os[3], gs[3];
  int N, vec, one_run;
  float eps;
};

__device__ __forceinline__ void row_offsets(const Args& a, int64_t row, int64_t& xo, int64_t& oo, int64_t& go) {
  if (a.one_run) {
    xo = row * a.xs[2]; oo = row * a.os[2]; go = row * a.gs[2];
    return;
  }
  const int64_t i2 = row % a.size2, w = row / a.size2, i1 = w % a.size1, i0 = w / a.size1;
  xo = i0 * a.xs[0] + i1 * a.xs[1] + i2 * a.xs[2];
  oo = i0 * a.os[0] + i1 * a.os[1] + i2 * a.os[2];
  go = i0 * a.gs[0] + i1 * a.gs[1] + i2 * a.gs[2];
}

// ---- 16 bytes of a plane <-> V floats -----------------------------------------------------------------------------------
__device__ __forceinline__ void ldv(const float* p, float (&v)[4]) {
  const f4 t = ld4(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = t.v[e];
}
__device__ __forceinline__ void ldv(const bf16_t* p, float (&v)[8]) {
  const f8 t = ld8(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = t.h[e >> 2].v[e & 3];
}
__device__ __forceinline__ void stv(float* p, const float (&v)[4]) { st4(p, f4{{v[0], v[1], v[2], v[3]}}); }
__device__ __forceinline__ void stv(bf16_t* p, const float (&v)[8]) {
  st8(p, f8{{f4{{v[0], v[1], v[2], v[3]}}, f4{{v[4], v[5], v[6], v[7]}}}});
}
// V float32 parameters (two accesses where V = 8)
template <int V>
__device__ __forceinline__ void ldw(const float* p, float (&v)[V]) {
#pragma unroll
  for (int h = 0; h < V / 4; ++h) {
    const f4 t = ld4(p + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * h + e] = t.v[e];
  }
}

// the V columns from `col` of one plane row: a 16-byte access, or predicated scalars; zeros past N
template <typename T, int V>
__device__ __forceinline__ void load_chunk(const T* p, int col, int N, int vec, float (&v)[V]) {
  if (vec) {
    if (col < N) {
      ldv(p + col, v);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = col + e < N ? io<T>::ld(p + col + e) : 0.f;
  }
}
template <typename T, int V>
__device__ __forceinline__ void store_chunk(T* p, int col, int N, int vec, const float (&v)[V]) {
  if (vec) {
    if (col < N) stv(p + col, v);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (col + e < N) io<T>::st(p + col + e, v[e]);
  }
}

// the affine parameters of V columns: W00, W01, W10, W11, B0, B1 (identity and zero without them)
template <int V>
struct Affine {
  float w[4][V], b[2][V];
};
template <int V>
__device__ __forceinline__ void load_affine(const float* w, const float* b, int col, int N, int vec, Affine<V>& o) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < V; ++e) o.w[j][e] = (j == 0 || j == 3) ? 1.f : 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < V; ++e) o.b[j][e] = 0.f;
  if (!w) return;
  if (vec) {
    if (col < N) {
#pragma unroll
      for (int j = 0; j < 4; ++j) ldw<V>(w + (int64_t)j * N + col, o.w[j]);
      if (b) {
#pragma unroll
        for (int j = 0; j < 2; ++j) ldw<V>(b + (int64_t)j * N + col, o.b[j]);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (col + e < N) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o.w[j][e] = w[(int64_t)j * N + col + e];
        if (b) {
#pragma unroll
          for (int j = 0; j < 2; ++j) o.b[j][e] = b[(int64_t)j * N + col + e];
        }
      }
  }
}

// ---- the sum of K values over a group: a wave (shuffles only), or the workgroup (plus one exchange through LDS) -------
// lds holds 2 x 6 x (G / 64) floats; rounds alternate between its halves, so one barrier a round is enough: a wave can
// write the half of round k + 2 only behind the barrier of round k + 1, which every wave passes after it has read round k.
template <int G, int K>
__device__ __forceinline__ void group_sum(float (&v)[K], float* lds, int& round) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (G > 64) {
    constexpr int NW = G / 64;
    float* buf = lds + (round & 1) * 6 * NW;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) buf[k * NW + wid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += buf[k * NW + w];
      v[k] = s;
    }
    ++round;
  }
}

// p, q, r from the centred sums M = (sum c_r^2, sum c_i^2, sum c_r c_i)  (modulus: M[0] = sum |c|^2).  a d - b^2 is
// (a0 d0 - b^2) + eps (a0 + d0 + eps) with the first term clamped at 0: rounding cannot push the determinant below zero.
template <int KIND>
__device__ __forceinline__ void whitening(const float (&M)[3], float invN, float eps, float& p, float& q, float& r) {
  if (KIND == CPLXAMD_LN_MODULUS) {
    p = r = 1.f / sqrtf(fmaf(M[0], invN, eps));
    q = 0.f;
  } else {
    const float a0 = M[0] * invN, d0 = M[1] * invN, b = M[2] * invN;
    const float a = a0 + eps, d = d0 + eps;
    const float s = sqrtf(fmaxf(fmaf(a0, d0, -b * b), 0.f) + eps * (a0 + d0 + eps));
    const float it = 1.f / (s * sqrtf(a + d + 2.f * s));
    p = (d + s) * it;
    q = -b * it;
    r = (a + s) * it;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int KIND, int G, int C, bool STREAM>
__global__ __launch_bounds__(G > kFwdThreads ? G : kFwdThreads) void ln_fwd_kernel(Args a) {
  constexpr int V = 16 / sizeof(T), NT = G > kFwdThreads ? G : kFwdThreads, RPW = NT / G, TILE = G * C * V;
  constexpr int NS = KIND == CPLXAMD_LN_MODULUS ? 3 : 5, NM = KIND == CPLXAMD_LN_MODULUS ? 1 : 3;
  constexpr bool PREG = G == 64;                 // the affine parameters of the thread's columns stay in registers
  __shared__ float lds[G > 64 ? 2 * 6 * (G / 64) : 1];
  int round = 0;
  const int gt = threadIdx.x % G, sub = threadIdx.x / G;
  const int N = a.N, vec = a.vec;
  const float invN = 1.f / (float)N;
  const int tiles = STREAM ? (N + TILE - 1) / TILE : 1;
  Affine<V> areg[PREG ? C : 1];
  if (PREG) {
#pragma unroll
    for (int c = 0; c < C; ++c) load_affine<V>(a.w, a.b, (c * G + gt) * V, N, vec, areg[c]);
  }
  for (int64_t row = (int64_t)blockIdx.x * RPW + sub; row < a.rows; row += (int64_t)gridDim.x * RPW) {
    int64_t xo, oo, go;
    row_offsets(a, row, xo, oo, go);
    const T *xr = reinterpret_cast<const T*>(a.x_r) + xo, *xi = reinterpret_cast<const T*>(a.x_i) + xo;
    T *yr = reinterpret_cast<T*>(a.o_r) + oo, *yi = reinterpret_cast<T*>(a.o_i) + oo;
    float cr[C][V], ci[C][V];
    float mr = 0.f, mi = 0.f, M[3] = {0.f, 0.f, 0.f}, seen = 0.f;
    for (int t = 0; t < tiles; ++t) {
      const int col0 = t * TILE;
      const float cnt = (float)(N - col0 < TILE ? N - col0 : TILE);
      float s[2] = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = col0 + (c * G + gt) * V;
        load_chunk<T, V>(xr, col, N, vec, cr[c]);
        load_chunk<T, V>(xi, col, N, vec, ci[c]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          s[0] += cr[c][e];
          s[1] += ci[c][e];
        }
      }
      group_sum<G, 2>(s, lds, round);
      const float tr = s[0] / cnt, ti = s[1] / cnt;          // the tile's mean
      float m[NM];
#pragma unroll
      for (int k = 0; k < NM; ++k) m[k] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = col0 + (c * G + gt) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const bool in = col + e < N;
          const float u = in ? cr[c][e] - tr : 0.f, v = in ? ci[c][e] - ti : 0.f;
          cr[c][e] = u;
          ci[c][e] = v;
          if constexpr (KIND == CPLXAMD_LN_MODULUS) {
            m[0] = fmaf(u, u, fmaf(v, v, m[0]));
          } else {
            m[0] = fmaf(u, u, m[0]);
            m[1] = fmaf(v, v, m[1]);
            m[2] = fmaf(u, v, m[2]);
          }
        }
      }
      group_sum<G, NM>(m, lds, round);
      if (!STREAM) {
        mr = tr;
        mi = ti;
#pragma unroll
        for (int k = 0; k < NM; ++k) M[k] = m[k];
      } else {                                                // Chan's update of (count, mean, centred sums)
        const float dr = tr - mr, di = ti - mi, tot = seen + cnt, f = cnt / tot, h = seen * f;
        mr = fmaf(dr, f, mr);
        mi = fmaf(di, f, mi);
        if constexpr (KIND == CPLXAMD_LN_MODULUS) {
          M[0] += m[0] + (dr * dr + di * di) * h;
        } else {
          M[0] += m[0] + dr * dr * h;
          M[1] += m[1] + di * di * h;
          M[2] += m[2] + dr * di * h;
        }
        seen = tot;
      }
    }
    float p, q, r;
    whitening<KIND>(M, invN, a.eps, p, q, r);
    if (gt == 0) {
      float* st = a.stats + row * NS;
      st[0] = mr;
      st[1] = mi;
      st[2] = p;
      if (NS == 5) {
        st[3] = q;
        st[4] = r;
      }
    }
    for (int t = 0; t < tiles; ++t) {
      const int col0 = t * TILE;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = col0 + (c * G + gt) * V;
        if (STREAM) {                                         // the second read of the row
          load_chunk<T, V>(xr, col, N, vec, cr[c]);
          load_chunk<T, V>(xi, col, N, vec, ci[c]);
#pragma unroll
          for (int e = 0; e < V; ++e) {
            cr[c][e] -= mr;
            ci[c][e] -= mi;
          }
        }
        Affine<V> loaded;
        if (!PREG) load_affine<V>(a.w, a.b, col, N, vec, loaded);
        const Affine<V>& f = PREG ? areg[c] : loaded;
        float outr[V], outi[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float u = cr[c][e], v = ci[c][e];
          const float zr = fmaf(p, u, q * v), zi = fmaf(q, u, r * v);
          outr[e] = fmaf(f.w[0][e], zr, fmaf(f.w[1][e], zi, f.b[0][e]));
          outi[e] = fmaf(f.w[2][e], zr, fmaf(f.w[3][e], zi, f.b[1][e]));
        }
        store_chunk<T, V>(yr, col, N, vec, outr);
        store_chunk<T, V>(yi, col, N, vec, outi);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int KIND, int G, int C, bool STREAM>
__global__ __launch_bounds__(G > kFwdThreads ? G : kFwdThreads) void ln_bwd_kernel(Args a) {
  constexpr int V = 16 / sizeof(T), NT = G > kFwdThreads ? G : kFwdThreads, RPW = NT / G, TILE = G * C * V;
  constexpr int NS = KIND == CPLXAMD_LN_MODULUS ? 3 : 5, NR = KIND == CPLXAMD_LN_MODULUS ? 3 : 6;
  constexpr bool PREG = G == 64;
  __shared__ float lds[G > 64 ? 2 * 6 * (G / 64) : RPW * TILE];   // wave plan: the final exchange of the partials
  int round = 0;
  const int gt = threadIdx.x % G, sub = threadIdx.x / G;
  const int N = a.N, vec = a.vec;
  const float invN = 1.f / (float)N;
  const int tiles = STREAM ? (N + TILE - 1) / TILE : 1;
  const bool want_dx = a.o_r != nullptr, want_p = a.part != nullptr;
  float* mine = want_p ? a.part + (int64_t)blockIdx.x * 6 * N : nullptr;
  Affine<V> areg[PREG ? C : 1];
  if (PREG) {
#pragma unroll
    for (int c = 0; c < C; ++c) load_affine<V>(a.w, nullptr, (c * G + gt) * V, N, vec, areg[c]);
  }
  float acc[STREAM ? 1 : C][STREAM ? 1 : V][6];              // sum g y^T (4) and sum g (2) of the thread's columns
#pragma unroll
  for (int c = 0; c < (STREAM ? 1 : C); ++c)
#pragma unroll
    for (int e = 0; e < (STREAM ? 1 : V); ++e)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[c][e][j] = 0.f;
  bool first = true;
  for (int64_t row = (int64_t)blockIdx.x * RPW + sub; row < a.rows; row += (int64_t)gridDim.x * RPW) {
    int64_t xo, oo, go;
    row_offsets(a, row, xo, oo, go);
    const T *xr = reinterpret_cast<const T*>(a.x_r) + xo, *xi = reinterpret_cast<const T*>(a.x_i) + xo;
    const T *gr = reinterpret_cast<const T*>(a.g_r) + go, *gi = reinterpret_cast<const T*>(a.g_i) + go;
    T *dr = reinterpret_cast<T*>(a.o_r) + oo, *di = reinterpret_cast<T*>(a.o_i) + oo;
    const float* st = a.stats + row * NS;
    const float mr = st[0], mi = st[1], p = st[2], q = NS == 5 ? st[3] : 0.f, r = NS == 5 ? st[4] : p;
    float yr[C][V], yi[C][V], ur[C][V], ui[C][V];            // y and the upstream gradient g of the tile
    // y = P (x - m) and g of a chunk, zeros past N
    auto load = [&](int c, int col) {
      load_chunk<T, V>(xr, col, N, vec, yr[c]);
      load_chunk<T, V>(xi, col, N, vec, yi[c]);
      load_chunk<T, V>(gr, col, N, vec, ur[c]);
      load_chunk<T, V>(gi, col, N, vec, ui[c]);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const bool in = col + e < N;
        const float u = yr[c][e] - mr, v = yi[c][e] - mi;
        yr[c][e] = in ? fmaf(p, u, q * v) : 0.f;
        yi[c][e] = in ? fmaf(q, u, r * v) : 0.f;
      }
    };
    // g^ = W^T g over g, in place, and its part of the row sums
    auto pull = [&](int c, int col, float (&s)[NR], bool sums) {
      Affine<V> loaded;
      if (!PREG) load_affine<V>(a.w, nullptr, col, N, vec, loaded);
      const Affine<V>& f = PREG ? areg[c] : loaded;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float hr = fmaf(f.w[0][e], ur[c][e], f.w[2][e] * ui[c][e]);
        const float hi = fmaf(f.w[1][e], ur[c][e], f.w[3][e] * ui[c][e]);
        ur[c][e] = hr;
        ui[c][e] = hi;
        if (!sums) continue;
        s[0] += hr;
        s[1] += hi;
        if constexpr (KIND == CPLXAMD_LN_MODULUS) {
          s[2] = fmaf(hr, yr[c][e], fmaf(hi, yi[c][e], s[2]));
        } else {
          s[2] = fmaf(hr, yr[c][e], s[2]);
          s[3] = fmaf(hr, yi[c][e], s[3]);
          s[4] = fmaf(hi, yr[c][e], s[4]);
          s[5] = fmaf(hi, yi[c][e], s[5]);
        }
      }
    };
    float s[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) s[k] = 0.f;
    // pass 1: the parameter-gradient partials of the thread's columns (from g and y), then g^ and the row sums
    for (int t = 0; t < tiles; ++t) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = t * TILE + (c * G + gt) * V;
        load(c, col);
        if (want_p) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float v[6] = {ur[c][e] * yr[c][e], ur[c][e] * yi[c][e], ui[c][e] * yr[c][e], ui[c][e] * yi[c][e],
                                ur[c][e], ui[c][e]};
            if (!STREAM) {
#pragma unroll
              for (int j = 0; j < 6; ++j) acc[c][e][j] += v[j];
            } else if (col + e < N) {                         // past the registers: the workgroup's own slice, in place
#pragma unroll
              for (int j = 0; j < 6; ++j) {
                float* at = mine + (int64_t)j * N + col + e;
                *at = first ? v[j] : *at + v[j];
              }
            }
          }
        }
        if (want_dx) pull(c, col, s, true);
      }
    }
    first = false;
    if (!want_dx) continue;
    group_sum<G, NR>(s, lds, round);
#pragma unroll
    for (int k = 0; k < NR; ++k) s[k] *= invN;
    float z00, z01 = 0.f, z11;
    if constexpr (KIND == CPLXAMD_LN_MODULUS) {
      z00 = z11 = s[2];
    } else {
      const float ga = 0.5f * (s[3] - s[4]) / (p + r);
      z00 = fmaf(-2.f * q, ga, s[2]);
      z01 = fmaf(p - r, ga, 0.5f * (s[3] + s[4]));
      z11 = fmaf(2.f * q, ga, s[5]);
    }
    // pass 2: dx = P (g^ - mean g^ - Z y)
    for (int t = 0; t < tiles; ++t) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = t * TILE + (c * G + gt) * V;
        if (STREAM) {                                         // the second read of the row
          load(c, col);
          pull(c, col, s, false);
        }
        float outr[V], outi[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float vr = ur[c][e] - s[0] - fmaf(z00, yr[c][e], z01 * yi[c][e]);
          const float vi = ui[c][e] - s[1] - fmaf(z01, yr[c][e], z11 * yi[c][e]);
          outr[e] = fmaf(p, vr, q * vi);
          outi[e] = fmaf(q, vr, r * vi);
        }
        store_chunk<T, V>(dr, col, N, vec, outr);
        store_chunk<T, V>(di, col, N, vec, outi);
      }
    }
  }
  if (STREAM || !want_p) return;
  if (G > 64) {                                               // a thread owns its columns alone
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int col = (c * G + gt) * V + e;
        if (col < N) {
#pragma unroll
          for (int j = 0; j < 6; ++j) mine[(int64_t)j * N + col] = acc[STREAM ? 0 : c][STREAM ? 0 : e][j];
        }
      }
  } else {                                                    // the waves of the workgroup combine, one sum at a time
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < V; ++e) lds[sub * TILE + (c * G + gt) * V + e] = acc[STREAM ? 0 : c][STREAM ? 0 : e][j];
      __syncthreads();
      for (int col = threadIdx.x; col < TILE && col < N; col += NT) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < RPW; ++w) v += lds[w * TILE + col];
        mine[(int64_t)j * N + col] = v;
      }
      __syncthreads();
    }
  }
}

// dW [4][N] and dB [2][N]: the partials of the workgroups, summed in workgroup order
__global__ __launch_bounds__(256) void ln_finish_kernel(const float* part, int grid, int N, float* dw, float* db) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, total = 6 * (int64_t)N;
  if (idx >= total) return;
  double s = 0.0;
  for (int g = 0; g < grid; ++g) s += part[g * total + idx];
  if (idx < 4 * (int64_t)N)
    dw[idx] = (float)s;
  else
    db[idx - 4 * (int64_t)N] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static int plan_of(int64_t N, int64_t tile) { return N <= kWaveMax ? CPLXAMD_LN_WAVE : N <= tile ? CPLXAMD_LN_BLOCK : CPLXAMD_LN_STREAM; }

template <typename T, int KIND>
static int launch_fwd(const Args& a, int plan, int64_t grid, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const dim3 g((uint32_t)grid), b(kFwdThreads);
  if (plan == CPLXAMD_LN_WAVE)
    hipLaunchKernelGGL((ln_fwd_kernel<T, KIND, 64, kWaveCols / V, false>), g, b, 0, st, a);
  else if (plan == CPLXAMD_LN_BLOCK)
    hipLaunchKernelGGL((ln_fwd_kernel<T, KIND, kFwdThreads, kTile / kFwdThreads / V, false>), g, b, 0, st, a);
  else
    hipLaunchKernelGGL((ln_fwd_kernel<T, KIND, kFwdThreads, kTile / kFwdThreads / V, true>), g, b, 0, st, a);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}
template <typename T, int KIND>
static int launch_bwd(const Args& a, int plan, int64_t grid, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const dim3 g((uint32_t)grid);
  if (plan == CPLXAMD_LN_WAVE)
    hipLaunchKernelGGL((ln_bwd_kernel<T, KIND, 64, kWaveCols / V, false>), g, dim3(kFwdThreads), 0, st, a);
  else if (plan == CPLXAMD_LN_BLOCK)
    hipLaunchKernelGGL((ln_bwd_kernel<T, KIND, kBwdThreads, kBwdTile / kBwdThreads / V, false>), g, dim3(kBwdThreads), 0, st, a);
  else
    hipLaunchKernelGGL((ln_bwd_kernel<T, KIND, kBwdThreads, kBwdTile / kBwdThreads / V, true>), g, dim3(kBwdThreads), 0, st, a);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

static bool mult(const int64_t (&st)[3], int v) { return st[0] % v == 0 && st[1] % v == 0 && st[2] % v == 0; }

// validate the descriptor and bring it into kernel form
static int make_args(const cplxamd_ln_desc& d, int dtype, Args& a) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (d.kind != CPLXAMD_LN_WHITEN && d.kind != CPLXAMD_LN_MODULUS) return CPLXAMD_EINVAL;
  if (d.N < 1 || !std::isfinite(d.eps) || d.eps < 0) return CPLXAMD_EINVAL;
  if (d.N > (1 << 30)) return CPLXAMD_ESHAPE;
  using D = cplxamd_ln_desc;
  int64_t size[3];
  const sp::RunStride<D> f[3] = {{&D::x_stride, a.xs}, {&D::o_stride, a.os}, {&D::g_stride, a.gs}};
  if (const int rc = sp::decode_runs(d, f, size, a.rows)) return rc;
  a.size1 = size[1];
  a.size2 = size[2];
  a.one_run = size[0] == 1 && size[1] == 1;
  a.N = (int)d.N;
  a.eps = (float)d.eps;
  return 0;
}

}  // namespace ln
}  // namespace cplxamd

using namespace cplxamd;

static_assert(sizeof(cplxamd_ln_desc) == 120, "cplxamd_ln_desc is 120 bytes");

extern "C" int cplxamd_ln_plan(int64_t rows, int64_t N, int kind, int dtype, int64_t* plan) {
  if (!plan || rows < 0 || N < 1 || (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) ||
      (kind != CPLXAMD_LN_WHITEN && kind != CPLXAMD_LN_MODULUS))
    return CPLXAMD_EINVAL;
  if (N > (1 << 30)) return CPLXAMD_ESHAPE;
  const int p = ln::plan_of(N, ln::kTile);
  const bool wave = p == CPLXAMD_LN_WAVE;
  const int64_t rpw = wave ? ln::kFwdThreads / 64 : 1, wgs = (rows + rpw - 1) / rpw;
  const int64_t fwd_cap = wave ? ln::kFwdGridWave : ln::kFwdGridBlock, per_wg = 6 * 4 * N;
  int64_t bwd = wave ? ln::kBwdGridWave : ln::kBwdGridBlock;
  if (bwd > ln::kWsCap / per_wg) bwd = ln::kWsCap / per_wg;        // long rows: fewer workgroups
  if (bwd < 1) bwd = 1;
  if (bwd > wgs) bwd = wgs;
  plan[CPLXAMD_LN_PLAN] = p;
  plan[CPLXAMD_LN_THREADS] = ln::kFwdThreads;
  plan[CPLXAMD_LN_ROWS_PER_WG] = rpw;
  plan[CPLXAMD_LN_TILE] = wave ? ln::kWaveMax : ln::kTile;
  plan[CPLXAMD_LN_GRID] = wgs < fwd_cap ? wgs : fwd_cap;
  plan[CPLXAMD_LN_SEAM_WAVE] = ln::kWaveMax;
  plan[CPLXAMD_LN_SEAM_BLOCK] = ln::kTile;
  plan[CPLXAMD_LN_BWD_THREADS] = wave ? ln::kFwdThreads : ln::kBwdThreads;
  plan[CPLXAMD_LN_BWD_ROWS_PER_WG] = rpw;
  plan[CPLXAMD_LN_BWD_GRID] = bwd;
  plan[CPLXAMD_LN_WS_BYTES] = bwd * per_wg;
  plan[CPLXAMD_LN_WS_CAP] = ln::kWsCap > per_wg ? ln::kWsCap : per_wg;
  plan[CPLXAMD_LN_STAT_FLOATS] = kind == CPLXAMD_LN_MODULUS ? 3 : 5;
  plan[CPLXAMD_LN_BWD_PLAN] = ln::plan_of(N, ln::kBwdTile);
  plan[CPLXAMD_LN_BWD_SEAM_BLOCK] = ln::kBwdTile;
  return 0;
}

extern "C" int cplxamd_ln_fwd(const void* x_r, const void* x_i, const float* weight, const float* bias, void* y_r, void* y_i,
                              float* stats, const cplxamd_ln_desc* d, int dtype, void* stream) {
  if (!x_r || !x_i || !y_r || !y_i || !stats || !d || (bias && !weight)) return CPLXAMD_EINVAL;
  ln::Args a{};
  int64_t plan[CPLXAMD_LN_PLAN_FIELDS];
  if (const int rc = ln::make_args(*d, dtype, a)) return rc;
  if (a.rows == 0) return 0;
  if (const int rc = cplxamd_ln_plan(a.rows, d->N, d->kind, dtype, plan)) return rc;
  a.x_r = x_r; a.x_i = x_i; a.o_r = y_r; a.o_i = y_i; a.stats = stats; a.w = weight; a.b = bias;
  const int v = dtype == CPLXAMD_BF16 ? 8 : 4;
  a.vec = a.N % v == 0 && aligned16(x_r) && aligned16(x_i) && aligned16(y_r) && aligned16(y_i) && aligned16(weight) &&
          aligned16(bias) && ln::mult(a.xs, v) && ln::mult(a.os, v);
  hipStream_t st = (hipStream_t)stream;
  const int p = (int)plan[CPLXAMD_LN_PLAN];
  const int64_t grid = plan[CPLXAMD_LN_GRID];
  const bool mod = d->kind == CPLXAMD_LN_MODULUS;
  if (dtype == CPLXAMD_BF16)
    return mod ? ln::launch_fwd<bf16_t, CPLXAMD_LN_MODULUS>(a, p, grid, st) : ln::launch_fwd<bf16_t, CPLXAMD_LN_WHITEN>(a, p, grid, st);
  return mod ? ln::launch_fwd<float, CPLXAMD_LN_MODULUS>(a, p, grid, st) : ln::launch_fwd<float, CPLXAMD_LN_WHITEN>(a, p, grid, st);
}

extern "C" int cplxamd_ln_bwd(const void* x_r, const void* x_i, const void* g_r, const void* g_i, const float* weight,
                              const float* stats, void* dx_r, void* dx_i, float* dweight, float* dbias,
                              const cplxamd_ln_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!x_r || !x_i || !g_r || !g_i || !stats || !d) return CPLXAMD_EINVAL;
  // dx may be left out (both planes NULL), and so may dweight with dbias: what is not asked for is not computed
  const bool want_dx = dx_r != nullptr, want_p = dweight != nullptr;
  if ((dx_i != nullptr) != want_dx || (dbias != nullptr) != want_p || (want_p && !ws)) return CPLXAMD_EINVAL;
  ln::Args a{};
  int64_t plan[CPLXAMD_LN_PLAN_FIELDS];
  if (const int rc = ln::make_args(*d, dtype, a)) return rc;
  if (a.rows == 0 || !(want_dx || want_p)) return 0;
  if (const int rc = cplxamd_ln_plan(a.rows, d->N, d->kind, dtype, plan)) return rc;
  if (want_p && ws_bytes < plan[CPLXAMD_LN_WS_BYTES]) return CPLXAMD_EWS;
  a.x_r = x_r; a.x_i = x_i; a.g_r = g_r; a.g_i = g_i; a.o_r = dx_r; a.o_i = dx_i;
  a.stats = const_cast<float*>(stats); a.w = weight; a.part = want_p ? reinterpret_cast<float*>(ws) : nullptr;
  const int v = dtype == CPLXAMD_BF16 ? 8 : 4;
  a.vec = a.N % v == 0 && aligned16(x_r) && aligned16(x_i) && aligned16(g_r) && aligned16(g_i) && aligned16(dx_r) &&
          aligned16(dx_i) && aligned16(weight) && ln::mult(a.xs, v) && ln::mult(a.os, v) && ln::mult(a.gs, v);
  hipStream_t st = (hipStream_t)stream;
  const int p = (int)plan[CPLXAMD_LN_BWD_PLAN];
  const int64_t grid = plan[CPLXAMD_LN_BWD_GRID];
  const bool mod = d->kind == CPLXAMD_LN_MODULUS;
  int rc;
  if (dtype == CPLXAMD_BF16)
    rc = mod ? ln::launch_bwd<bf16_t, CPLXAMD_LN_MODULUS>(a, p, grid, st) : ln::launch_bwd<bf16_t, CPLXAMD_LN_WHITEN>(a, p, grid, st);
  else
    rc = mod ? ln::launch_bwd<float, CPLXAMD_LN_MODULUS>(a, p, grid, st) : ln::launch_bwd<float, CPLXAMD_LN_WHITEN>(a, p, grid, st);
  if (rc || !want_p) return rc;
  const int64_t total = 6 * d->N;
  hipLaunchKernelGGL(ln::ln_finish_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, a.part, (int)grid, a.N,
                     dweight, dbias);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}
