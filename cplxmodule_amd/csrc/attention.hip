// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
// Scaled dot-product attention of planar complex tensors (cplx.scaled_dot_product_attention).
//
//   c = q k^H,   s = scale Re c  |  scale |c|,   p = softmax_j s (real),   o = p v (complex)
//
// FORWARD: one launch, a flash kernel on the matrix instructions.  A workgroup of four waves owns 128 queries of one
// batch entry, a wave 32 of them; the keys go by in tiles of 32 (float32) or 64 (bf16) through two LDS stages, the
// global loads of tile t + 1 in flight (in registers) while tile t is multiplied.  The scores are computed TRANSPOSED,
// S^T = K Q^H: in the 32x32 accumulator (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) a lane then
// holds ONE query and 16 keys, so the running maximum and sum of the online softmax are in-register reductions plus
// one exchange between the half-waves, and every rescale is a per-lane scalar.  `real` is one chain of depth 2 E over
// the concatenated planes [k_r | k_i] . [q_r | q_i]; `abs` adds the two products of Im c on the same K fragments.
// The accumulator's key-to-register assignment IS the B operand of O^T = V^T P^T: a sum over keys does not care about
// their order, the V tile is read from LDS in the matching key permutation, and P never leaves the registers.
// Nothing of size L x S exists anywhere; keys are summed in ascending order (same input, same bits); no scratch (the
// compiler reports 0 bytes for every instance: DESIGN 25.3), no atomics, nothing read on the host.
//
// BACKWARD: three launches -- D_i = Re(g^H o)_i; one workgroup per 32 queries walks the keys and writes dq; one per 32
// keys walks the queries and writes dk, dv.  p is recomputed from q, k and the saved log-sum-exp; 32 x 32 tiles in LDS as
// float32, every tile product on v_mfma_f32_32x32x2_f32 for both dtypes; no atomics (limits: 25.5).
#include <cmath>
#include <type_traits>

#include "common.h"
#include "launch.h"
#include "prims.h"
#include "runs.h"

namespace cplxamd {
namespace attn {

constexpr int QT = 128;                       // queries per workgroup of the forward
constexpr int BT = 32;                        // rows per tile of the backward kernels
constexpr float kLog2e = 1.4426950408889634f;

struct Args {
  const void *q_r, *q_i, *k_r, *k_i, *v_r, *v_i;
  void *o_r, *o_i;
  float* lse;
  const void *g_r, *g_i;
  void *dq_r, *dq_i, *dk_r, *dk_i, *dv_r, *dv_i;
  float* dvec;
  int L, S, E, Ev, causal, tiles, vecq, veck, vecv;
  float scale;
  int64_t size[3];
  int64_t bq[3], bk[3], bv[3], bo[3], bl[3], bdq[3], bdk[3], bdv[3];
  int64_t rq, rk, rv, ro, rdq, rdk, rdv;
};

// offsets of batch entry b in every tensor at once would cost registers: one tensor per call
__device__ __forceinline__ int64_t batch_off(const Args& g, int64_t b, const int64_t (&st)[3]) {
  const int64_t i2 = b % g.size[2], w = b / g.size[2], i1 = w % g.size[1], i0 = w / g.size[1];
  return i0 * st[0] + i1 * st[1] + i2 * st[2];
}

template <typename T, int DP>
struct Fwd {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int KT = BF ? 64 : 32, NS = KT / 32;   // keys per stage, 32-key subtiles
  static constexpr int KD = BF ? 16 : 2;                   // contraction depth of one matrix instruction
  static constexpr int NQ = 2 * DP / KD;                   // steps of the chain over both planes
  static constexpr int NE = DP / 32;                       // 32-row tiles of O^T per plane
  // K rows [k_r | k_i]: float32 2 DP + 1 floats (odd: the 32 rows of a fragment read fall into distinct banks), bf16
  // 2 DP + 8 (16-byte rows, 16-byte slots rotate).  V: float32 as K; bf16 TRANSPOSED, [plane, ev][keys + 4].
  static constexpr int LDK = BF ? 2 * DP + 8 : 2 * DP + 1;
  static constexpr int LDV = BF ? KT + 4 : 2 * DP + 1;
  static constexpr int KBYTES = KT * LDK * (int)sizeof(T);
  static constexpr int VBYTES = BF ? 2 * DP * LDV * 2 : KT * LDV * 4;
  static constexpr int STAGE = (KBYTES + VBYTES + 15) / 16 * 16;
  static constexpr int LDS = 2 * STAGE;
  // what a thread holds of a tile in flight: float32 single elements, bf16 16-byte chunks (V: of a PAIR of keys)
  static constexpr int KCH = BF ? KT * 2 * DP / 8 / 256 : KT * 2 * DP / 256;
  static constexpr int VCH = BF ? (KT / 2) * 2 * DP / 8 / 256 : KT * 2 * DP / 256;
  static_assert(KBYTES % 16 == 0, "V stage alignment");
};

__device__ __forceinline__ uint4 load8(const bf16_t* p, int nvalid, bool vec) {
  if (nvalid <= 0) return make_uint4(0, 0, 0, 0);
  if (vec && nvalid >= 8) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t lo = 2 * u < nvalid ? p[2 * u] : 0, hi = 2 * u + 1 < nvalid ? p[2 * u + 1] : 0;
    w[u] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename T, int DP> struct TileRegs;
template <int DP> struct TileRegs<float, DP> {
  float k[Fwd<float, DP>::KCH], v[Fwd<float, DP>::VCH];
};
template <int DP> struct TileRegs<bf16_t, DP> {
  uint4 k[Fwd<bf16_t, DP>::KCH], v[Fwd<bf16_t, DP>::VCH][2];
};

// global -> registers: the key tile at k0, both planes of K and V; rows past S and columns past E / Ev are zeros
template <int DP>
__device__ __forceinline__ void fetch(TileRegs<float, DP>& o, const Args& g, const float* kr, const float* ki, const float* vr,
                                      const float* vi, int k0) {
  using F = Fwd<float, DP>;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // addresses are rebuilt per tile, not kept in registers across the loop
#pragma unroll
  for (int n = 0; n < F::KCH; ++n) {
    const int c = tid + 256 * n, col = c % DP, rest = c / DP, pl = rest & 1, key = k0 + (rest >> 1);
    const bool ok = key < g.S;
    o.k[n] = ok && col < g.E ? (pl ? ki : kr)[(int64_t)key * g.rk + col] : 0.0f;
    o.v[n] = ok && col < g.Ev ? (pl ? vi : vr)[(int64_t)key * g.rv + col] : 0.0f;
  }
}
template <int DP>
__device__ __forceinline__ void commit(const TileRegs<float, DP>& o, char* stage) {
  using F = Fwd<float, DP>;
  float* sK = reinterpret_cast<float*>(stage);
  float* sV = reinterpret_cast<float*>(stage + F::KBYTES);
#pragma unroll
  for (int n = 0; n < F::KCH; ++n) {
    const int c = threadIdx.x + 256 * n, col = c % DP, rest = c / DP, pl = rest & 1, row = rest >> 1;
    sK[row * F::LDK + pl * DP + col] = o.k[n];
    sV[row * F::LDV + pl * DP + col] = o.v[n];
  }
}
template <int DP>
__device__ __forceinline__ void fetch(TileRegs<bf16_t, DP>& o, const Args& g, const bf16_t* kr, const bf16_t* ki,
                                      const bf16_t* vr, const bf16_t* vi, int k0) {
  using F = Fwd<bf16_t, DP>;
  constexpr int CPR = DP / 8;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // addresses are rebuilt per tile, not kept in registers across the loop
#pragma unroll
  for (int n = 0; n < F::KCH; ++n) {
    const int c = tid + 256 * n, cc = c % CPR, rest = c / CPR, pl = rest & 1, key = k0 + (rest >> 1);
    o.k[n] = load8((pl ? ki : kr) + (int64_t)key * g.rk + 8 * cc, key < g.S ? g.E - 8 * cc : 0, g.veck);
  }
#pragma unroll
  for (int n = 0; n < F::VCH; ++n) {
    const int c = tid + 256 * n, kp = c & 31, rest = c >> 5, cc = rest % CPR, pl = rest / CPR;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = k0 + 2 * kp + u;
      o.v[n][u] = load8((pl ? vi : vr) + (int64_t)key * g.rv + 8 * cc, key < g.S ? g.Ev - 8 * cc : 0, g.vecv);
    }
  }
}
template <int DP>
__device__ __forceinline__ void commit(const TileRegs<bf16_t, DP>& o, char* stage) {
  using F = Fwd<bf16_t, DP>;
  constexpr int CPR = DP / 8;
  char* sK = stage;
  char* sV = stage + F::KBYTES;
#pragma unroll
  for (int n = 0; n < F::KCH; ++n) {
    const int c = threadIdx.x + 256 * n, cc = c % CPR, rest = c / CPR, pl = rest & 1, row = rest >> 1;
    *reinterpret_cast<uint4*>(sK + (row * F::LDK + pl * DP + 8 * cc) * 2) = o.k[n];
  }
  // transposed: element e of the two loads = (ev 8 cc + e; keys 2 kp, 2 kp + 1), one 4-byte write; kp is the fastest
  // index across lanes, so the 32 writes of a half-wave are consecutive words of one row
#pragma unroll
  for (int n = 0; n < F::VCH; ++n) {
    const int c = threadIdx.x + 256 * n, kp = c & 31, rest = c >> 5, cc = rest % CPR, pl = rest / CPR;
    const uint32_t w0[4] = {o.v[n][0].x, o.v[n][0].y, o.v[n][0].z, o.v[n][0].w};
    const uint32_t w1[4] = {o.v[n][1].x, o.v[n][1].y, o.v[n][1].z, o.v[n][1].w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int sh = (e & 1) * 16;
      *reinterpret_cast<uint32_t*>(sV + ((pl * DP + 8 * cc + e) * F::LDV + 2 * kp) * 2) =
          ((w0[e >> 1] >> sh) & 0xffffu) | ((w1[e >> 1] >> sh) << 16);
    }
  }
}

__device__ __forceinline__ f32x16 mma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <typename T, int DP, bool ABS>
__global__ __launch_bounds__(256) void attn_fwd_kernel(Args g) {
  using F = Fwd<T, DP>;
  constexpr bool BF = F::BF;
  constexpr int KT = F::KT, NS = F::NS, KD = F::KD, NQ = F::NQ, NE = F::NE;
  using Frag = std::conditional_t<BF, bf16x8, float>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // heavy (late, under a causal mask) query tiles first
  const int tile = g.tiles - 1 - (int)(blockIdx.x % (uint32_t)g.tiles);
  const int64_t b = blockIdx.x / (uint32_t)g.tiles;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l31 = lane & 31, lk = lane >> 5;
  const int q0 = tile * QT, wq0 = q0 + 32 * wid, qrow = wq0 + l31;
  const T* qr = reinterpret_cast<const T*>(g.q_r) + batch_off(g, b, g.bq);
  const T* qi = reinterpret_cast<const T*>(g.q_i) + batch_off(g, b, g.bq);
  const int64_t ko = batch_off(g, b, g.bk), vo = batch_off(g, b, g.bv);
  const T *kr = reinterpret_cast<const T*>(g.k_r) + ko, *ki = reinterpret_cast<const T*>(g.k_i) + ko;
  const T *vr = reinterpret_cast<const T*>(g.v_r) + vo, *vi = reinterpret_cast<const T*>(g.v_i) + vo;

  // the wave's queries as B fragments of the whole chain [q_r | q_i], zeros past L and E
  Frag qf[NQ];
#pragma unroll
  for (int s = 0; s < NQ; ++s) {
    constexpr int HALF = KD / 2;
    const int pl = s * KD >= DP, e0 = s * KD - pl * DP + lk * HALF;
    const T* src = (pl ? qi : qr) + (int64_t)qrow * g.rq + e0;
    const bool rok = qrow < g.L;
    if constexpr (BF) {
      qf[s] = __builtin_bit_cast(bf16x8, load8(src, rok ? g.E - e0 : 0, g.vecq));
    } else {
      qf[s] = rok && e0 < g.E ? *src : 0.0f;
    }
  }

  f32x16 acc[NE][2];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e][0] = acc[e][1] = f32x16{0};
  float m = -INFINITY, l = 0.0f;

  int nt = (g.S + KT - 1) / KT;
  if (g.causal) {
    const int last = min(q0 + QT, g.L) - 1;             // keys past the last query of the tile are never visible
    nt = min(nt, last / KT + 1);
  }
  TileRegs<T, DP> regs;
  fetch<DP>(regs, g, kr, ki, vr, vi, 0);
  for (int t = 0; t < nt; ++t) {
    char* stage = smem + (t & 1) * F::STAGE;
    commit<DP>(regs, stage);
    __syncthreads();          // one barrier per tile: the other stage is rewritten only after everyone passed this one
    if (t + 1 < nt) fetch<DP>(regs, g, kr, ki, vr, vi, (t + 1) * KT);
    const int k0 = t * KT;
    bool live[NS], any = false;
#pragma unroll
    for (int sub = 0; sub < NS; ++sub) {
      const int kb = k0 + 32 * sub;
      live[sub] = kb < g.S && !(g.causal && kb > wq0 + 31);   // wave-uniform: subtiles wholly above the diagonal are skipped
      any |= live[sub];
    }
    if (!any) continue;

    // ---- S^T = K Q^H on this tile: sc[sub][r] = score of key k0 + 32 sub + (r & 3) + 8 (r >> 2) + 4 lk and query qrow
    float sc[NS][16];
#pragma unroll
    for (int sub = 0; sub < NS; ++sub) {
      if (!live[sub]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[sub][r] = -INFINITY;
        continue;
      }
      f32x16 cr = f32x16{0}, ca = f32x16{0}, cb = f32x16{0};
#pragma unroll
      for (int s = 0; s < NQ; ++s) {
        // (every step of the compiled head runs: columns past E are zeros in LDS and in qf.  Uniform branches around
        // the steps past E cost up to 680 bytes of scratch per lane at head 128 -- the allocator spilled the
        // accumulators across the blocks they made)
        Frag a;
        if constexpr (BF)
          a = *reinterpret_cast<const bf16x8*>(stage + ((32 * sub + l31) * F::LDK + s * KD + 8 * lk) * 2);
        else
          a = reinterpret_cast<const float*>(stage)[(32 * sub + l31) * F::LDK + s * KD + lk];
        cr = mma(a, qf[s], cr);
        if constexpr (ABS) {                                  // Im c = q_i . k_r - q_r . k_i, on the same K fragments
          if (s < NQ / 2)
            ca = mma(a, qf[s + NQ / 2], ca);
          else
            cb = mma(a, qf[s - NQ / 2], cb);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * lk;
        float s;
        if constexpr (ABS) {
          const float im = ca[r] - cb[r];
          s = g.scale * sqrtf(cr[r] * cr[r] + im * im);
        } else {
          s = g.scale * cr[r];
        }
        sc[sub][r] = key >= g.S || (g.causal && key > qrow) ? -INFINITY : s;
      }
    }

    // ---- online softmax: per lane (= per query), one exchange with the other half-wave.  Key 0 is visible to every
    // query and lies in tile 0, so the running maximum is finite from the first tile on
    float tmax = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < NS; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sc[sub][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);
    const float alpha = exp2f((m - mn) * kLog2e);
    m = mn;
    float ps = 0.0f;
#pragma unroll
    for (int sub = 0; sub < NS; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[sub][r] = exp2f((sc[sub][r] - mn) * kLog2e);
        ps += sc[sub][r];
      }
    l = l * alpha + ps;                                       // (per half-wave; the halves are added at the end)
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      acc[e][0] *= alpha;
      acc[e][1] *= alpha;
    }

    // ---- O^T += V^T P^T: the score registers are the B operand as they are
    const char* sVb = stage + F::KBYTES;
#pragma unroll
    for (int sub = 0; sub < NS; ++sub) {
      if (!live[sub]) continue;
      if constexpr (BF) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 pw = make_uint4(pack_bf16(sc[sub][8 * h], sc[sub][8 * h + 1]), pack_bf16(sc[sub][8 * h + 2], sc[sub][8 * h + 3]),
                                      pack_bf16(sc[sub][8 * h + 4], sc[sub][8 * h + 5]), pack_bf16(sc[sub][8 * h + 6], sc[sub][8 * h + 7]));
          const bf16x8 pb = __builtin_bit_cast(bf16x8, pw);
          const int col = 32 * sub + 16 * h + 4 * lk;         // keys col .. col + 3 and col + 8 .. col + 11
#pragma unroll
          for (int e = 0; e < NE; ++e) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
              const char* row = sVb + ((pl * DP + 32 * e + l31) * F::LDV + col) * 2;
              const uint2 lo = *reinterpret_cast<const uint2*>(row), hi = *reinterpret_cast<const uint2*>(row + 16);
              const bf16x8 a = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
              acc[e][pl] = mma(a, pb, acc[e][pl]);
            }
          }
        }
      } else {
        const float* sV = reinterpret_cast<const float*>(sVb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int krow = 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * lk;
#pragma unroll
          for (int e = 0; e < NE; ++e) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
              acc[e][pl] = mma(sV[krow * F::LDV + pl * DP + 32 * e + l31], sc[sub][r], acc[e][pl]);
          }
        }
      }
    }
  }

  // ---- o = O / l, lse = m + log l
  l += __shfl_xor(l, 32, 64);
  if (qrow >= g.L) return;
  const float inv = 1.0f / l;
  const int64_t oo = batch_off(g, b, g.bo) + (int64_t)qrow * g.ro;
  T *orp = reinterpret_cast<T*>(g.o_r) + oo, *oip = reinterpret_cast<T*>(g.o_i) + oo;
#pragma unroll
  for (int e = 0; e < NE; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ev = 32 * e + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (ev < g.Ev) {
        io<T>::st(orp + ev, acc[e][0][r] * inv);
        io<T>::st(oip + ev, acc[e][1][r] * inv);
      }
    }
  if (lk == 0) g.lse[batch_off(g, b, g.bl) + qrow] = m + logf(l);
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
// D[b][i] = Re(g^H o)_i = sum_ev g_r o_r + g_i o_i, one thread per (batch, query)
template <typename T>
__global__ __launch_bounds__(256) void attn_dvec_kernel(Args g, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / g.L, off = batch_off(g, b, g.bo) + (idx % g.L) * g.ro;
  const T *orp = reinterpret_cast<const T*>(g.o_r) + off, *oip = reinterpret_cast<const T*>(g.o_i) + off;
  const T *grp = reinterpret_cast<const T*>(g.g_r) + off, *gip = reinterpret_cast<const T*>(g.g_i) + off;
  float s = 0.0f;
  for (int e = 0; e < g.Ev; ++e) s += io<T>::ld(grp + e) * io<T>::ld(orp + e) + io<T>::ld(gip + e) * io<T>::ld(oip + e);
  g.dvec[idx] = s;
}

// 32 rows [re | im] of a tensor as floats, zeros past `rows`: a thread owns one column (n <= 128) of every other row, and
// all of its 32 loads are in flight before the first is stored (one workgroup per CU: nothing else hides their latency)
template <typename T>
__device__ __forceinline__ void load_rows(float* dst, int ld, const T* pr, const T* pi, int64_t rs, int row0, int rows, int n) {
  const int col = threadIdx.x & 127, r0 = threadIdx.x >> 7;
  if (col >= n) return;
  float v[BT];
#pragma unroll
  for (int i = 0; i < BT / 2; ++i) {
    const int r = row0 + r0 + 2 * i;
    const int64_t off = (int64_t)r * rs + col;
    v[2 * i] = r < rows ? io<T>::ld(pr + off) : 0.0f;
    v[2 * i + 1] = r < rows ? io<T>::ld(pi + off) : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < BT / 2; ++i) {
    dst[(r0 + 2 * i) * ld + col] = v[2 * i];
    dst[(r0 + 2 * i) * ld + n + col] = v[2 * i + 1];
  }
}

// OWNK = false: the workgroup owns 32 queries, walks the key tiles and writes dq = dC K.
// OWNK = true:  it owns 32 keys, walks the query tiles and writes dk = dC^H Q and dv = P^T G.
// dC = scale dS (real) or scale dS C / |C| (abs; 0 where |C| = 0), dS = P (dP - D), dP = G_r V_r^T + G_i V_i^T.
template <typename T, bool ABS, bool OWNK>
__global__ __launch_bounds__(256) void attn_bwd_kernel(Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int E = g.E, Ev = g.Ev, LQ = 2 * E + 1, LG = 2 * Ev + 1, LP = BT + 1;
  float* sQ = reinterpret_cast<float*>(smem);       // queries [q_r | q_i]
  float* sG = sQ + BT * LQ;                          // their upstream gradients [g_r | g_i]
  float* sK = sG + BT * LG;                          // keys
  float* sV = sK + BT * LQ;                          // values
  float* sP = sV + BT * LG;                          // [owner][visitor]: p, Re dC, Im dC
  float* sA = sP + BT * LP;
  float* sB = sA + BT * LP;
  float* sC = sB + BT * LP;                          // (the second half of dP)
  float* sLse = sC + BT * LP;
  float* sD = sLse + BT;

  const int tile = blockIdx.x % (uint32_t)g.tiles;
  const int64_t b = blockIdx.x / (uint32_t)g.tiles;
  const int own0 = tile * BT;
  const int64_t qo = batch_off(g, b, g.bq), ko = batch_off(g, b, g.bk), vo = batch_off(g, b, g.bv), go = batch_off(g, b, g.bo);
  const T *qr = reinterpret_cast<const T*>(g.q_r) + qo, *qi = reinterpret_cast<const T*>(g.q_i) + qo;
  const T *kr = reinterpret_cast<const T*>(g.k_r) + ko, *ki = reinterpret_cast<const T*>(g.k_i) + ko;
  const T *vr = reinterpret_cast<const T*>(g.v_r) + vo, *vi = reinterpret_cast<const T*>(g.v_i) + vo;
  const T *gr = reinterpret_cast<const T*>(g.g_r) + go, *gi = reinterpret_cast<const T*>(g.g_i) + go;
  const float* lse = g.lse + batch_off(g, b, g.bl);
  const float* dvec = g.dvec + b * g.L;

  auto load_q = [&](int q0) {
    load_rows<T>(sQ, LQ, qr, qi, g.rq, q0, g.L, E);
    load_rows<T>(sG, LG, gr, gi, g.ro, q0, g.L, Ev);
    if (threadIdx.x < BT) {
      const int q = q0 + threadIdx.x;
      sLse[threadIdx.x] = q < g.L ? lse[q] : 0.0f;
      sD[threadIdx.x] = q < g.L ? dvec[q] : 0.0f;
    }
  };
  auto load_k = [&](int k0) {
    load_rows<T>(sK, LQ, kr, ki, g.rk, k0, g.S, E);
    load_rows<T>(sV, LG, vr, vi, g.rv, k0, g.S, Ev);
  };

  int t_lo = 0, t_hi;
  if (OWNK) {
    load_k(own0);
    t_hi = (g.L + BT - 1) / BT;
    if (g.causal) t_lo = own0 / BT;                   // queries before the tile's first key see none of its keys
  } else {
    load_q(own0);
    t_hi = (g.S + BT - 1) / BT;
    if (g.causal) t_hi = min(t_hi, (min(own0 + BT, g.L) - 1) / BT + 1);
  }

  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l31 = lane & 31, lk = lane >> 5;
  const int o = threadIdx.x >> 3, dl = threadIdx.x & 7;       // the pointwise phase: pairs (o, dl + 8 mm)
  const int T1 = (2 * E + 31) / 32, T2 = OWNK ? (2 * Ev + 31) / 32 : 0;   // 32-column tiles of [d_r | d_i] (and of dv)
  f32x16 acc[4];                                              // wave w owns column tiles w, w + 4, ...
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) acc[jj] = f32x16{0};

  // D[o][v] = sum_x A[o][x] B[v][x] over the depth steps [s0, s1) (x = 2 s + lk): A rows are the owner's, B the visitor's
  auto chain = [&](const float* A, const float* B, int ld, int s0, int s1) {
    f32x16 c = f32x16{0};
    const float *pa = A + l31 * ld + lk, *pb = B + l31 * ld + lk;
#pragma unroll 8
    for (int s = s0; s < s1; ++s) c = mma(pa[2 * s], pb[2 * s], c);
    return c;
  };
  auto put = [&](float* dst, const f32x16& c) {               // accumulator -> [owner][visitor] tile
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * lk) * LP + l31] = c[r];
  };

  for (int t = t_lo; t < t_hi; ++t) {
    const int vis0 = t * BT;
    __syncthreads();                                  // the last tile's products are done with the visitor rows
    if (OWNK) load_q(vis0); else load_k(vis0);
    __syncthreads();
    // ---- the 32 x 32 tiles Re c, Im c and dP on the float32 matrix instruction, one chain (or half of one) per wave:
    // real: Re c in two halves (sA, sB), dP in two halves (sP, sC); abs: Re c (sA), Im c (sB), dP in halves (sP, sC)
    {
      const float *ownQK = OWNK ? sK : sQ, *visQK = OWNK ? sQ : sK, *ownGV = OWNK ? sV : sG, *visGV = OWNK ? sG : sV;
      if (wid >= 2) {
        const int h = Ev / 2;
        put(wid == 2 ? sP : sC, wid == 2 ? chain(ownGV, visGV, LG, 0, h) : chain(ownGV, visGV, LG, h, Ev));
      } else if (!ABS) {
        const int h = E / 2;
        put(wid == 0 ? sA : sB, wid == 0 ? chain(ownQK, visQK, LQ, 0, h) : chain(ownQK, visQK, LQ, h, E));
      } else if (wid == 0) {
        put(sA, chain(ownQK, visQK, LQ, 0, E));
      } else {                                        // Im c = sum_d q_i k_r - q_r k_i: k as it lies, q from the other plane
        f32x16 c = f32x16{0};
        const float *qrow = sQ + l31 * LQ, *krow = sK + l31 * LQ;
#pragma unroll 8
        for (int s = 0; s < E; ++s) {
          const int x = 2 * s + lk;
          const float qv = x < E ? qrow[x + E] : -qrow[x - E], kv = krow[x];
          c = OWNK ? mma(kv, qv, c) : mma(qv, kv, c);
        }
        put(sB, c);
      }
    }
    __syncthreads();
    // ---- pointwise: p, dS and dC of the 32 x 32 pairs, four per thread, in place
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const int v = dl + 8 * mm, at = o * LP + v;
      const int qi_ = OWNK ? v : o, ki_ = OWNK ? o : v;
      const float cr = ABS ? sA[at] : sA[at] + sB[at], ci = ABS ? sB[at] : 0.0f, dp = sP[at] + sC[at];
      const int qg = (OWNK ? vis0 : own0) + qi_, kg = (OWNK ? own0 : vis0) + ki_;
      const bool valid = qg < g.L && kg < g.S && !(g.causal && kg > qg);
      const float mod = ABS ? sqrtf(cr * cr + ci * ci) : 0.0f;
      const float s = g.scale * (ABS ? mod : cr);
      const float p = valid ? expf(s - sLse[qi_]) : 0.0f;
      const float ds = g.scale * p * (dp - sD[qi_]);
      sP[at] = p;
      if (ABS) {
        const float w = mod > 0.0f ? ds / mod : 0.0f;
        sA[at] = w * cr;
        sB[at] = w * ci;
      } else {
        sA[at] = ds;
      }
    }
    __syncthreads();
    // ---- the owner's sums over the 32 visitors, again on the matrix instruction: D[o][c] += sum_v coef[o][v] X[v][c],
    // c a column of [d_r | d_i] (coef = Re dC, and Im dC against the other plane with its sign) or of dv (coef = p)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = wid + 4 * jj;
      if (j >= T1 + T2) break;
      const bool isv = j >= T1;
      const int c = l31 + 32 * (isv ? j - T1 : j), half = isv ? Ev : E;
      const bool ok = c < 2 * half;
      const int cc = ok ? c : 0, ldx = isv ? LG : LQ;
      const float* coef = (isv ? sP : sA) + l31 * LP + lk;
      const float* X = (isv ? sG : OWNK ? sQ : sK) + lk * ldx;
      f32x16 d = acc[jj];
#pragma unroll
      for (int s = 0; s < BT / 2; ++s) d = mma(coef[2 * s], ok ? X[2 * s * ldx + cc] : 0.0f, d);
      if (ABS && !isv) {                              // dq = dC K: (-b k_i, +b k_r); dk = dC^H Q: (+b q_i, -b q_r)
        const int pc = cc < E ? cc + E : cc - E;
        const float sg = !ok ? 0.0f : ((cc < E) == OWNK) ? 1.0f : -1.0f;
        const float* cb = sB + l31 * LP + lk;
#pragma unroll
        for (int s = 0; s < BT / 2; ++s) d = mma(cb[2 * s], sg * X[2 * s * ldx + pc], d);
      }
      acc[jj] = d;
    }
  }

  // ---- store: lane = column (consecutive lanes, consecutive addresses), registers = the owner's rows
  const int rows = OWNK ? g.S : g.L;
  const int64_t o1 = batch_off(g, b, OWNK ? g.bdk : g.bdq), o2 = OWNK ? batch_off(g, b, g.bdv) : 0;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wid + 4 * jj;
    if (j >= T1 + T2) break;
    const bool isv = j >= T1;
    const int c = l31 + 32 * (isv ? j - T1 : j), half = isv ? Ev : E;
    if (c >= 2 * half) continue;
    const int pl = c >= half, dcol = c - pl * half;
    void* base = isv ? (pl ? g.dv_i : g.dv_r) : OWNK ? (pl ? g.dk_i : g.dk_r) : (pl ? g.dq_i : g.dq_r);
    const int64_t rs = isv ? g.rdv : OWNK ? g.rdk : g.rdq;
    T* dst = reinterpret_cast<T*>(base) + (isv ? o2 : o1) + dcol;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = own0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (row < rows) io<T>::st(dst + (int64_t)row * rs, acc[jj][r]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static int head_bucket(int64_t E, int64_t Ev) {
  const int64_t d = E > Ev ? E : Ev;
  return d <= 32 ? 32 : d <= 64 ? 64 : 128;
}
static int fwd_lds(int dtype, int dp) {
  if (dtype == CPLXAMD_BF16) return dp == 32 ? Fwd<bf16_t, 32>::LDS : dp == 64 ? Fwd<bf16_t, 64>::LDS : Fwd<bf16_t, 128>::LDS;
  return dp == 32 ? Fwd<float, 32>::LDS : dp == 64 ? Fwd<float, 64>::LDS : Fwd<float, 128>::LDS;
}
static int bwd_lds(int64_t E, int64_t Ev) {
  return (int)((BT * 2 * (2 * E + 1 + 2 * Ev + 1) + 4 * BT * (BT + 1) + 2 * BT) * sizeof(float));
}
static bool sizes_ok(int64_t L, int64_t S, int64_t E, int64_t Ev) {
  return L >= 1 && S >= 1 && E >= 1 && Ev >= 1 && E <= 128 && Ev <= 128;
}

// validate the descriptor and bring it into kernel form
static int make_args(const cplxamd_attn_desc& d, int dtype, bool bwd, Args& g, int64_t& batch) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (!sizes_ok(d.L, d.S, d.E, d.Ev)) return CPLXAMD_EINVAL;
  if (d.flags & ~(CPLXAMD_ATTN_CAUSAL | CPLXAMD_ATTN_ABS)) return CPLXAMD_EINVAL;
  if (!std::isfinite(d.scale)) return CPLXAMD_EINVAL;
  if (d.q_rs < 0 || d.k_rs < 0 || d.v_rs < 0 || d.o_rs < d.Ev) return CPLXAMD_EINVAL;
  if (bwd && (d.dq_rs < 0 || d.dk_rs < 0 || d.dv_rs < 0)) return CPLXAMD_EINVAL;
  if (d.L > INT32_MAX - QT || d.S > INT32_MAX - 64) return CPLXAMD_ESHAPE;
  using D = cplxamd_attn_desc;
  const sp::RunStride<D> f[8] = {{&D::q_stride, g.bq},   {&D::k_stride, g.bk},   {&D::v_stride, g.bv},   {&D::o_stride, g.bo},
                                 {&D::lse_stride, g.bl}, {&D::dq_stride, g.bdq}, {&D::dk_stride, g.bdk}, {&D::dv_stride, g.bdv}};
  if (const int rc = sp::decode_runs(d, f, g.size, batch)) return rc;
  g.L = (int)d.L;
  g.S = (int)d.S;
  g.E = (int)d.E;
  g.Ev = (int)d.Ev;
  g.causal = (d.flags & CPLXAMD_ATTN_CAUSAL) != 0;
  g.scale = (float)d.scale;
  g.rq = d.q_rs;
  g.rk = d.k_rs;
  g.rv = d.v_rs;
  g.ro = d.o_rs;
  g.rdq = d.dq_rs;
  g.rdk = d.dk_rs;
  g.rdv = d.dv_rs;
  return 0;
}

static bool mult8(const int64_t (&st)[3]) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

template <typename T, int DP, bool ABS>
static int launch_fwd(const Args& g, int64_t grid, hipStream_t st) {
  static PerDeviceOnce once;
  constexpr int lds = Fwd<T, DP>::LDS;
  if (const int rc = set_max_dyn_lds(once, attn_fwd_kernel<T, DP, ABS>, lds)) return rc;
  hipLaunchKernelGGL((attn_fwd_kernel<T, DP, ABS>), dim3((uint32_t)grid), dim3(256), lds, st, g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}
template <typename T, bool ABS>
static int launch_fwd_head(const Args& g, int dp, int64_t grid, hipStream_t st) {
  if (dp == 32) return launch_fwd<T, 32, ABS>(g, grid, st);
  if (dp == 64) return launch_fwd<T, 64, ABS>(g, grid, st);
  return launch_fwd<T, 128, ABS>(g, grid, st);
}

template <typename T, bool ABS, bool OWNK>
static int launch_bwd(Args g, int64_t batch, hipStream_t st) {
  static PerDeviceOnce once;
  const int lds = bwd_lds(128, 128);
  if (const int rc = set_max_dyn_lds(once, attn_bwd_kernel<T, ABS, OWNK>, lds)) return rc;
  g.tiles = ((OWNK ? g.S : g.L) + BT - 1) / BT;
  const int64_t grid = batch * g.tiles;
  if (grid > INT32_MAX) return CPLXAMD_ESHAPE;
  hipLaunchKernelGGL((attn_bwd_kernel<T, ABS, OWNK>), dim3((uint32_t)grid), dim3(256), bwd_lds(g.E, g.Ev), st, g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}
template <typename T, bool ABS>
static int run_bwd(const Args& g, int64_t batch, hipStream_t st) {
  const int64_t total = batch * g.L;
  if ((total + 255) / 256 > INT32_MAX) return CPLXAMD_ESHAPE;
  hipLaunchKernelGGL((attn_dvec_kernel<T>), dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, g, total);
  CPLXAMD_CHECK_LAUNCH();
  if (g.dq_r)
    if (const int rc = launch_bwd<T, ABS, false>(g, batch, st)) return rc;
  return g.dk_r ? launch_bwd<T, ABS, true>(g, batch, st) : 0;
}

}  // namespace attn
}  // namespace cplxamd

using namespace cplxamd;

static_assert(sizeof(cplxamd_attn_desc) == 320, "cplxamd_attn_desc is 320 bytes");

extern "C" int cplxamd_attn_plan(int64_t L, int64_t S, int64_t E, int64_t Ev, int64_t batch, int dtype, int64_t* plan) {
  if (!plan || batch < 0 || (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) || !attn::sizes_ok(L, S, E, Ev))
    return CPLXAMD_EINVAL;
  const int dp = attn::head_bucket(E, Ev);
  const int64_t tiles = (L + attn::QT - 1) / attn::QT;
  int64_t grid, rows;
  if (__builtin_mul_overflow(tiles, batch, &grid) || grid > INT32_MAX || __builtin_mul_overflow(batch, L, &rows) ||
      rows > INT64_MAX / 4)
    return CPLXAMD_ESHAPE;
  plan[CPLXAMD_ATTN_Q_TILE] = attn::QT;
  plan[CPLXAMD_ATTN_K_TILE] = dtype == CPLXAMD_BF16 ? 64 : 32;
  plan[CPLXAMD_ATTN_HEAD] = dp;
  plan[CPLXAMD_ATTN_Q_TILES] = tiles;
  plan[CPLXAMD_ATTN_GRID] = grid;
  plan[CPLXAMD_ATTN_LDS_BYTES] = attn::fwd_lds(dtype, dp);
  plan[CPLXAMD_ATTN_WS_BYTES] = 4 * rows;
  return 0;
}

extern "C" int cplxamd_attn_fwd(const void* q_r, const void* q_i, const void* k_r, const void* k_i, const void* v_r,
                                const void* v_i, void* o_r, void* o_i, float* lse, const cplxamd_attn_desc* d, int dtype,
                                void* stream) {
  if (!q_r || !q_i || !k_r || !k_i || !v_r || !v_i || !o_r || !o_i || !lse || !d) return CPLXAMD_EINVAL;
  attn::Args g{};
  int64_t batch = 0, plan[CPLXAMD_ATTN_PLAN_FIELDS];
  if (const int rc = attn::make_args(*d, dtype, false, g, batch)) return rc;
  if (batch == 0) return 0;
  if (const int rc = cplxamd_attn_plan(d->L, d->S, d->E, d->Ev, batch, dtype, plan)) return rc;
  g.q_r = q_r; g.q_i = q_i; g.k_r = k_r; g.k_i = k_i; g.v_r = v_r; g.v_i = v_i;
  g.o_r = o_r; g.o_i = o_i; g.lse = lse;
  g.tiles = (int)plan[CPLXAMD_ATTN_Q_TILES];
  g.vecq = aligned16(q_r) && aligned16(q_i) && g.E % 8 == 0 && g.rq % 8 == 0 && attn::mult8(g.bq);
  g.veck = aligned16(k_r) && aligned16(k_i) && g.E % 8 == 0 && g.rk % 8 == 0 && attn::mult8(g.bk);
  g.vecv = aligned16(v_r) && aligned16(v_i) && g.Ev % 8 == 0 && g.rv % 8 == 0 && attn::mult8(g.bv);
  const int dp = (int)plan[CPLXAMD_ATTN_HEAD];
  const int64_t grid = plan[CPLXAMD_ATTN_GRID];
  hipStream_t st = (hipStream_t)stream;
  const bool abs_score = (d->flags & CPLXAMD_ATTN_ABS) != 0;
  if (dtype == CPLXAMD_BF16)
    return abs_score ? attn::launch_fwd_head<bf16_t, true>(g, dp, grid, st) : attn::launch_fwd_head<bf16_t, false>(g, dp, grid, st);
  return abs_score ? attn::launch_fwd_head<float, true>(g, dp, grid, st) : attn::launch_fwd_head<float, false>(g, dp, grid, st);
}

extern "C" int cplxamd_attn_bwd(const void* q_r, const void* q_i, const void* k_r, const void* k_i, const void* v_r,
                                const void* v_i, const void* o_r, const void* o_i, const void* g_r, const void* g_i,
                                const float* lse, void* dq_r, void* dq_i, void* dk_r, void* dk_i, void* dv_r, void* dv_i,
                                const cplxamd_attn_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!q_r || !q_i || !k_r || !k_i || !v_r || !v_i || !o_r || !o_i || !g_r || !g_i || !lse || !d || !ws) return CPLXAMD_EINVAL;
  // dq may be left out (both planes NULL), and so may dk with dv (all four): that kernel is not launched
  const bool want_q = dq_r != nullptr, want_kv = dk_r != nullptr;
  if ((dq_i != nullptr) != want_q || (dk_i != nullptr) != want_kv || (dv_r != nullptr) != want_kv || (dv_i != nullptr) != want_kv)
    return CPLXAMD_EINVAL;
  attn::Args g{};
  int64_t batch = 0, plan[CPLXAMD_ATTN_PLAN_FIELDS];
  if (const int rc = attn::make_args(*d, dtype, true, g, batch)) return rc;
  if (batch == 0) return 0;
  if (const int rc = cplxamd_attn_plan(d->L, d->S, d->E, d->Ev, batch, dtype, plan)) return rc;
  if (ws_bytes < plan[CPLXAMD_ATTN_WS_BYTES]) return CPLXAMD_EWS;
  g.q_r = q_r; g.q_i = q_i; g.k_r = k_r; g.k_i = k_i; g.v_r = v_r; g.v_i = v_i;
  g.o_r = const_cast<void*>(o_r); g.o_i = const_cast<void*>(o_i); g.lse = const_cast<float*>(lse);
  g.g_r = g_r; g.g_i = g_i;
  g.dq_r = dq_r; g.dq_i = dq_i; g.dk_r = dk_r; g.dk_i = dk_i; g.dv_r = dv_r; g.dv_i = dv_i;
  g.dvec = reinterpret_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  const bool abs_score = (d->flags & CPLXAMD_ATTN_ABS) != 0;
  if (dtype == CPLXAMD_BF16)
    return abs_score ? attn::run_bwd<bf16_t, true>(g, batch, st) : attn::run_bwd<bf16_t, false>(g, batch, st);
  return abs_score ? attn::run_bwd<float, true>(g, batch, st) : attn::run_bwd<float, false>(g, batch, st);
}
