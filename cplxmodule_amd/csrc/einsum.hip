// Strided complex tensor contraction on the matrix cores, one launch per product:
//   C[b.., m.., n..] = sum_{k..} op(A)[b.., m.., k..] * op(B)[b.., n.., k..],   op = identity or conjugate per operand,
// planar re / im, float32 operands on v_mfma_f32_32x32x2_f32 (an fmaf chain in k order, as gemm_generic.hip) and bf16
// operands on v_mfma_f32_32x32x16_bf16 (float32 accumulation), lane maps as in gemm_generic.hip / conv_bf16.hip.
//
// Reference arithmetic: cplx.einsum cplxmodule/cplx.py:1032-1059 (re = E(ar, br) - E(ai, bi), im = E(ar, bi) + E(ai, br)).
//
// Every index group (batch, M, N, K) is a list of <= 8 (extent, strideA, strideB, strideC) modes that travels BY VALUE in
// the kernel arguments (cplxamd_einsum_desc, 912 bytes): no device table, no copy, no synchronisation.
//
// Tile: 64 NB x 64 NB outputs per 256-thread block (2 x 2 waves, NB x NB MFMA tiles x {re, im} each; NB = 2 when the
// problem has enough 128 x 128 tiles to fill the chip, else 1), BK = 16 (float32) / 32 (bf16).  The four real products
// of the complex product share one staged A tile and one staged B tile per K step; conjugation is a sign on two of them.
//
// Addressing: one thread per tile row decodes its M (N) index over the modes ONCE per tile into LDS tables of 64-bit
// offsets (A / B row offsets for the loads, C row / column offsets for the store); the K offsets of the next stage are
// decoded by BK threads while the current stage is committed (one multiply when K is a single mode, a mixed-radix
// decode otherwise).  The batch offset is block-uniform.
//
// Loads follow the data, per operand (EinsumArgs::mode_a / mode_b, chosen on the host):
//   KVEC   innermost K mode has stride 1 and base pointer, strides and extent are 16-byte compatible: 16-byte loads;
//   KFAST  k runs across lanes, scalar loads (stride-1 K that is misaligned; and the gather case: correct, slow);
//   ROWS   innermost M (N) mode has stride 1: rows run across lanes, the tile is transposed on its way into LDS
//          (bf16, ROWVEC: 16-byte loads of 8 consecutive rows where alignment allows, 2-byte loads otherwise).
// The store runs along N (column = lane of the MFMA result).  When C's unit stride is in an M mode instead, the host
// swaps the operands and the M / N groups (C^T = B A^T): the store then runs along that unit stride without a pass
// through LDS.  The choice depends on C alone, so it is the same for every layout of A and B.
//
// Single LDS stage + register prefetch: the global loads of stage s + 1 are in flight during the MFMAs of stage s.
// No scratch, no atomics, no split-K: the summation order is k ascending whatever the layout, the same inputs give the
// same bits.  Tails in M, N and K by predication.
#include <limits.h>

#include "common.h"
#include "prims.h"

namespace cplxamd {


enum { ELOAD_KFAST = CPLXAMD_EINSUM_LOAD_KFAST, ELOAD_KVEC = CPLXAMD_EINSUM_LOAD_KVEC, ELOAD_ROWS = CPLXAMD_EINSUM_LOAD_ROWS,
       ELOAD_ROWVEC = CPLXAMD_EINSUM_LOAD_ROWVEC };
constexpr int EG_B = CPLXAMD_EINSUM_BATCH, EG_M = CPLXAMD_EINSUM_M, EG_N = CPLXAMD_EINSUM_N, EG_K = CPLXAMD_EINSUM_K;
constexpr int EMAX = CPLXAMD_EINSUM_MAX_MODES;

struct EinsumArgs {
  const void *a_r, *a_i, *b_r, *b_i;
  void *c_r, *c_i;
  cplxamd_einsum_desc d;
  uint32_t B, M, N, K, tiles_m, tiles_n;   // products of the groups' extents; tiles per batch entry
  int conj_a, conj_b, mode_a, mode_b;
};
static_assert(sizeof(EinsumArgs) <= 1024, "the descriptor travels in the kernel arguments");

// linear index of group G -> element offsets (the last mode runs fastest; the outermost needs no division)
template <int G>
__device__ __forceinline__ void edecode(const cplxamd_einsum_desc& d, uint32_t idx, int64_t& oa, int64_t& ob, int64_t& oc) {
  const int n = d.nmodes[G];
#pragma unroll
  for (int i = EMAX - 1; i >= 0; --i) {
    if (i < n) {
      uint32_t r = idx;
      if (i > 0) {
        const uint32_t e = (uint32_t)d.extent[G][i], q = idx / e;
        r = idx - q * e;
        idx = q;
      }
      if (G != EG_N) oa += (int64_t)r * d.stride_a[G][i];
      if (G != EG_M) ob += (int64_t)r * d.stride_b[G][i];
      if (G != EG_K) oc += (int64_t)r * d.stride_c[G][i];
    }
  }
}

template <int BM, int BK>
struct ETables {
  int64_t row_a[BM], row_b[BM], row_cm[BM], row_cn[BM];   // per tile row / column
  int64_t k_a[2][BK], k_b[2][BK];                         // per k of a stage, double-buffered by stage parity
};

template <int BM, int BK>
__device__ __forceinline__ void etables_rows(ETables<BM, BK>& tb, const EinsumArgs& g, uint32_t m0, uint32_t n0) {
  const int t = threadIdx.x;
  int64_t oa = 0, ob = 0, oc = 0;
  if (t < BM) {
    if (m0 + t < g.M) edecode<EG_M>(g.d, m0 + t, oa, ob, oc);
    tb.row_a[t] = oa;
    tb.row_cm[t] = oc;
  } else if (t < 2 * BM) {
    const int u = t - BM;
    if (n0 + u < g.N) edecode<EG_N>(g.d, n0 + u, oa, ob, oc);
    tb.row_b[u] = ob;
    tb.row_cn[u] = oc;
  }
}

template <int BM, int BK>
__device__ __forceinline__ void etables_k(ETables<BM, BK>& tb, const EinsumArgs& g, int buf, uint32_t k0) {
  const int t = threadIdx.x;
  if (t < BK) {
    int64_t oa = 0, ob = 0, oc = 0;
    if (k0 + t < g.K) edecode<EG_K>(g.d, k0 + t, oa, ob, oc);
    tb.k_a[buf][t] = oa;
    tb.k_b[buf][t] = ob;
  }
}

struct ETile {
  uint32_t m0, n0;
  int64_t ba, bb, bc;
};
template <int BM>
__device__ __forceinline__ ETile etile(const EinsumArgs& g) {
  // tiles of one batch entry are neighbours, and within it the tiles that share an A panel
  const uint32_t bid = blockIdx.x;
  const uint32_t tn = bid % g.tiles_n, rest = bid / g.tiles_n;
  const uint32_t tm = rest % g.tiles_m, bz = rest / g.tiles_m;
  ETile tl{tm * BM, tn * BM, 0, 0, 0};
  edecode<EG_B>(g.d, bz, tl.ba, tl.bb, tl.bc);
  return tl;
}

// C/D layout of a 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <typename T, int NB, int BM, int BK>
__device__ __forceinline__ void estore(const ETables<BM, BK>& tb, const EinsumArgs& g, const ETile& tl,
                                       const f32x16 (&acc_r)[NB][NB], const f32x16 (&acc_i)[NB][NB]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 1) * 32 * NB, wn = (wid & 1) * 32 * NB, l31 = lane & 31, lk = lane >> 5;
  T* cr = reinterpret_cast<T*>(g.c_r) + tl.bc;
  T* ci = reinterpret_cast<T*>(g.c_i) + tl.bc;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int col = wn + j * 32 + l31;
    if (tl.n0 + col >= g.N) continue;
    const int64_t ocn = tb.row_cn[col];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (tl.m0 + row >= g.M) continue;
        const int64_t o = tb.row_cm[row] + ocn;
        io<T>::st(cr + o, acc_r[i][j][r]);
        io<T>::st(ci + o, acc_i[i][j][r]);
      }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// float32: operands staged k-major in LDS, [BK][BM + 1] floats per plane (every ds_read_b32 of the MFMA phase is
// conflict-free), as gemm_generic.hip
// ------------------------------------------------------------------------------------------------------------------
constexpr int EFK = 16;
template <int NB> struct EF {
  static constexpr int BM = 64 * NB, LD = BM + 1, PLANE = EFK * LD, PER = BM * EFK / 256;
};

template <int NB> struct EFRegs { float r[EF<NB>::PER], i[EF<NB>::PER]; };

template <int NB>
__device__ __forceinline__ void ef_fetch(EFRegs<NB>& o, const float* pr, const float* pi, const int64_t* row, const int64_t* kt,
                                         uint32_t row0, uint32_t rows, uint32_t k0, uint32_t K, int mode) {
  constexpr int BM = EF<NB>::BM, PER = EF<NB>::PER, KSTEP = 256 / BM;
  const int t = threadIdx.x;
  if (mode == ELOAD_KVEC) {          // a quad of lanes covers the 16 k of one row: 64 contiguous bytes
    const int c = t & 3, rb = t >> 2;
#pragma unroll
    for (int j = 0; j < PER / 4; ++j) {
      const int r = rb + 64 * j;
      float4 vr = make_float4(0.f, 0.f, 0.f, 0.f), vi = vr;
      if (row0 + r < rows && k0 + 4 * c < K) {
        const int64_t off = row[r] + kt[4 * c];
        vr = *reinterpret_cast<const float4*>(pr + off);
        vi = *reinterpret_cast<const float4*>(pi + off);
      }
      o.r[4 * j] = vr.x; o.r[4 * j + 1] = vr.y; o.r[4 * j + 2] = vr.z; o.r[4 * j + 3] = vr.w;
      o.i[4 * j] = vi.x; o.i[4 * j + 1] = vi.y; o.i[4 * j + 2] = vi.z; o.i[4 * j + 3] = vi.w;
    }
  } else if (mode == ELOAD_KFAST) {  // k fastest across lanes
    const int k = t & 15, rb = t >> 4;
    const bool kok = k0 + k < K;
    const int64_t ko = kt[k];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int r = rb + 16 * j;
      const bool ok = kok && row0 + r < rows;
      const int64_t off = row[r] + ko;
      o.r[j] = ok ? pr[off] : 0.0f;
      o.i[j] = ok ? pi[off] : 0.0f;
    }
  } else {                           // rows fastest across lanes
    const int r = t % BM, kb = t / BM;
    const bool rok = row0 + r < rows;
    const int64_t ro = row[r];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int k = kb + KSTEP * j;
      const bool ok = rok && k0 + k < K;
      const int64_t off = ro + kt[k];
      o.r[j] = ok ? pr[off] : 0.0f;
      o.i[j] = ok ? pi[off] : 0.0f;
    }
  }
}

template <int NB>
__device__ __forceinline__ void ef_commit(float* dr, float* di, const EFRegs<NB>& o, int mode) {
  constexpr int BM = EF<NB>::BM, PER = EF<NB>::PER, KSTEP = 256 / BM, LD = EF<NB>::LD;
  const int t = threadIdx.x;
  if (mode == ELOAD_KVEC) {
    const int c = t & 3, rb = t >> 2;
#pragma unroll
    for (int j = 0; j < PER / 4; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dr[(4 * c + u) * LD + rb + 64 * j] = o.r[4 * j + u];
        di[(4 * c + u) * LD + rb + 64 * j] = o.i[4 * j + u];
      }
  } else if (mode == ELOAD_KFAST) {
    const int k = t & 15, rb = t >> 4;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      dr[k * LD + rb + 16 * j] = o.r[j];
      di[k * LD + rb + 16 * j] = o.i[j];
    }
  } else {
    const int r = t % BM, kb = t / BM;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      dr[(kb + KSTEP * j) * LD + r] = o.r[j];
      di[(kb + KSTEP * j) * LD + r] = o.i[j];
    }
  }
}

template <int NB>
__global__ __launch_bounds__(256, 2) void einsum_f32_kernel(EinsumArgs g) {
  constexpr int BM = EF<NB>::BM, LD = EF<NB>::LD, PLANE = EF<NB>::PLANE;
  __shared__ float sm[4 * PLANE];            // A_r, A_i, B_r, B_i
  __shared__ ETables<BM, EFK> tb;
  float *sAr = sm, *sAi = sm + PLANE, *sBr = sm + 2 * PLANE, *sBi = sm + 3 * PLANE;

  const ETile tl = etile<BM>(g);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 1) * 32 * NB, wn = (wid & 1) * 32 * NB, l31 = lane & 31, lk = lane >> 5;
  const float sa = g.conj_a ? -1.0f : 1.0f, sb = g.conj_b ? -1.0f : 1.0f;
  const float* pa_r = reinterpret_cast<const float*>(g.a_r) + tl.ba;
  const float* pa_i = reinterpret_cast<const float*>(g.a_i) + tl.ba;
  const float* pb_r = reinterpret_cast<const float*>(g.b_r) + tl.bb;
  const float* pb_i = reinterpret_cast<const float*>(g.b_i) + tl.bb;

  f32x16 acc_r[NB][NB], acc_i[NB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      acc_r[i][j] = f32x16{0};
      acc_i[i][j] = f32x16{0};
    }

  etables_rows(tb, g, tl.m0, tl.n0);
  etables_k(tb, g, 0, 0);
  __syncthreads();
  EFRegs<NB> ra, rb;
  auto fetch = [&](uint32_t k0, int buf) {
    ef_fetch<NB>(ra, pa_r, pa_i, tb.row_a, tb.k_a[buf], tl.m0, g.M, k0, g.K, g.mode_a);
    ef_fetch<NB>(rb, pb_r, pb_i, tb.row_b, tb.k_b[buf], tl.n0, g.N, k0, g.K, g.mode_b);
  };
  if (g.K > 0) fetch(0, 0);
  int buf = 0;
  for (uint32_t k0 = 0; k0 < g.K; k0 += EFK, buf ^= 1) {
    const bool more = k0 + EFK < g.K;
    ef_commit<NB>(sAr, sAi, ra, g.mode_a);
    ef_commit<NB>(sBr, sBi, rb, g.mode_b);
    if (more) etables_k(tb, g, buf ^ 1, k0 + EFK);
    __syncthreads();                          // tile and next k offsets visible
    if (more) fetch(k0 + EFK, buf ^ 1);       // in flight during the MFMAs below
#pragma unroll
    for (int kk = 0; kk < EFK; kk += 2) {
      float ar[NB], br[NB], ai[NB], bi[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        ar[i] = sAr[(kk + lk) * LD + wm + i * 32 + l31];
        br[i] = sBr[(kk + lk) * LD + wn + i * 32 + l31];
        ai[i] = sa * sAi[(kk + lk) * LD + wm + i * 32 + l31];
        bi[i] = sb * sBi[(kk + lk) * LD + wn + i * 32 + l31];
      }
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[i], br[j], acc_r[i][j], 0, 0, 0);
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai[i], bi[j], acc_r[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[i], bi[j], acc_i[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[i], br[j], acc_i[i][j], 0, 0, 0);
        }
    }
    __syncthreads();                          // the stage is free again
  }
  estore<float, NB>(tb, g, tl, acc_r, acc_i);
}

// ------------------------------------------------------------------------------------------------------------------
// bf16: operands staged row-major in LDS, 80-byte rows (64 B of k + 16 B pad: every ds_read_b128 lane group hits 16
// distinct 16-byte slots), as conv_bf16.hip.  A thread owns NB 16-byte chunks (8 consecutive k of one row) per plane.
// ------------------------------------------------------------------------------------------------------------------
constexpr int EHK = 32, EHROW = 80;
template <int NB> struct EH {
  static constexpr int BM = 64 * NB, PLANE = BM * EHROW;
};
template <int NB> struct EHRegs { uint4 r[2], i[2]; };   // NB chunks of 8 k; ROWVEC: two k of 8 rows

__device__ __forceinline__ uint32_t epack2(bf16_t lo, bf16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }

template <int NB>
__device__ __forceinline__ void eh_fetch(EHRegs<NB>& o, const bf16_t* pr, const bf16_t* pi, const int64_t* row,
                                         const int64_t* kt, uint32_t row0, uint32_t rows, uint32_t k0, uint32_t K, int mode) {
  const int t = threadIdx.x;
  if (mode == ELOAD_ROWVEC) {   // 16 lanes (NB = 1: 8) cover the rows of one k pair: 16-byte loads of 8 consecutive rows
    constexpr int CH = 8 * NB;
    const int c = t % CH, kp = t / CH;
    o.r[0] = o.r[1] = o.i[0] = o.i[1] = make_uint4(0, 0, 0, 0);
    if (kp < 16 && row0 + 8 * c < rows) {
      const int64_t ro = row[8 * c];
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (k0 + 2 * kp + u < K) {
          const int64_t off = ro + kt[2 * kp + u];
          o.r[u] = *reinterpret_cast<const uint4*>(pr + off);
          o.i[u] = *reinterpret_cast<const uint4*>(pi + off);
        }
    }
    return;
  }
  // KVEC / KFAST: a quad of lanes covers the 32 k of one row; ROWS: a wave covers 64 rows of one chunk
  const int q = mode == ELOAD_ROWS ? t >> 6 : t & 3, rb = mode == ELOAD_ROWS ? t & 63 : t >> 2;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int r = rb + 64 * j;
    const bool rok = row0 + r < rows;
    const int64_t ro = row[r];
    uint4 vr = make_uint4(0, 0, 0, 0), vi = vr;
    if (mode == ELOAD_KVEC) {
      if (rok && k0 + 8 * q < K) {
        const int64_t off = ro + kt[8 * q];
        vr = *reinterpret_cast<const uint4*>(pr + off);
        vi = *reinterpret_cast<const uint4*>(pi + off);
      }
    } else {
      bf16_t er[8], ei[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ok = rok && k0 + 8 * q + u < K;
        const int64_t off = ro + kt[8 * q + u];
        er[u] = ok ? pr[off] : (bf16_t)0;
        ei[u] = ok ? pi[off] : (bf16_t)0;
      }
      vr = make_uint4(epack2(er[0], er[1]), epack2(er[2], er[3]), epack2(er[4], er[5]), epack2(er[6], er[7]));
      vi = make_uint4(epack2(ei[0], ei[1]), epack2(ei[2], ei[3]), epack2(ei[4], ei[5]), epack2(ei[6], ei[7]));
    }
    o.r[j] = vr;
    o.i[j] = vi;
  }
}

template <int NB>
__device__ __forceinline__ void eh_commit(char* dr, char* di, const EHRegs<NB>& o, int mode) {
  const int t = threadIdx.x;
  if (mode == ELOAD_ROWVEC) {   // transposed: element e of the two loads = (row 8 c + e; k pair kp), one 4-byte write
    constexpr int CH = 8 * NB;
    const int c = t % CH, kp = t / CH;
    if (kp < 16) {
      const uint32_t r0[4] = {o.r[0].x, o.r[0].y, o.r[0].z, o.r[0].w}, r1[4] = {o.r[1].x, o.r[1].y, o.r[1].z, o.r[1].w};
      const uint32_t i0[4] = {o.i[0].x, o.i[0].y, o.i[0].z, o.i[0].w}, i1[4] = {o.i[1].x, o.i[1].y, o.i[1].z, o.i[1].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int w = e >> 1, sh = (e & 1) * 16;
        *reinterpret_cast<uint32_t*>(dr + (8 * c + e) * EHROW + kp * 4) = ((r0[w] >> sh) & 0xffffu) | ((r1[w] >> sh) << 16);
        *reinterpret_cast<uint32_t*>(di + (8 * c + e) * EHROW + kp * 4) = ((i0[w] >> sh) & 0xffffu) | ((i1[w] >> sh) << 16);
      }
    }
    return;
  }
  const int q = mode == ELOAD_ROWS ? t >> 6 : t & 3, rb = mode == ELOAD_ROWS ? t & 63 : t >> 2;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    *reinterpret_cast<uint4*>(dr + (rb + 64 * j) * EHROW + q * 16) = o.r[j];
    *reinterpret_cast<uint4*>(di + (rb + 64 * j) * EHROW + q * 16) = o.i[j];
  }
}

__device__ __forceinline__ bf16x8 eh_frag(const char* s, int row, int kc, uint32_t flip) {
  uint4 v = *reinterpret_cast<const uint4*>(s + row * EHROW + kc * 16);
  v.x ^= flip; v.y ^= flip; v.z ^= flip; v.w ^= flip;     // flip = 0x80008000: the negated fragment
  return __builtin_bit_cast(bf16x8, v);
}

template <int NB>
__global__ __launch_bounds__(256, 2) void einsum_bf16_kernel(EinsumArgs g) {
  constexpr int BM = EH<NB>::BM, PLANE = EH<NB>::PLANE;
  __shared__ __attribute__((aligned(16))) char sm[4 * PLANE];   // A_r, A_i, B_r, B_i
  __shared__ ETables<BM, EHK> tb;
  char *sAr = sm, *sAi = sm + PLANE, *sBr = sm + 2 * PLANE, *sBi = sm + 3 * PLANE;

  const ETile tl = etile<BM>(g);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = (wid >> 1) * 32 * NB, wn = (wid & 1) * 32 * NB, l31 = lane & 31, lk = lane >> 5;
  const uint32_t fa = g.conj_a ? 0x80008000u : 0u, fb = g.conj_b ? 0x80008000u : 0u;
  const bf16_t* pa_r = reinterpret_cast<const bf16_t*>(g.a_r) + tl.ba;
  const bf16_t* pa_i = reinterpret_cast<const bf16_t*>(g.a_i) + tl.ba;
  const bf16_t* pb_r = reinterpret_cast<const bf16_t*>(g.b_r) + tl.bb;
  const bf16_t* pb_i = reinterpret_cast<const bf16_t*>(g.b_i) + tl.bb;

  f32x16 acc_r[NB][NB], acc_i[NB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      acc_r[i][j] = f32x16{0};
      acc_i[i][j] = f32x16{0};
    }

  etables_rows(tb, g, tl.m0, tl.n0);
  etables_k(tb, g, 0, 0);
  __syncthreads();
  EHRegs<NB> ra, rb;
  auto fetch = [&](uint32_t k0, int buf) {
    eh_fetch<NB>(ra, pa_r, pa_i, tb.row_a, tb.k_a[buf], tl.m0, g.M, k0, g.K, g.mode_a);
    eh_fetch<NB>(rb, pb_r, pb_i, tb.row_b, tb.k_b[buf], tl.n0, g.N, k0, g.K, g.mode_b);
  };
  if (g.K > 0) fetch(0, 0);
  int buf = 0;
  for (uint32_t k0 = 0; k0 < g.K; k0 += EHK, buf ^= 1) {
    const bool more = k0 + EHK < g.K;
    eh_commit<NB>(sAr, sAi, ra, g.mode_a);
    eh_commit<NB>(sBr, sBi, rb, g.mode_b);
    if (more) etables_k(tb, g, buf ^ 1, k0 + EHK);
    __syncthreads();
    if (more) fetch(k0 + EHK, buf ^ 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kc = ks * 2 + lk;
      bf16x8 ar[NB], ai[NB], nai[NB], br[NB], bi[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        ar[i] = eh_frag(sAr, wm + i * 32 + l31, kc, 0u);
        ai[i] = eh_frag(sAi, wm + i * 32 + l31, kc, fa);
        nai[i] = eh_frag(sAi, wm + i * 32 + l31, kc, fa ^ 0x80008000u);
        br[i] = eh_frag(sBr, wn + i * 32 + l31, kc, 0u);
        bi[i] = eh_frag(sBi, wn + i * 32 + l31, kc, fb);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[i], br[j], acc_r[i][j], 0, 0, 0);
          acc_r[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nai[i], bi[j], acc_r[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[i], bi[j], acc_i[i][j], 0, 0, 0);
          acc_i[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ai[i], br[j], acc_i[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  estore<bf16_t, NB>(tb, g, tl, acc_r, acc_i);
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static bool einsum_group_total(const cplxamd_einsum_desc& d, int grp, uint32_t* total) {
  int64_t p = 1;
  for (int i = 0; i < d.nmodes[grp]; ++i) {
    p *= d.extent[grp][i];
    if (p > INT_MAX) return false;
  }
  *total = (uint32_t)p;
  return true;
}

// how an operand's tile is loaded: `st` = its stride vectors, `rows` = its free group (M for A, N for B)
static int einsum_load_mode(const cplxamd_einsum_desc& d, const int64_t (*st)[EMAX], int rows, const void* pr, const void* pi,
                            int esize) {
  const int nk = d.nmodes[EG_K], nr = d.nmodes[rows];
  if (nk > 0 && st[EG_K][nk - 1] == 1) {
    const int vec = 16 / esize;
    bool ok = ((uintptr_t)pr % 16 == 0) && ((uintptr_t)pi % 16 == 0) && d.extent[EG_K][nk - 1] % vec == 0;
    for (int i = 0; ok && i + 1 < nk; ++i) ok = st[EG_K][i] % vec == 0;
    for (int i = 0; ok && i < nr; ++i) ok = st[rows][i] % vec == 0;
    for (int i = 0; ok && i < d.nmodes[EG_B]; ++i) ok = st[EG_B][i] % vec == 0;
    return ok ? ELOAD_KVEC : ELOAD_KFAST;
  }
  if (nr > 0 && st[rows][nr - 1] == 1) {
    if (esize != 2) return ELOAD_ROWS;
    // bf16: 16-byte loads of 8 consecutive rows when nothing can break such a group or its alignment
    bool ok = ((uintptr_t)pr % 16 == 0) && ((uintptr_t)pi % 16 == 0) && d.extent[rows][nr - 1] % 8 == 0;
    for (int i = 0; ok && i + 1 < nr; ++i) ok = st[rows][i] % 8 == 0;
    for (int i = 0; ok && i < nk; ++i) ok = st[EG_K][i] % 8 == 0;
    for (int i = 0; ok && i < d.nmodes[EG_B]; ++i) ok = st[EG_B][i] % 8 == 0;
    return ok ? ELOAD_ROWVEC : ELOAD_ROWS;
  }
  return ELOAD_KFAST;
}

// 128 x 128 tiles when they fill the chip, else 64 x 64 (a function of the extents alone)
static int einsum_tile(const EinsumArgs& g) {
  const int64_t big = (int64_t)g.B * ((g.M + 127) / 128) * ((g.N + 127) / 128);
  return (g.M > 64 || g.N > 64) && big >= 256 ? 128 : 64;
}

struct EinsumDispatch {
  int swapped, tile;
  int64_t grid;     // 0: an empty result, nothing to launch
};

// Every host-side decision of a contraction: argument checks, the M / N swap, the load mode of both operands, the tile and
// the grid.  Only the low four bits of the operand addresses are looked at; no GPU call.
static int einsum_dispatch(EinsumArgs& g, EinsumDispatch& dp, const void* a_r, const void* a_i, const void* b_r, const void* b_i,
                           const cplxamd_einsum_desc* d, int conj_a, int conj_b, int in_dtype, int out_dtype) {
  if (!d) return CPLXAMD_EINVAL;
  for (int grp = 0; grp < 4; ++grp) {
    if (d->nmodes[grp] < 0 || d->nmodes[grp] > EMAX) return CPLXAMD_EINVAL;
    for (int i = 0; i < d->nmodes[grp]; ++i) {
      if (d->extent[grp][i] < 0) return CPLXAMD_EINVAL;
      if (grp != EG_K && d->extent[grp][i] > 1 && d->stride_c[grp][i] == 0) return CPLXAMD_EINVAL;
    }
  }
  if ((in_dtype != CPLXAMD_F32 && in_dtype != CPLXAMD_BF16) || out_dtype != in_dtype) return CPLXAMD_ESHAPE;
  g.d = *d;
  if (!einsum_group_total(g.d, EG_B, &g.B) || !einsum_group_total(g.d, EG_M, &g.M) ||
      !einsum_group_total(g.d, EG_N, &g.N) || !einsum_group_total(g.d, EG_K, &g.K))
    return CPLXAMD_ESHAPE;
  g.a_r = a_r; g.a_i = a_i; g.b_r = b_r; g.b_i = b_i;
  g.conj_a = conj_a != 0; g.conj_b = conj_b != 0;
  g.mode_a = g.mode_b = ELOAD_KFAST;
  g.tiles_m = g.tiles_n = 0;
  dp.swapped = 0; dp.tile = 64; dp.grid = 0;
  if (g.B == 0 || g.M == 0 || g.N == 0) return 0;
  // the store runs along N: when C's unit stride is in an M mode, compute C^T = B A^T instead
  const int nm = g.d.nmodes[EG_M], nn = g.d.nmodes[EG_N];
  const bool n_unit = nn > 0 && g.d.stride_c[EG_N][nn - 1] == 1, m_unit = nm > 0 && g.d.stride_c[EG_M][nm - 1] == 1;
  if (m_unit && !n_unit) {
    cplxamd_einsum_desc s = g.d;
    s.nmodes[EG_M] = nn; s.nmodes[EG_N] = nm;
    for (int i = 0; i < EMAX; ++i) {
      s.extent[EG_M][i] = g.d.extent[EG_N][i]; s.extent[EG_N][i] = g.d.extent[EG_M][i];
      s.stride_c[EG_M][i] = g.d.stride_c[EG_N][i]; s.stride_c[EG_N][i] = g.d.stride_c[EG_M][i];
    }
    for (int grp = 0; grp < 4; ++grp) {
      const int src = grp == EG_M ? EG_N : grp == EG_N ? EG_M : grp;
      for (int i = 0; i < EMAX; ++i) {
        s.stride_a[grp][i] = g.d.stride_b[src][i];
        s.stride_b[grp][i] = g.d.stride_a[src][i];
      }
    }
    g.d = s;
    g.a_r = b_r; g.a_i = b_i; g.b_r = a_r; g.b_i = a_i;
    g.conj_a = conj_b != 0; g.conj_b = conj_a != 0;
    const uint32_t tmp = g.M; g.M = g.N; g.N = tmp;
    dp.swapped = 1;
  }
  const int esize = in_dtype == CPLXAMD_F32 ? 4 : 2;
  g.mode_a = einsum_load_mode(g.d, g.d.stride_a, EG_M, g.a_r, g.a_i, esize);
  g.mode_b = einsum_load_mode(g.d, g.d.stride_b, EG_N, g.b_r, g.b_i, esize);
  dp.tile = einsum_tile(g);
  g.tiles_m = (g.M + dp.tile - 1) / dp.tile;
  g.tiles_n = (g.N + dp.tile - 1) / dp.tile;
  dp.grid = (int64_t)g.B * g.tiles_m * g.tiles_n;
  if (dp.grid > INT_MAX) return CPLXAMD_ESHAPE;
  return 0;
}

static int launch_einsum(const EinsumArgs& g, const EinsumDispatch& dp, int dtype, hipStream_t st) {
  if (dtype == CPLXAMD_F32) {
    if (dp.tile == 128) einsum_f32_kernel<2><<<dim3((uint32_t)dp.grid), 256, 0, st>>>(g);
    else einsum_f32_kernel<1><<<dim3((uint32_t)dp.grid), 256, 0, st>>>(g);
  } else {
    if (dp.tile == 128) einsum_bf16_kernel<2><<<dim3((uint32_t)dp.grid), 256, 0, st>>>(g);
    else einsum_bf16_kernel<1><<<dim3((uint32_t)dp.grid), 256, 0, st>>>(g);
  }
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // namespace cplxamd

extern "C" int cplxamd_ceinsum(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* c_r, void* c_i,
                               const cplxamd_einsum_desc* d, int conj_a, int conj_b, int in_dtype, int out_dtype,
                               void* stream) {
  using namespace cplxamd;
  if (!a_r || !a_i || !b_r || !b_i || !c_r || !c_i || !d) return CPLXAMD_EINVAL;
  EinsumArgs g;
  EinsumDispatch dp;
  const int rc = einsum_dispatch(g, dp, a_r, a_i, b_r, b_i, d, conj_a, conj_b, in_dtype, out_dtype);
  if (rc != 0 || dp.grid == 0) return rc;
  g.c_r = c_r; g.c_i = c_i;
  return launch_einsum(g, dp, in_dtype, (hipStream_t)stream);
}

extern "C" int cplxamd_einsum_plan(const cplxamd_einsum_desc* d, uint64_t a_r, uint64_t a_i, uint64_t b_r, uint64_t b_i,
                                   int dtype, int64_t* plan) {
  using namespace cplxamd;
  if (!d || !plan) return CPLXAMD_EINVAL;
  EinsumArgs g;
  EinsumDispatch dp;
  const int rc = einsum_dispatch(g, dp, (const void*)(uintptr_t)a_r, (const void*)(uintptr_t)a_i, (const void*)(uintptr_t)b_r,
                                 (const void*)(uintptr_t)b_i, d, 0, 0, dtype, dtype);
  if (rc != 0) return rc;
  plan[CPLXAMD_EINSUM_PLAN_MODE_A] = g.mode_a;
  plan[CPLXAMD_EINSUM_PLAN_MODE_B] = g.mode_b;
  plan[CPLXAMD_EINSUM_PLAN_SWAPPED] = dp.swapped;
  plan[CPLXAMD_EINSUM_PLAN_TILE] = dp.tile;
  plan[CPLXAMD_EINSUM_PLAN_GRID] = dp.grid;
  return 0;
}
