// Shared device helpers for the cplxamd kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cplxamd.h"

#define CPLXAMD_CHECK_LAUNCH()                          \
  do {                                                  \
    hipError_t e__ = hipGetLastError();                 \
    if (e__ != hipSuccess) return (int)e__;             \
  } while (0)

// The 16-bit matrix instruction of a translation unit.  The MFMA GEMM and channels-last convolution sources are compiled
// twice: as they are (bf16 operands) and, from gemm_f16*.hip / conv_cl*_f16.hip with CPLXAMD_GEMM_F16 / CPLXAMD_CONV_F16
// defined, for IEEE-half operands -- same staging, same LDS images (a 16-bit pattern is a 16-bit pattern; the conjugate's
// sign flip is bit 15 in both), only the matrix instruction differs.  The half variants write float32 (the fp16 split
// products of cplxmodule_amd/x3.py).
#if defined(CPLXAMD_GEMM_F16) || defined(CPLXAMD_CONV_F16)
typedef _Float16 cplxamd_f16x8 __attribute__((ext_vector_type(8)));
#define CPLXAMD_MFMA16(a, b, c) \
  __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cplxamd_f16x8, a), __builtin_bit_cast(cplxamd_f16x8, b), c, 0, 0, 0)
#else
#define CPLXAMD_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#endif

namespace cplxamd {

constexpr int kWave = 64;

// Rounds of the Philox4x32 counter-based generator behind the in-kernel noise (reparam.hip, layout.hip;
// numpy statement + Random123 known answers: oracle/philox.py).  7 is the smallest round count for which
// Philox4x32 passes BigCrush (Salmon et al., SC'11, "Parallel random numbers: as easy as 1, 2, 3", table 2);
// 10 is Random123's default safety margin.  The bf16 noise-injection kernels are bound by the generator's
// quarter-rate 32x32->64 multiplies, not by HBM, so the margin costs throughput directly
// (profiles/r02_reparam_rounds.txt).
#ifndef CPLXAMD_PHILOX_ROUNDS
#define CPLXAMD_PHILOX_ROUNDS 7
#endif
constexpr int kPhiloxRounds = CPLXAMD_PHILOX_ROUNDS;

typedef uint16_t bf16_t;  // raw bf16 bits

// floats per channel of the batch-norm backward coefficients (bn.hip bn_bwd_finalize; read by conv_cl_wgrad.hip's FOLD kernel):
// mu, mv, e00, e01, e10, e11, cuu, cuv, cvv, ku, kv, pad
constexpr int kBnBwdCoef = 12;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}

// round-to-nearest-even, NaN stays NaN (same rule as torch's float -> bfloat16): the gfx950 hardware
// conversion v_cvt_pk_bf16_f32 (one instruction per PAIR; the integer emulation it replaces was ~5 VALU ops
// per value, which showed in the VALU-bound bf16 noise-injection kernels)
typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
typedef float f32x2_hw __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  const f32x2_hw v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_hw));
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  return __builtin_bit_cast(bf16_t, (__bf16)f);
}

template <typename T> struct io;
template <> struct io<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct io<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf16_to_f32(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f32_to_bf16(v); }
};

// One LDS-DMA instruction (global_load_lds_dwordx4): every lane moves the 16 bytes at its global
// address straight into LDS at  lds_wave_base + lane * 16  (no VGPR round trip).
// Issued as inline asm ON PURPOSE: the compiler treats the builtin as an LDS store that may alias
// every later ds_read and inserts `s_waitcnt vmcnt(0)` in front of those reads, which silently
// turns a multi-stage ring into a fully synchronous copy (found in the ISA of the round-1 kernels:
// a vmcnt(0) right behind every counted wait).  With the asm form the compiler does not track the
// transfer at all; the kernels order LDS-DMA writes against reads themselves with counted
// `s_waitcnt vmcnt(N)` + `s_barrier`.  M0 carries the wave-uniform LDS byte address (the low 32
// bits of a flat LDS pointer are the LDS offset); the compiler itself never uses M0 on gfx9+.
__device__ __forceinline__ void lds_dma16(const void* gsrc, const void* lds_wave_base) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :
               : "s"(m0), "v"(gsrc)
               : "memory");
}

// Same, with the LDS destination given as a wave-uniform BYTE OFFSET that the caller built from
// scalar values (lds_offset_of() once per kernel + integer arithmetic on uniform values): the M0
// set-up then stays on the scalar unit -- a generic LDS pointer costs two VALU ops and a
// v_readfirstlane per transfer.
__device__ __forceinline__ uint32_t lds_offset_of(const void* lds_ptr) {
  return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_ptr);
}
__device__ __forceinline__ void lds_dma16_at(const void* gsrc, uint32_t lds_off_uniform) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
               :
               : "s"(lds_off_uniform), "v"(gsrc)
               : "memory");
}

// Scalar-base form: global address = sbase (wave-uniform, SGPR pair) + voff (32-bit per-lane byte
// offset).  The per-lane part of a tile piece does not depend on the K position, so it is computed
// once per kernel; advancing along K is scalar arithmetic on sbase -- no VALU work per transfer.
__device__ __forceinline__ void lds_dma16_sv(const void* sbase_uniform, uint32_t voff,
                                             uint32_t lds_off_uniform) {
  // readfirstlane pins the base to scalar registers even where the compiler's divergence analysis
  // gives up.  (The builtin returns a SIGNED int: widen through uint32_t, or the low half
  // sign-extends into the high one -- that was a GPU memory fault in the first version.)
  const uint64_t a = (uint64_t)(uintptr_t)sbase_uniform;
  const uint64_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const uint64_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  const uint64_t sb = (hi << 32) | lo;
  // (readfirstlane: a no-op for a value that already lives in an SGPR; a loop-carried ring position may not)
  const uint32_t m0v = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_off_uniform);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
               :
               : "s"(m0v), "v"(voff), "s"(sb)
               : "memory");
}

// 4-wide vector access (16 B for float, 8 B for bf16)
struct f4 { float v[4]; };
// two f4 halves = 8 elements: one 16-B access for bf16, two for float (needs 16-B alignment of p)
struct f8 { f4 h[2]; };
__device__ __forceinline__ f4 ld4(const float* p) {
  float4 t = *reinterpret_cast<const float4*>(p);
  return f4{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void st4(float* p, const f4& a) {
  *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
}
__device__ __forceinline__ f4 ld4(const bf16_t* p) {
  uint2 t = *reinterpret_cast<const uint2*>(p);
  return f4{{__uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u),
             __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u)}};
}
__device__ __forceinline__ void st4(bf16_t* p, const f4& a) {
  uint2 t;
  t.x = pack_bf16(a.v[0], a.v[1]);
  t.y = pack_bf16(a.v[2], a.v[3]);
  *reinterpret_cast<uint2*>(p) = t;
}
__device__ __forceinline__ f8 ld8(const float* p) { return f8{{ld4(p), ld4(p + 4)}}; }
__device__ __forceinline__ void st8(float* p, const f8& a) { st4(p, a.h[0]); st4(p + 4, a.h[1]); }
__device__ __forceinline__ f8 ld8(const bf16_t* p) {
  const uint4 t = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {t.x, t.y, t.z, t.w};
  f8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r.h[e >> 1].v[(e & 1) * 2] = __uint_as_float(w[e] << 16);
    r.h[e >> 1].v[(e & 1) * 2 + 1] = __uint_as_float(w[e] & 0xffff0000u);
  }
  return r;
}
__device__ __forceinline__ void st8(bf16_t* p, const f8& a) {
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    w[e] = pack_bf16(a.h[e >> 1].v[(e & 1) * 2], a.h[e >> 1].v[(e & 1) * 2 + 1]);
  *reinterpret_cast<uint4*>(p) = uint4{w[0], w[1], w[2], w[3]};
}

// ---- correctly rounded float32 primitives ---------------------------------------------------
// HIP's __fsqrt_rn is the NATIVE (1 ulp) square root and __fmul_rn / __fadd_rn are plain
// operators (clang __clang_hip_math.h); sqrtf() IS correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.  Files that need one rounding per operation also
// carry `#pragma clang fp contract(off)`.
__device__ __forceinline__ float rn_sqrt(float x) { return sqrtf(x); }

// log evaluated in fp64 and rounded once (= correctly rounded float32 log).  The empty asm
// hides the float origin of `d`, otherwise LLVM shrinks (float)log((double)x) to logf(x).
__device__ __forceinline__ float exact_logf(float x) {
  double d = (double)x;
  asm volatile("" : "+v"(d));
  return (float)log(d);
}

// ---- wave / block reductions (wave = 64 lanes) ---------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over a block of NT threads; result valid in thread 0.  `smem` holds NT/64 T's.
template <typename T, int NT>
__device__ __forceinline__ T block_sum(T v, T* smem) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) smem[wid] = v;
  __syncthreads();
  T r = T(0);
  if (threadIdx.x < NT / 64) r = smem[threadIdx.x];
  if (wid == 0) r = wave_sum(r);
  __syncthreads();
  return r;
}

// ---- the Philox4x32-R counter-based stream (DESIGN.md "noise stream" / "uniform stream"; oracle/philox.py) -----
// A value every lane read from the same address, pinned to scalar registers: the compiler cannot prove that a loaded
// stream position is wave-uniform and would otherwise run Philox's key schedule (2 adds per round) on the vector ALU --
// 14 of ~70 instructions per call in kernels that PMC shows 93 % VALU-busy (profiles/r03_reparam_pmc.txt).
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

struct u32x4 { uint32_t v[4]; };

__device__ __forceinline__ u32x4 philox4x32(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32);
  uint32_t c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
    // one 32x32->64 product each (v_mad_u64_u32) instead of a mul_lo + mul_hi pair
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32);
    const uint32_t lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
    // three-input XOR in one instruction (v_bitop3_b32, truth table 0x96)
    c0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96);
    c1 = lo1;
    c2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return u32x4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float u01(uint32_t x) {
  // ((x >> 8) + 0.5) * 2^-24 as ONE fused multiply-add: bit-identical to the add-then-multiply of the stream definition
  // (below 2^23 both are exact; from 2^23 on the sum is a tie that either form rounds to the same even neighbour)
  return fmaf((float)(x >> 8), 5.9604644775390625e-08f, 2.98023223876953125e-08f);
}

// Scale undo of the half-precision split products (split.hip, 'x2'): the operands carry powers of two sa, sb with
// exponents in [-120, 120]; scale_a / scale_b = device {s, 1 / s}.  The accumulators hold sa sb C, and sa sb itself
// leaves float32's range when both operands are tiny (max|A| max|B| <= 2^-98: sa sb = inf, 1 / (sa sb) = 0) or both huge.
// So the undo is two multiplies, acc * a1 * a2, whose intermediate stays finite and normal whenever the result does:
//   1/sa and 1/sb on the same side of 1: a1 = 1/sa, a2 = 1/sb (the intermediate lies between acc and the result);
//   on opposite sides: a1 = (1/sa)(1/sb), exact and within 2^+-120, a2 = 1.
// Either way the same bits as acc * (1/sa 1/sb) wherever that product was representable.  A bias cannot ride in scaled
// accumulators (it would start as bias * (sa sb), which is inf for tiny operands and made a zero bias NaN): the scaled
// kernels add it behind the undo, whatever the scales -- one order of operations, so that C(A 2^p, B 2^q, bias 2^(p+q))
// is C(A, B, bias) 2^(p+q) bit for bit while the exponents stay inside the clip.
struct ScaleUndo { float a1, a2; };
__device__ __forceinline__ ScaleUndo scale_undo(const float* scale_a, const float* scale_b) {
  ScaleUndo u{1.0f, 1.0f};
  if (!scale_a) return u;
  const float ia = scale_a[1], ib = scale_b[1];
  const bool mixed = (ia > 1.0f) != (ib > 1.0f);
  u.a1 = mixed ? ia * ib : ia;
  u.a2 = mixed ? 1.0f : ib;
  return u;
}

// grid for HBM-bound streaming kernels: cap at 256 CUs x 8 blocks, grid-stride the rest
inline int stream_grid(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

}  // namespace cplxamd
