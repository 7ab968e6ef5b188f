// The hand-written device primitives of the MFMA kernels (gfx950 / CDNA4 only): ONE definition of everything that
// encodes a hardware contract -- wait counters, buffer descriptors, LDS-DMA through a descriptor -- plus the vector
// types and the small host helpers those kernels share.  Include after common.h.
#pragma once
#include "common.h"

namespace cplxamd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// -v for a fragment of eight 16-bit floats (bf16 or IEEE half: the sign is bit 15 in both)
__device__ __forceinline__ bf16x8 neg_frag(bf16x8 v) {
  uint4 u = __builtin_bit_cast(uint4, v);
  u.x ^= 0x80008000u; u.y ^= 0x80008000u; u.z ^= 0x80008000u; u.w ^= 0x80008000u;
  return __builtin_bit_cast(bf16x8, u);
}

// Raw buffer descriptor over [base, base + bytes): 48-bit base, stride 0, num_records in bytes; word 3 holds the 32-bit
// data format and nothing else (no swizzle, no thread-id add-on).
__device__ __forceinline__ i32x4 make_rsrc(const void* base, uint32_t bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)base;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)bytes);
  return i32x4{(int)lo, (int)(hi & 0xffffu), (int)nb, 0x00020000};
}

// LDS-DMA through a buffer descriptor (`buffer_load_dwordx4 ... offen lds`): lane data = 16 bytes at
// base + voff (+ soff), zeros when that is outside [0, num_records) (voff wraps in 32 bits, so a "negative" row is out of
// range too: borders and rows before / after the tensor need no mask); destination M0 + lane * 16.  M0 carries the
// wave-uniform LDS byte address and is written right in front of the load (the compiler never uses M0 on gfx9+); the
// s_nop is the wait state between an SALU write of M0 and the LDS-DMA that reads it.  Inline asm for the reason given at
// common.h's lds_dma16: the kernels count these transfers themselves with wait_vmcnt<N>.
//
// One function per instruction sequence.  With a wave-uniform scalar offset in an SGPR (the caller's LDS offset is
// already scalar):
__device__ __forceinline__ void buf_lds16_soff(i32x4 rsrc, uint32_t voff, uint32_t soff_uniform, uint32_t lds_off_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
               :
               : "v"(voff), "s"(rsrc), "s"(lds_off_uniform), "s"(soff_uniform)
               : "memory");
#endif
}
// without one (soffset is the immediate 0; readfirstlane pins a loop-carried ring position to an SGPR):
__device__ __forceinline__ void buf_lds16(i32x4 rsrc, uint32_t voff, uint32_t lds_off_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t m0v = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_off_uniform);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
               :
               : "v"(voff), "s"(rsrc), "s"(m0v)
               : "memory");
#endif
}
// and the same for data that is read once: nontemporal, so that it does not push re-read rows out of the L2
__device__ __forceinline__ void buf_lds16_nt(i32x4 rsrc, uint32_t voff, uint32_t lds_off_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t m0v = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_off_uniform);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen nt lds"
               :
               : "v"(voff), "s"(rsrc), "s"(m0v)
               : "memory");
#endif
}

// ---- K-major LDS images for the hardware-transposed fragment reads of the weight-gradient kernels --------------------
// [k][64 channels] image, 128-B rows; the 64-B half is swapped on every other PAIR of k rows so that the 4 k rows one
// 16-lane group of a transposed read touches fall into distinct banks.  chunk: 16-B index 0..7
__device__ __forceinline__ int img_off(int k, int chunk) { return k * 128 + ((chunk ^ (((k >> 1) & 1) << 2)) << 4); }

// byte offset (inside an image) of this lane's transposed read for channels rb..rb+15, first pixel row kb:
// lane m of a 16-lane group addresses T[kb + (m >> 2)][rb + 4 (m & 3)] and receives T[kb .. kb+3][rb + m]
__device__ __forceinline__ uint32_t frag_base(int rb, int kb, int m) {
  const int r = rb + 4 * (m & 3), k = kb + (m >> 2);
  return (uint32_t)(img_off(k, r >> 3) + (r & 7) * 2);
}
// 8 consecutive pixels starting at the base row (+16 ks): two 4 x 16 transposes, rows +0 and +4 (the swizzle only
// looks at bit 1 of the row, so +4 and +16 are plain byte offsets)
__device__ __forceinline__ bf16x8 frag_at(const char* img, uint32_t base, int ks) {
  s16x4 v[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    v[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + base + (ks * 16 + 4 * h) * 128));
  const s16x8 both = __builtin_shufflevector(v[0], v[1], 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, both);
}

// n / d for any 32-bit n (round-up method); d == 1: s < 0
struct FastDiv { uint32_t m; int s; };

__device__ __forceinline__ uint32_t fast_div(uint32_t n, FastDiv d) {
  if (d.s < 0) return n;
  const uint32_t t = __umulhi(d.m, n);
  return (t + ((n - t) >> 1)) >> d.s;
}

inline FastDiv make_div(uint32_t d) {
  if (d <= 1) return FastDiv{0u, -1};
  int s = 0;
  while ((1ull << s) < d) ++s;                            // s = ceil(log2 d) >= 1
  const uint64_t m = (((1ull << s) - d) << 32) / d + 1;   // ceil(2^(32+s) / d) - 2^32
  return FastDiv{(uint32_t)m, s - 1};
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace cplxamd
