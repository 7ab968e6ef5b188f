// Structured compaction of the masked layers (cplxmodule_amd/compact.py; include/cplxamd.h, last section): the live
// rows / columns of a mask as ascending index lists, and the gather / expand passes that move activations, weights and
// gradients between the full and the compacted index spaces.  Everything here is a copy or one multiply per element:
// HBM-bound, deterministic (no atomics anywhere; the lists come out of ordered prefix sums), capturable (no host
// round trip, no allocation).
#include "common.h"

#pragma clang fp contract(off)

namespace cplxamd {

// ---- live index -------------------------------------------------------------------------------------------------------
constexpr int kRowT = 256;        // threads reducing one row of the mask
constexpr int kColT = 256;        // columns per block of the column pass
constexpr int kColChunkRows = 64; // rows per chunk of the column pass ...
constexpr int kLiveChunks = 64;   // ... in at least this many chunks when there are that many rows, and
constexpr int64_t kLivePartInts = (int64_t)1 << 22;   // as many more as keep the chunk partials within 16 MiB
constexpr int kScanT = 1024;      // threads of the ordered compaction (one block per list)
constexpr int kScanItems = 4;     // consecutive indices per thread and pass

// Chunks of the column pass: one per 64 rows, at most kLiveChunksMax (the compaction ORs a column's chunk partials
// serially, so at O = 2^20 both walks are 1024 long: a thread of live_cols_kernel over its rows, a thread of the scan over
// the partials -- independent loads either way), fewer where the partials [chunks][C] would pass kLivePartInts, never
// fewer than kLiveChunks.  A mask that is long on BOTH axes therefore keeps 64 chunks and walks of O / 64 rows, but then
// has C / 256 * 64 blocks in flight and is bound by reading the mask once.  Runs on a plan rebuild only.
constexpr int kLiveChunksMax = 1024;
static inline int live_chunks(int64_t O, int64_t C) {
  int64_t c = (O + kColChunkRows - 1) / kColChunkRows;
  int64_t cap = kLivePartInts / (C < 1 ? 1 : C);
  if (cap > kLiveChunksMax) cap = kLiveChunksMax;
  if (cap < kLiveChunks) cap = kLiveChunks;
  if (c > cap) c = cap;
  return (int)(c < 1 ? 1 : c);
}

// flag[o] = any(mask[o, :, :] != 0): one block per row, the row is contiguous
__global__ __launch_bounds__(kRowT) void live_rows_kernel(const float* mask, int64_t len, int* flag) {
  const float* row = mask + (int64_t)blockIdx.x * len;
  int any = 0;
  for (int64_t i = threadIdx.x; i < len; i += kRowT) any |= (row[i] != 0.0f);
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flag[blockIdx.x] = any ? 1 : 0;
}

// part[chunk][c] = any(mask[rows of the chunk, c, :] != 0): a thread owns one column, lanes walk neighbouring columns
__global__ __launch_bounds__(kColT) void live_cols_kernel(const float* mask, int64_t O, int64_t C, int64_t T, int* part) {
  const int64_t c = (int64_t)blockIdx.x * kColT + threadIdx.x;
  if (c >= C) return;
  const int64_t per = (O + gridDim.y - 1) / gridDim.y;
  const int64_t o0 = (int64_t)blockIdx.y * per;
  int64_t o1 = o0 + per;
  if (o1 > O) o1 = O;
  int any = 0;
  for (int64_t o = o0; o < o1; ++o) {
    const float* p = mask + (o * C + c) * T;
    for (int64_t t = 0; t < T; ++t) any |= (p[t] != 0.0f);
  }
  part[(int64_t)blockIdx.y * C + c] = any ? 1 : 0;
}

// exclusive prefix sum of one int per thread over the block (kScanT threads); `total` = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* smem, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) smem[wid] = inc;
  __syncthreads();
  if (wid == 0) {
    const int w = lane < kScanT / 64 ? smem[lane] : 0;
    int winc = w;
#pragma unroll
    for (int o = 1; o < kScanT / 64; o <<= 1) {
      const int t = __shfl_up(winc, o, 64);
      if (lane >= o) winc += t;
    }
    if (lane < kScanT / 64) smem[lane] = winc - w;
    if (lane == kScanT / 64 - 1) smem[kScanT / 64] = winc;
  }
  __syncthreads();
  const int r = smem[wid] + inc - v;
  total = smem[kScanT / 64];
  __syncthreads();
  return r;
}

// Ordered compaction of one list per block (block 0: rows, block 1: columns).  Selected = live, or one of the `npad`
// lowest-numbered dead indices, npad = min(total, roundup(live, granule)) - live (0 for an empty live set): the list stays
// ascending because position(i) = live_before(i) + min(dead_before(i), npad).  The block walks the indices in passes of
// kScanT * kScanItems with a running carry, so any length is one launch.
__global__ __launch_bounds__(kScanT) void live_scan_kernel(const int* row_flag, const int* col_part, int chunks, int64_t O,
                                                           int64_t C, int granule, int* rows, int* cols, int* inv_rows,
                                                           int* inv_cols, int* counts) {
  __shared__ int smem[kScanT / 64 + 1];
  const bool is_col = blockIdx.x == 1;
  const int64_t n = is_col ? C : O;
  int* idx = is_col ? cols : rows;
  int* inv = is_col ? inv_cols : inv_rows;
  constexpr int64_t kPass = (int64_t)kScanT * kScanItems;
  auto live_at = [&](int64_t i) -> int {
    if (!is_col) return row_flag[i];
    int any = 0;
    for (int k = 0; k < chunks; ++k) any |= col_part[(int64_t)k * C + i];
    return any;
  };
  // pass A: the live count (the padding depends on it)
  int mine = 0;
  for (int64_t i = threadIdx.x; i < n; i += kScanT) mine += live_at(i);
  int nlive;
  block_excl_scan(mine, smem, nlive);
  int64_t padded = 0;
  if (nlive > 0) {
    padded = ((int64_t)nlive + granule - 1) / granule * granule;
    if (padded > n) padded = n;
  }
  const int npad = (int)(padded - nlive);
  if (threadIdx.x == 0) {
    counts[2 * blockIdx.x] = nlive;
    counts[2 * blockIdx.x + 1] = (int)padded;
  }
  // pass B: positions
  int carry = 0;                                    // live indices in front of this pass
  for (int64_t base = 0; base < n; base += kPass) {
    const int64_t i0 = base + (int64_t)threadIdx.x * kScanItems;
    int f[kScanItems], cnt = 0;
#pragma unroll
    for (int e = 0; e < kScanItems; ++e) {
      f[e] = (i0 + e < n) ? live_at(i0 + e) : 0;
      cnt += f[e];
    }
    int pass_total;
    int before = carry + block_excl_scan(cnt, smem, pass_total);
#pragma unroll
    for (int e = 0; e < kScanItems; ++e) {
      const int64_t i = i0 + e;
      if (i < n) {
        const int64_t dead_before = i - before;
        const bool sel = f[e] || dead_before < npad;
        const int pos = before + (int)(dead_before < npad ? dead_before : npad);
        inv[i] = sel ? pos : -1;
        if (sel) idx[pos] = (int)i;
        before += f[e];
      }
    }
    carry += pass_total;
  }
}

// ---- gather / expand along one axis -----------------------------------------------------------------------------------
// 16 bytes per lane where the shapes and the pointers allow it: VW = the output is written as one 16-byte store per
// kVec consecutive elements of its [axis, inner] face, VR = each of those groups is also ONE 16-byte load (inner is a
// multiple of kVec); otherwise element loads.  Both kernels only move bits (the optional fill is converted).
constexpr int kCT = 256;

template <typename T> struct vec16 {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

template <typename T>
__device__ __forceinline__ void ld16(vec16<T>& d, const T* p) {
  const uint4 t = *reinterpret_cast<const uint4*>(p);
  d = __builtin_bit_cast(vec16<T>, t);
}
template <typename T>
__device__ __forceinline__ void st16(T* p, const vec16<T>& s) {
  *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, s);
}

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return f32_to_bf16(v); }

// out[o, j, i] = src[o, idx[j], i]      src [outer, A, inner], out [outer, J, inner]
template <typename T, bool VW, bool VR>
__global__ __launch_bounds__(kCT) void gather_axis_kernel(const T* s0, const T* s1, const int* idx, T* o0, T* o1,
                                                          int64_t outer, int64_t A, int64_t J, int64_t inner) {
  constexpr int V = VW ? vec16<T>::N : 1;
  const int64_t face = J * inner, groups = face / V, total = outer * groups;
  const int64_t stride = (int64_t)gridDim.x * kCT;
  for (int64_t g = (int64_t)blockIdx.x * kCT + threadIdx.x; g < total; g += stride) {
    const int64_t o = g / groups, r = (g - o * groups) * V;
    if (VR) {
      const int64_t j = r / inner, i = r - j * inner;
      const int64_t so = (o * A + idx[j]) * inner + i;
      vec16<T> a;
      ld16(a, s0 + so);
      st16(o0 + o * face + r, a);
      if (s1) {
        ld16(a, s1 + so);
        st16(o1 + o * face + r, a);
      }
    } else {
      vec16<T> a, b;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int64_t rr = r + e;
        const int64_t j = inner == 1 ? rr : rr / inner, i = inner == 1 ? 0 : rr - j * inner;
        const int64_t so = (o * A + idx[j]) * inner + i;
        a.v[e] = s0[so];
        if (s1) b.v[e] = s1[so];
      }
      if (VW) {
        st16(o0 + o * face + r, a);
        if (s1) st16(o1 + o * face + r, b);
      } else {
        o0[o * face + r] = a.v[0];
        if (s1) o1[o * face + r] = b.v[0];
      }
    }
  }
}

// out[o, a, i] = inv[a] >= 0 ? src[o, inv[a], i] : fill[a] (0 without fill)     src [outer, J, inner], out [outer, A, inner]
template <typename T, bool VW, bool VR>
__global__ __launch_bounds__(kCT) void expand_axis_kernel(const T* s0, const T* s1, const int* inv, const float* f0,
                                                          const float* f1, T* o0, T* o1, int64_t outer, int64_t J, int64_t A,
                                                          int64_t inner) {
  constexpr int V = VW ? vec16<T>::N : 1;
  const int64_t face = A * inner, groups = face / V, total = outer * groups;
  const int64_t stride = (int64_t)gridDim.x * kCT;
  for (int64_t g = (int64_t)blockIdx.x * kCT + threadIdx.x; g < total; g += stride) {
    const int64_t o = g / groups, r = (g - o * groups) * V;
    vec16<T> a, b;
    if (VR) {
      const int64_t ax = r / inner, i = r - ax * inner;
      const int k = inv[ax];
      if (k >= 0) {
        const int64_t so = (o * J + k) * inner + i;
        ld16(a, s0 + so);
        if (s1) ld16(b, s1 + so);
      } else {
        const T va = from_f32<T>(f0 ? f0[ax] : 0.0f), vb = from_f32<T>(f1 ? f1[ax] : 0.0f);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          a.v[e] = va;
          b.v[e] = vb;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int64_t rr = r + e;
        const int64_t ax = inner == 1 ? rr : rr / inner, i = inner == 1 ? 0 : rr - ax * inner;
        const int k = inv[ax];
        if (k >= 0) {
          const int64_t so = (o * J + k) * inner + i;
          a.v[e] = s0[so];
          if (s1) b.v[e] = s1[so];
        } else {
          a.v[e] = from_f32<T>(f0 ? f0[ax] : 0.0f);
          b.v[e] = from_f32<T>(f1 ? f1[ax] : 0.0f);
        }
      }
    }
    if (VW) {
      st16(o0 + o * face + r, a);
      if (o1) st16(o1 + o * face + r, b);
    } else {
      o0[o * face + r] = a.v[0];
      if (o1) o1[o * face + r] = b.v[0];
    }
  }
}

// ---- the weight: gather on two axes with the mask, and its adjoint -------------------------------------------------------
// W'[r, c, t] = W[rows[r], cols[c], t] * mask[rows[r], cols[c], t]     (V4: 4 consecutive elements of the [c, t] face per
// thread, one vector store)
template <typename TI, typename TO, bool V4>
__global__ __launch_bounds__(kCT) void compact_weight_kernel(const TI* w0, const TI* w1, const float* mask, const int* rows,
                                                             const int* cols, TO* o0, TO* o1, int64_t C, int64_t R,
                                                             int64_t Cn, int64_t T) {
  constexpr int V = V4 ? 4 : 1;
  const int64_t face = Cn * T, groups = face / V, total = R * groups;
  const int64_t stride = (int64_t)gridDim.x * kCT;
  for (int64_t g = (int64_t)blockIdx.x * kCT + threadIdx.x; g < total; g += stride) {
    const int64_t r = g / groups, q = (g - r * groups) * V;
    const int64_t row = rows[r];
    f4 a, b;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int64_t qq = q + e;
      const int64_t c = T == 1 ? qq : qq / T, t = T == 1 ? 0 : qq - c * T;
      const int64_t so = (row * C + cols[c]) * T + t;
      const float m = mask[so];
      a.v[e] = io<TI>::ld(w0 + so) * m;
      if (w1) b.v[e] = io<TI>::ld(w1 + so) * m;
    }
    if (V4) {
      st4(o0 + r * face + q, a);
      if (w1) st4(o1 + r * face + q, b);
    } else {
      io<TO>::st(o0 + r * face + q, a.v[0]);
      if (w1) io<TO>::st(o1 + r * face + q, b.v[0]);
    }
  }
}

// dW[o, c, t] = inv_rows[o] >= 0 && inv_cols[c] >= 0 ? dW'[inv_rows[o], inv_cols[c], t] * mask[o, c, t] : 0
template <typename TI, typename TO, bool V4>
__global__ __launch_bounds__(kCT) void expand_weight_kernel(const TI* s0, const TI* s1, const float* mask, const int* inv_rows,
                                                            const int* inv_cols, TO* o0, TO* o1, int64_t O, int64_t C,
                                                            int64_t Cn, int64_t T) {
  constexpr int V = V4 ? 4 : 1;
  const int64_t face = C * T, groups = face / V, total = O * groups;
  const int64_t stride = (int64_t)gridDim.x * kCT;
  for (int64_t g = (int64_t)blockIdx.x * kCT + threadIdx.x; g < total; g += stride) {
    const int64_t o = g / groups, q = (g - o * groups) * V;
    const int ir = inv_rows[o];
    f4 a = {{0.f, 0.f, 0.f, 0.f}}, b = {{0.f, 0.f, 0.f, 0.f}};
    if (ir >= 0) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int64_t qq = q + e;
        const int64_t c = T == 1 ? qq : qq / T, t = T == 1 ? 0 : qq - c * T;
        const int ic = inv_cols[c];
        if (ic >= 0) {
          const int64_t so = ((int64_t)ir * Cn + ic) * T + t;
          const float m = mask[o * face + qq];
          a.v[e] = io<TI>::ld(s0 + so) * m;
          if (s1) b.v[e] = io<TI>::ld(s1 + so) * m;
        }
      }
    }
    if (V4) {
      st4(o0 + o * face + q, a);
      if (s1) st4(o1 + o * face + q, b);
    } else {
      io<TO>::st(o0 + o * face + q, a.v[0]);
      if (s1) io<TO>::st(o1 + o * face + q, b.v[0]);
    }
  }
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace cplxamd

using namespace cplxamd;

extern "C" {

int64_t cplxamd_live_index_ws_bytes(int64_t O, int64_t C) {
  if (O < 0 || C < 0) return 0;
  return (int64_t)sizeof(int) * (O + (int64_t)live_chunks(O, C) * C);
}

int cplxamd_live_index(const float* mask, int64_t O, int64_t C, int64_t T, int granule, int* rows, int* cols, int* inv_rows,
                       int* inv_cols, int* counts, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !rows || !cols || !inv_rows || !inv_cols || !counts || !ws || O < 1 || C < 1 || T < 1 || granule < 1)
    return CPLXAMD_EINVAL;
  if (O > (1 << 20) || C > (1 << 20) || T > (1 << 20) || granule > (1 << 20)) return CPLXAMD_ESHAPE;
  if (ws_bytes < cplxamd_live_index_ws_bytes(O, C)) return CPLXAMD_EWS;
  hipStream_t st = (hipStream_t)stream;
  int* row_flag = (int*)ws;
  int* col_part = row_flag + O;
  const int chunks = live_chunks(O, C);
  live_rows_kernel<<<(unsigned)O, kRowT, 0, st>>>(mask, C * T, row_flag);
  CPLXAMD_CHECK_LAUNCH();
  live_cols_kernel<<<dim3((unsigned)((C + kColT - 1) / kColT), chunks), kColT, 0, st>>>(mask, O, C, T, col_part);
  CPLXAMD_CHECK_LAUNCH();
  live_scan_kernel<<<2, kScanT, 0, st>>>(row_flag, col_part, chunks, O, C, granule, rows, cols, inv_rows, inv_cols, counts);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

int cplxamd_gather_axis(const void* src_r, const void* src_i, const int* idx, void* out_r, void* out_i, int64_t outer,
                        int64_t axis, int64_t n_idx, int64_t inner, int dtype, void* stream) {
  if (!src_r || !idx || !out_r || ((src_i == nullptr) != (out_i == nullptr)) || outer < 0 || axis < 0 || n_idx < 0 || inner < 0)
    return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (outer * n_idx * inner == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int V = dtype == CPLXAMD_F32 ? 4 : 8;
  const bool vw = (n_idx * inner) % V == 0 && al16(out_r) && al16(out_i);
  const bool vr = vw && inner % V == 0 && al16(src_r) && al16(src_i);
  const int grid = stream_grid(outer * n_idx * inner / (vw ? V : 1), kCT);
#define GA(T, VW, VR) \
  gather_axis_kernel<T, VW, VR><<<grid, kCT, 0, st>>>((const T*)src_r, (const T*)src_i, idx, (T*)out_r, (T*)out_i, outer, axis, n_idx, inner)
#define GA_T(T)                  \
  do {                           \
    if (vr) GA(T, true, true);   \
    else if (vw) GA(T, true, false); \
    else GA(T, false, false);    \
  } while (0)
  if (dtype == CPLXAMD_F32) GA_T(float);
  else GA_T(bf16_t);
#undef GA_T
#undef GA
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

int cplxamd_expand_axis(const void* src_r, const void* src_i, const int* inv, const float* fill_r, const float* fill_i,
                        void* out_r, void* out_i, int64_t outer, int64_t n_idx, int64_t axis, int64_t inner, int dtype,
                        void* stream) {
  if (!src_r || !inv || !out_r || ((src_i == nullptr) != (out_i == nullptr)) || outer < 0 || axis < 0 || n_idx < 0 || inner < 0)
    return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (outer * axis * inner == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int V = dtype == CPLXAMD_F32 ? 4 : 8;
  const bool vw = (axis * inner) % V == 0 && al16(out_r) && al16(out_i);
  const bool vr = vw && inner % V == 0 && al16(src_r) && al16(src_i);
  const int grid = stream_grid(outer * axis * inner / (vw ? V : 1), kCT);
#define EA(T, VW, VR)                                                                                                        \
  expand_axis_kernel<T, VW, VR><<<grid, kCT, 0, st>>>((const T*)src_r, (const T*)src_i, inv, fill_r, fill_i, (T*)out_r, (T*)out_i, \
                                                      outer, n_idx, axis, inner)
#define EA_T(T)                      \
  do {                               \
    if (vr) EA(T, true, true);       \
    else if (vw) EA(T, true, false); \
    else EA(T, false, false);        \
  } while (0)
  if (dtype == CPLXAMD_F32) EA_T(float);
  else EA_T(bf16_t);
#undef EA_T
#undef EA
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

#define CPLXAMD_DTYPE_PAIRS(X)                                                     \
  do {                                                                             \
    if (in_dtype == CPLXAMD_F32 && out_dtype == CPLXAMD_F32) X(float, float);      \
    else if (in_dtype == CPLXAMD_F32 && out_dtype == CPLXAMD_BF16) X(float, bf16_t); \
    else if (in_dtype == CPLXAMD_BF16 && out_dtype == CPLXAMD_F32) X(bf16_t, float); \
    else if (in_dtype == CPLXAMD_BF16 && out_dtype == CPLXAMD_BF16) X(bf16_t, bf16_t); \
    else return CPLXAMD_EINVAL;                                                    \
  } while (0)

int cplxamd_compact_weight(const void* w_r, const void* w_i, const float* mask, const int* rows, const int* cols, void* out_r,
                           void* out_i, int64_t O, int64_t C, int64_t T, int64_t n_rows, int64_t n_cols, int in_dtype,
                           int out_dtype, void* stream) {
  if (!w_r || !mask || !rows || !cols || !out_r || ((w_i == nullptr) != (out_i == nullptr)) || O < 0 || C < 0 || T < 0 ||
      n_rows < 0 || n_cols < 0 || n_rows > O || n_cols > C)
    return CPLXAMD_EINVAL;
  if (n_rows * n_cols * T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (n_cols * T) % 4 == 0 && al16(out_r) && al16(out_i);
  const int grid = stream_grid(n_rows * n_cols * T / (v4 ? 4 : 1), kCT);
#define CW(TI, TO)                                                                                                              \
  do {                                                                                                                          \
    if (v4)                                                                                                                     \
      compact_weight_kernel<TI, TO, true><<<grid, kCT, 0, st>>>((const TI*)w_r, (const TI*)w_i, mask, rows, cols, (TO*)out_r,   \
                                                                (TO*)out_i, C, n_rows, n_cols, T);                              \
    else                                                                                                                        \
      compact_weight_kernel<TI, TO, false><<<grid, kCT, 0, st>>>((const TI*)w_r, (const TI*)w_i, mask, rows, cols, (TO*)out_r,  \
                                                                 (TO*)out_i, C, n_rows, n_cols, T);                             \
  } while (0)
  CPLXAMD_DTYPE_PAIRS(CW);
#undef CW
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

int cplxamd_expand_weight(const void* src_r, const void* src_i, const float* mask, const int* inv_rows, const int* inv_cols,
                          void* out_r, void* out_i, int64_t O, int64_t C, int64_t T, int64_t n_rows, int64_t n_cols,
                          int in_dtype, int out_dtype, void* stream) {
  if (!src_r || !mask || !inv_rows || !inv_cols || !out_r || ((src_i == nullptr) != (out_i == nullptr)) || O < 0 || C < 0 ||
      T < 0 || n_rows < 0 || n_cols < 0 || n_rows > O || n_cols > C)
    return CPLXAMD_EINVAL;
  (void)n_rows;
  if (O * C * T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C * T) % 4 == 0 && al16(out_r) && al16(out_i);
  const int grid = stream_grid(O * C * T / (v4 ? 4 : 1), kCT);
#define EW2(TI, TO)                                                                                                              \
  do {                                                                                                                           \
    if (v4)                                                                                                                      \
      expand_weight_kernel<TI, TO, true><<<grid, kCT, 0, st>>>((const TI*)src_r, (const TI*)src_i, mask, inv_rows, inv_cols,     \
                                                               (TO*)out_r, (TO*)out_i, O, C, n_cols, T);                         \
    else                                                                                                                         \
      expand_weight_kernel<TI, TO, false><<<grid, kCT, 0, st>>>((const TI*)src_r, (const TI*)src_i, mask, inv_rows, inv_cols,    \
                                                                (TO*)out_r, (TO*)out_i, O, C, n_cols, T);                        \
  } while (0)
  CPLXAMD_DTYPE_PAIRS(EW2);
#undef EW2
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
