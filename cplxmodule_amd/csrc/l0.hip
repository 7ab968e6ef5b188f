// L0 relevance gate (LinearL0, nn/relevance/extensions/real/ell_zero.py) and the LASSO relevance mask (lasso.py).
//
// The hard-concrete gate of Louizos et al. (ICLR 2018) in the reference's -ve log-alpha parametrisation:
//   train  z = clamp((zeta - gamma) sigmoid((log u - log(1 - u) - log_alpha) / beta) + gamma, 0, 1),  u ~ U(0, 1)
//   eval   z = clamp((zeta - gamma) sigmoid(-log_alpha) + gamma, 0, 1)
// with beta, gamma, zeta = 0.66, -0.1, 1.1 (ell_zero.py:46, gate() :127-154).  The clamp passes the gradient where
// 0 <= pre-clamp value <= 1 (torch.clamp's rule).
//
// Uniform stream ("DESIGN.md: uniform stream"): element e of the reference's `u` tensor, flattened in stream order, is
//   u_e = u01(Philox4x32-R(counter = (e >> 2, offset), key = seed)[e & 3]),  u01(x) = ((x >> 8) + 0.5) 2^-24
// (common.h; numpy statement: oracle/philox.py, philox4x32 + _u01).  For every layout the layer uses, e is the flat index
// of the [rows][cols] operand the gate multiplies: the weight [O][I] (group None), the input [B][I] (u: [B, 1, I]) and
// the pre-activation [B][O] (u: [B, O, 1]).  The backward regenerates z from (seed, offset); nothing noise-shaped is kept.
//
// Entry points (include/cplxamd.h):
//   cplxamd_l0_gate_fwd   out = A (.) z (+ bias[c]) in the GEMM operand dtype; A NULL: out = z (the relevance mask),
//                         optionally thresholded (z > 0) and summed (the sparsity count).
//   cplxamd_l0_gate_bwd   dA = D (.) z and d log_alpha = D (.) A (.) dz/dlog_alpha -- elementwise, or reduced over the
//                         rows per column in a fixed order (per-workgroup partials + one ordered final pass: repeated
//                         calls are bit-identical); optionally also A (.) z again (the weight gradient's operand).
//   cplxamd_l1_mask       LASSO relevance  log(|w| + 1e-20) >= threshold  as bool, with its count.
//   cplxamd_philox_uniform  the uniform stream, materialised (tests).
// HBM traffic (group None, float32 W, bf16 operand): forward 4 + 4 + 2 B per weight; backward 4 (D) + 4 (W) + 4 (log_alpha)
// + 4 (dW) + 4 (d log_alpha) B per weight.
#include "common.h"

// one rounding per torch op, as in the reference (explicit fmaf() calls are deliberate)
#pragma clang fp contract(off)

namespace cplxamd {

constexpr int kL0Threads = 256;
constexpr float kL0Gamma = -0.1f, kL0Span = 1.2f;   // zeta - gamma = 1.1 - (-0.1) rounded to float32

// z and (dz non-NULL) dz/dlog_alpha for one element; !train: the eval gate (no u, no beta).
// The eval gate (masks: `z > 0` must come out as in the reference) spells the reference's operations with one
// rounding each.  The training gate runs once per weight or activation element per pass and is VALU-bound in that
// form (two correctly rounded divisions alone are ~30 instructions): it multiplies by 1 / beta and takes the sigmoid's
// reciprocal from v_rcp_f32 (1 ulp) -- a few ulp on z, far inside the 1e-5 parity of its tests.
constexpr float kL0InvBeta = 1.0f / 0.66f;
__device__ __forceinline__ float l0_gate(float la, float u, bool train, float* dz) {
  float s;
  if (train) {
    const float logit = logf(u) - logf(1.0f - u);
    s = __builtin_amdgcn_rcpf(1.0f + expf(-((logit - la) * kL0InvBeta)));
  } else {
    s = 1.0f / (1.0f + expf(la));
  }
  const float pre = kL0Span * s + kL0Gamma;
  if (dz) {
    const float ds = s * (1.0f - s) * kL0Span;
    *dz = (pre >= 0.0f && pre <= 1.0f) ? (train ? -ds * kL0InvBeta : -ds) : 0.0f;
  }
  return fminf(fmaxf(pre, 0.0f), 1.0f);
}

// the 8 uniforms of elements 8 v .. 8 v + 7 (two Philox calls)
__device__ __forceinline__ void uniforms8(int64_t v, uint64_t seed, uint64_t offset, float* u) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u32x4 x = philox4x32(2 * (uint64_t)v + h, offset, seed);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[4 * h + j] = u01(x.v[j]);
  }
}
__device__ __forceinline__ float uniform1(int64_t e, uint64_t seed, uint64_t offset) {
  return u01(philox4x32((uint64_t)e >> 2, offset, seed).v[e & 3]);
}

struct L0Args {
  const void* a;          // [rows][cols] operand (NULL: 1)
  const float* la;        // [rows][cols] (elementwise) or [cols] (per column)
  const float* u;         // supplied uniforms [rows][cols] (NULL: Philox)
  uint64_t seed, offset;
  const uint64_t* state;  // device {seed, offset} (NULL: the two above)
  const float* bias;      // [cols] or NULL
  void* out;
  int64_t rows;
  int cols;
  double* partial;        // per-block sums of out (NULL: none)
};

template <typename TA, typename TO, bool COLS, bool TRAIN, bool PHILOX, bool HARD, bool VEC>
__global__ __launch_bounds__(kL0Threads) void l0_fwd_kernel(L0Args p) {
  __shared__ double red[kL0Threads / 64];
  uint64_t seed = p.seed, offset = p.offset;
  if (TRAIN && PHILOX && p.state) { seed = uniform64(p.state[0]); offset = uniform64(p.state[1]); }
  const TA* a = (const TA*)p.a;
  TO* out = (TO*)p.out;
  const int64_t n = p.rows * (int64_t)p.cols;
  const int64_t stride = (int64_t)gridDim.x * kL0Threads;
  double acc = 0.0;
  if (VEC) {
    // 8 elements per thread and step (cols % 8 == 0 when COLS: the 8 share one row); the column advances by a fixed
    // step per iteration (one 64-bit division per thread, not per step)
    const int64_t v0 = (int64_t)blockIdx.x * kL0Threads + threadIdx.x;
    const int64_t dc = COLS ? (8 * stride) % p.cols : 0;
    int64_t c = COLS ? (8 * v0) % p.cols : 0;
    for (int64_t v = v0; v < (n >> 3); v += stride) {
      const int64_t e = 8 * v;
      if (!COLS) c = e;
      const f8 la = ld8(p.la + c);
      f8 av, bv, o;
      if (a) av = ld8(a + e);
      if (COLS && p.bias) bv = ld8(p.bias + c);
      float u[8];
      if (TRAIN) {
        if (PHILOX) uniforms8(v, seed, offset, u);
        else {
          const f8 t = ld8(p.u + e);
#pragma unroll
          for (int j = 0; j < 8; ++j) u[j] = t.h[j >> 2].v[j & 3];
        }
      }
      float part = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float z = l0_gate(la.h[j >> 2].v[j & 3], TRAIN ? u[j] : 0.0f, TRAIN, nullptr);
        if (HARD) z = z > 0.0f ? 1.0f : 0.0f;
        float y = a ? av.h[j >> 2].v[j & 3] * z : z;
        if (COLS && p.bias) y = y + bv.h[j >> 2].v[j & 3];
        o.h[j >> 2].v[j & 3] = y;
        part += y;
      }
      st8(out + e, o);
      acc += (double)part;
      if (COLS) {
        c += dc;
        if (c >= p.cols) c -= p.cols;
      }
    }
  } else {
    for (int64_t e = (int64_t)blockIdx.x * kL0Threads + threadIdx.x; e < n; e += stride) {
      const int64_t c = COLS ? e % p.cols : e;
      float u = 0.0f;
      if (TRAIN) u = PHILOX ? uniform1(e, seed, offset) : p.u[e];
      float z = l0_gate(p.la[c], u, TRAIN, nullptr);
      if (HARD) z = z > 0.0f ? 1.0f : 0.0f;
      float y = a ? io<TA>::ld(a + e) * z : z;
      if (COLS && p.bias) y = y + p.bias[c];
      io<TO>::st(out + e, y);
      acc += (double)y;
    }
  }
  if (p.partial) {
    const double s = block_sum<double, kL0Threads>(acc, red);
    if (threadIdx.x == 0) p.partial[blockIdx.x] = s;
  }
}

// one block: *out = sum(partial[0..m)) in a fixed order
__global__ __launch_bounds__(kL0Threads) void l0_total_kernel(const double* partial, int m, double* out) {
  __shared__ double red[kL0Threads / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < m; i += kL0Threads) acc += partial[i];
  const double s = block_sum<double, kL0Threads>(acc, red);
  if (threadIdx.x == 0) *out = s;
}

struct L0BwdArgs {
  const void* d;          // upstream gradient of A (.) z, [rows][cols]
  const void* a;          // A, [rows][cols]
  const float* la;
  const float* u;
  uint64_t seed, offset;
  const uint64_t* state;
  void* da;               // D (.) z (NULL: not wanted)
  void* az;               // A (.) z (NULL: not wanted)
  float* dla;             // elementwise: [rows][cols]; per column: unused (partials instead)
  int64_t rows;
  int cols;
  int64_t rows_per_chunk;
  float* partial;         // per column: [chunks][cols]
};

template <typename TD, typename TA, typename TDA, typename TZ, bool TRAIN, bool PHILOX>
__device__ __forceinline__ void l0_bwd_elem(const L0BwdArgs& p, int64_t e, float la, float d, float av, uint64_t seed,
                                            uint64_t offset, float u_in, float& g) {
  float dz;
  const float u = TRAIN ? (PHILOX ? uniform1(e, seed, offset) : u_in) : 0.0f;
  const float z = l0_gate(la, u, TRAIN, &dz);
  if (p.da) io<TDA>::st((TDA*)p.da + e, d * z);
  if (p.az) io<TZ>::st((TZ*)p.az + e, av * z);
  g = d * av * dz;
}

// elementwise mode: every output written once, 8 per thread and step
template <typename TD, typename TA, typename TDA, typename TZ, bool TRAIN, bool PHILOX>
__global__ __launch_bounds__(kL0Threads) void l0_bwd_elem_kernel(L0BwdArgs p) {
  uint64_t seed = p.seed, offset = p.offset;
  if (TRAIN && PHILOX && p.state) { seed = uniform64(p.state[0]); offset = uniform64(p.state[1]); }
  const int64_t n = p.rows * (int64_t)p.cols;
  const int64_t stride = (int64_t)gridDim.x * kL0Threads;
  for (int64_t v = (int64_t)blockIdx.x * kL0Threads + threadIdx.x; v < (n >> 3); v += stride) {
    const int64_t e = 8 * v;
    const f8 la = ld8(p.la + e), d = ld8((const TD*)p.d + e), av = ld8((const TA*)p.a + e);
    float u[8];
    if (TRAIN) {
      if (PHILOX) uniforms8(v, seed, offset, u);
      else {
        const f8 t = ld8(p.u + e);
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = t.h[j >> 2].v[j & 3];
      }
    }
    f8 oda, oaz, odl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float dz;
      const float z = l0_gate(la.h[j >> 2].v[j & 3], TRAIN ? u[j] : 0.0f, TRAIN, &dz);
      const float dv = d.h[j >> 2].v[j & 3], a = av.h[j >> 2].v[j & 3];
      oda.h[j >> 2].v[j & 3] = dv * z;
      oaz.h[j >> 2].v[j & 3] = a * z;
      odl.h[j >> 2].v[j & 3] = dv * a * dz;
    }
    if (p.da) st8((TDA*)p.da + e, oda);
    if (p.az) st8((TZ*)p.az + e, oaz);
    st8(p.dla + e, odl);
  }
  if (blockIdx.x == 0) {
    const int64_t e = ((n >> 3) << 3) + threadIdx.x;
    if (e < n) {
      float g;
      l0_bwd_elem<TD, TA, TDA, TZ, TRAIN, PHILOX>(p, e, p.la[e], io<TD>::ld((const TD*)p.d + e),
                                                  io<TA>::ld((const TA*)p.a + e), seed, offset,
                                                  (TRAIN && !PHILOX) ? p.u[e] : 0.0f, g);
      p.dla[e] = g;
    }
  }
}

// Per-column mode: the workgroup grid is (column strips, row chunks).  A thread owns V consecutive columns (V = 8 when
// cols % 8 == 0, else 1) and walks the rows r0 + ty, r0 + ty + TY, ... of its chunk; the TY row lanes of a workgroup are
// summed through LDS in ty order, and the chunk's sums go to partial[chunk][col].  Fixed shapes -> fixed order.
template <typename TD, typename TA, typename TDA, typename TZ, bool TRAIN, bool PHILOX, int V>
__global__ __launch_bounds__(kL0Threads) void l0_bwd_cols_kernel(L0BwdArgs p) {
  __shared__ float red[kL0Threads * V];
  uint64_t seed = p.seed, offset = p.offset;
  if (TRAIN && PHILOX && p.state) { seed = uniform64(p.state[0]); offset = uniform64(p.state[1]); }
  const int CG = (p.cols + V - 1) / V;
  const int TX = CG < kL0Threads ? CG : kL0Threads, TY = kL0Threads / TX;
  const int tx = (int)threadIdx.x % TX, ty = (int)threadIdx.x / TX;
  const int g = (int)blockIdx.x * TX + tx;
  const bool live = ty < TY && g < CG;
  const int c0 = g * V;
  const int64_t r0 = (int64_t)blockIdx.y * p.rows_per_chunk;
  const int64_t r1 = r0 + p.rows_per_chunk < p.rows ? r0 + p.rows_per_chunk : p.rows;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.0f;
  if (live) {
    float la[V];
    if (V == 8) {
      const f8 t = ld8(p.la + c0);
#pragma unroll
      for (int j = 0; j < V; ++j) la[j] = t.h[j >> 2].v[j & 3];
    } else {
      la[0] = p.la[c0];
    }
    for (int64_t r = r0 + ty; r < r1; r += TY) {
      const int64_t e = r * p.cols + c0;
      if (V == 8) {
        const f8 d = ld8((const TD*)p.d + e), av = ld8((const TA*)p.a + e);
        float u[8];
        if (TRAIN) {
          if (PHILOX) uniforms8(e >> 3, seed, offset, u);
          else {
            const f8 t = ld8(p.u + e);
#pragma unroll
            for (int j = 0; j < 8; ++j) u[j] = t.h[j >> 2].v[j & 3];
          }
        }
        f8 oda, oaz;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float dz;
          const float z = l0_gate(la[j], TRAIN ? u[j] : 0.0f, TRAIN, &dz);
          const float dv = d.h[j >> 2].v[j & 3], a = av.h[j >> 2].v[j & 3];
          oda.h[j >> 2].v[j & 3] = dv * z;
          oaz.h[j >> 2].v[j & 3] = a * z;
          acc[j] += dv * a * dz;
        }
        if (p.da) st8((TDA*)p.da + e, oda);
        if (p.az) st8((TZ*)p.az + e, oaz);
      } else {
        float gsum;
        l0_bwd_elem<TD, TA, TDA, TZ, TRAIN, PHILOX>(p, e, la[0], io<TD>::ld((const TD*)p.d + e),
                                                    io<TA>::ld((const TA*)p.a + e), seed, offset,
                                                    (TRAIN && !PHILOX) ? p.u[e] : 0.0f, gsum);
        acc[0] += gsum;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) red[threadIdx.x * V + j] = acc[j];
  __syncthreads();
  float* dst = p.partial + (int64_t)blockIdx.y * p.cols;
  for (int f = (int)threadIdx.x; f < TX * V; f += kL0Threads) {
    const int c = (int)blockIdx.x * TX * V + f;
    if (c >= p.cols) continue;
    const int l = f / V, j = f % V;
    float t = 0.0f;
    for (int y = 0; y < TY; ++y) t += red[(y * TX + l) * V + j];
    dst[c] = t;
  }
}

// dla[c] = sum over chunks of partial[chunk][c]: 16 columns per block, 64 chunk lanes (lane l sums chunks l, l + 64,
// ...), then the 64 lane sums in lane order -- a fixed order for fixed shapes
__global__ __launch_bounds__(1024) void l0_cols_final(const float* partial, int chunks, int cols, float* dla) {
  __shared__ float red[64][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = (int)blockIdx.x * 16 + tx;
  float acc = 0.0f;
  if (c < cols)
    for (int k = ty; k < chunks; k += 64) acc += partial[(int64_t)k * cols + c];
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c < cols) {
    float t = 0.0f;
    for (int l = 0; l < 64; ++l) t += red[l][tx];
    dla[c] = t;
  }
}

struct L0ColsPlan { int strips, chunks, v; int64_t rows_per_chunk; };
static bool l0_cols_plan(int64_t rows, int cols, L0ColsPlan& q) {
  if (rows <= 0 || cols <= 0) return false;
  q.v = cols % 8 == 0 ? 8 : 1;
  const int cg = (cols + q.v - 1) / q.v;
  const int tx = cg < kL0Threads ? cg : kL0Threads, ty = kL0Threads / tx;
  q.strips = (cg + tx - 1) / tx;
  // >= 16 row steps per thread, about 2048 workgroups (8 per CU), at most 1024 chunks
  int64_t chunks = rows / (16 * (int64_t)ty);
  int64_t cap = 2048 / q.strips;
  if (cap > 1024) cap = 1024;
  if (chunks > cap) chunks = cap;
  if (chunks < 1) chunks = 1;
  int64_t rpc = (rows + chunks - 1) / chunks;
  rpc = (rpc + ty - 1) / ty * ty;
  q.rows_per_chunk = rpc;
  q.chunks = (int)((rows + rpc - 1) / rpc);
  return true;
}

__global__ __launch_bounds__(kL0Threads) void l1_mask_kernel(const float* w, float threshold, uint8_t* mask,
                                                            double* partial, int64_t n) {
  __shared__ double red[kL0Threads / 64];
  const int64_t stride = (int64_t)gridDim.x * kL0Threads;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kL0Threads + threadIdx.x; e < n; e += stride) {
    // lasso.py:14  torch.ge(torch.log(abs(w) + 1e-20), threshold): one rounding per torch op, correctly rounded log
    const float m = exact_logf(fabsf(w[e]) + 1e-20f) >= threshold ? 1.0f : 0.0f;
    if (mask) mask[e] = (uint8_t)m;
    acc += (double)m;
  }
  if (partial) {
    const double s = block_sum<double, kL0Threads>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kL0Threads) void philox_uniform_kernel(float* u, uint64_t seed, uint64_t offset,
                                                                    int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kL0Threads;
  for (int64_t e = (int64_t)blockIdx.x * kL0Threads + threadIdx.x; e < n; e += stride) u[e] = uniform1(e, seed, offset);
}

constexpr int kL0MaxBlocks = 2048;    // = stream_grid's cap: the per-block partials of a total

template <typename TA, typename TO, bool COLS, bool TRAIN, bool PHILOX>
static int l0_fwd_go(const L0Args& p, bool hard, bool vec, int grid, hipStream_t st) {
#define L0F(H, VV) l0_fwd_kernel<TA, TO, COLS, TRAIN, PHILOX, H, VV><<<grid, kL0Threads, 0, st>>>(p)
  if (hard) { if (vec) L0F(true, true); else L0F(true, false); }
  else { if (vec) L0F(false, true); else L0F(false, false); }
#undef L0F
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TA, typename TO>
static int l0_fwd_dispatch(const L0Args& p, bool cols, bool train, bool hard, bool vec, int grid, hipStream_t st) {
  const bool philox = p.u == nullptr;
  if (cols) {
    if (!train) return l0_fwd_go<TA, TO, true, false, false>(p, hard, vec, grid, st);
    return philox ? l0_fwd_go<TA, TO, true, true, true>(p, hard, vec, grid, st)
                  : l0_fwd_go<TA, TO, true, true, false>(p, hard, vec, grid, st);
  }
  if (!train) return l0_fwd_go<TA, TO, false, false, false>(p, hard, vec, grid, st);
  return philox ? l0_fwd_go<TA, TO, false, true, true>(p, hard, vec, grid, st)
                : l0_fwd_go<TA, TO, false, true, false>(p, hard, vec, grid, st);
}

template <typename TD, typename TA, typename TDA, typename TZ, bool TRAIN, bool PHILOX>
static int l0_bwd_go(const L0BwdArgs& p, bool cols, const L0ColsPlan& q, float* dla, hipStream_t st) {
  if (!cols) {
    const int64_t n = p.rows * (int64_t)p.cols;
    l0_bwd_elem_kernel<TD, TA, TDA, TZ, TRAIN, PHILOX><<<stream_grid(n >> 3, kL0Threads), kL0Threads, 0, st>>>(p);
    CPLXAMD_CHECK_LAUNCH();
    return 0;
  }
  const dim3 grid((unsigned)q.strips, (unsigned)q.chunks);
  if (q.v == 8) l0_bwd_cols_kernel<TD, TA, TDA, TZ, TRAIN, PHILOX, 8><<<grid, kL0Threads, 0, st>>>(p);
  else l0_bwd_cols_kernel<TD, TA, TDA, TZ, TRAIN, PHILOX, 1><<<grid, kL0Threads, 0, st>>>(p);
  CPLXAMD_CHECK_LAUNCH();
  l0_cols_final<<<(p.cols + 15) / 16, 1024, 0, st>>>(p.partial, q.chunks, p.cols, dla);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TD, typename TA, typename TDA, typename TZ>
static int l0_bwd_dispatch(const L0BwdArgs& p, bool cols, bool train, const L0ColsPlan& q, float* dla,
                           hipStream_t st) {
  if (!train) return l0_bwd_go<TD, TA, TDA, TZ, false, false>(p, cols, q, dla, st);
  return p.u ? l0_bwd_go<TD, TA, TDA, TZ, true, false>(p, cols, q, dla, st)
             : l0_bwd_go<TD, TA, TDA, TZ, true, true>(p, cols, q, dla, st);
}

}  // namespace cplxamd

using namespace cplxamd;

static bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool dt_ok(int t) { return t == CPLXAMD_F32 || t == CPLXAMD_BF16; }

extern "C" {

int cplxamd_l0_gate_fwd(const void* a, const float* log_alpha, const float* u, uint64_t seed, uint64_t offset,
                        const uint64_t* state, const float* bias, void* out, int64_t rows, int cols, int mode,
                        int a_dtype, int out_dtype, double* total, void* ws, void* stream) {
  if (!log_alpha || !out || rows < 0 || cols < 0 || (mode & ~7)) return CPLXAMD_EINVAL;
  if ((a && !dt_ok(a_dtype)) || !dt_ok(out_dtype) || (total && !ws)) return CPLXAMD_EINVAL;
  const bool cols_mode = (mode & CPLXAMD_L0_COLS) != 0, train = (mode & CPLXAMD_L0_TRAIN) != 0,
             hard = (mode & CPLXAMD_L0_HARD) != 0;
  if (bias && !cols_mode) return CPLXAMD_EINVAL;
  const int64_t n = rows * (int64_t)cols;
  hipStream_t st = (hipStream_t)stream;
  // the 8-wide form needs 16-byte aligned operands, n % 8 == 0 and (per column) 8 columns of one row per thread
  const bool vec = n % 8 == 0 && (!cols_mode || cols % 8 == 0) && al16p(a) && al16p(log_alpha) && al16p(out) &&
                   al16p(bias) && (!train || al16p(u));
  const int grid = stream_grid(vec ? (n >> 3) : n, kL0Threads);
  L0Args p{a, log_alpha, train ? u : nullptr, seed, offset, state, bias, out, rows, cols,
           total ? (double*)ws : nullptr};
  if (n == 0) {
    if (total) {
      l0_total_kernel<<<1, kL0Threads, 0, st>>>((const double*)ws, 0, total);
      CPLXAMD_CHECK_LAUNCH();
    }
    return 0;
  }
  int rc;
  const int at = a ? a_dtype : CPLXAMD_F32;
  if (at == CPLXAMD_F32 && out_dtype == CPLXAMD_F32) rc = l0_fwd_dispatch<float, float>(p, cols_mode, train, hard, vec, grid, st);
  else if (at == CPLXAMD_F32 && out_dtype == CPLXAMD_BF16) rc = l0_fwd_dispatch<float, bf16_t>(p, cols_mode, train, hard, vec, grid, st);
  else if (at == CPLXAMD_BF16 && out_dtype == CPLXAMD_BF16) rc = l0_fwd_dispatch<bf16_t, bf16_t>(p, cols_mode, train, hard, vec, grid, st);
  else rc = l0_fwd_dispatch<bf16_t, float>(p, cols_mode, train, hard, vec, grid, st);
  if (rc) return rc;
  if (total) {
    l0_total_kernel<<<1, kL0Threads, 0, st>>>((const double*)ws, grid, total);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

int64_t cplxamd_l0_gate_bwd_ws_bytes(int64_t rows, int cols) {
  L0ColsPlan q;
  if (!l0_cols_plan(rows, cols, q)) return 0;
  return (int64_t)q.chunks * cols * (int64_t)sizeof(float);
}

int cplxamd_l0_gate_bwd(const void* d, const void* a, const float* log_alpha, const float* u, uint64_t seed,
                        uint64_t offset, const uint64_t* state, void* da, void* az, float* d_log_alpha, int64_t rows,
                        int cols, int mode, int d_dtype, int a_dtype, int da_dtype, int az_dtype, void* ws,
                        int64_t ws_bytes, void* stream) {
  if (!d || !a || !log_alpha || !d_log_alpha || rows < 0 || cols < 0 || (mode & ~3)) return CPLXAMD_EINVAL;
  if (!dt_ok(d_dtype) || !dt_ok(a_dtype) || !dt_ok(da_dtype) || !dt_ok(az_dtype)) return CPLXAMD_EINVAL;
  const bool cols_mode = (mode & CPLXAMD_L0_COLS) != 0, train = (mode & CPLXAMD_L0_TRAIN) != 0;
  const int64_t n = rows * (int64_t)cols;
  if (n == 0) {
    // no rows to sum: the per-column gradient is 0, not whatever the caller's buffer held (a memset node when captured)
    if (cols_mode && cols > 0) return (int)hipMemsetAsync(d_log_alpha, 0, (size_t)cols * sizeof(float), (hipStream_t)stream);
    return 0;
  }
  if (!al16p(d) || !al16p(a) || !al16p(log_alpha) || !al16p(da) || !al16p(az) || !al16p(d_log_alpha) ||
      (train && !al16p(u)) || !al16p(ws))
    return CPLXAMD_EALIGN;
  L0ColsPlan q{};
  if (cols_mode) {
    if (!l0_cols_plan(rows, cols, q)) return CPLXAMD_ESHAPE;
    if (!ws || ws_bytes < cplxamd_l0_gate_bwd_ws_bytes(rows, cols)) return CPLXAMD_EWS;
  }
  L0BwdArgs p{d, a, log_alpha, train ? u : nullptr, seed, offset, state, da, az, d_log_alpha, rows, cols,
              q.rows_per_chunk, (float*)ws};
  hipStream_t st = (hipStream_t)stream;
  // the combinations the layers use (an output not asked for takes the dtype of its sibling, else of A):
  //   all float32; float32 D with bf16 A, dA, A (.) z (input group); bf16 D, dA with float32 A (output group); all bf16
  if (!da) da_dtype = az ? az_dtype : a_dtype;
  if (!az) az_dtype = da_dtype;
#define L0B(TD, TA, TDA, TZ) return l0_bwd_dispatch<TD, TA, TDA, TZ>(p, cols_mode, train, q, d_log_alpha, st)
  const int key = d_dtype | (a_dtype << 1) | (da_dtype << 2) | (az_dtype << 3);
  switch (key) {
    case 0: L0B(float, float, float, float);
    case 2 | 4 | 8: L0B(float, bf16_t, bf16_t, bf16_t);
    case 1 | 4 | 8: L0B(bf16_t, float, bf16_t, bf16_t);
    case 1 | 2 | 4 | 8: L0B(bf16_t, bf16_t, bf16_t, bf16_t);
    default: return CPLXAMD_EINVAL;
  }
#undef L0B
}

int cplxamd_l1_mask(const float* w, float threshold, uint8_t* mask, double* count, void* ws, int64_t n, void* stream) {
  if (!w || n < 0 || (!mask && !count) || (count && !ws)) return CPLXAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int grid = stream_grid(n, kL0Threads);
  if (n > 0) {
    l1_mask_kernel<<<grid, kL0Threads, 0, st>>>(w, threshold, mask, count ? (double*)ws : nullptr, n);
    CPLXAMD_CHECK_LAUNCH();
  }
  if (count) {
    l0_total_kernel<<<1, kL0Threads, 0, st>>>((const double*)ws, n > 0 ? grid : 0, count);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

int cplxamd_philox_uniform(float* u, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  if (!u || n < 0) return CPLXAMD_EINVAL;
  if (n == 0) return 0;
  philox_uniform_kernel<<<stream_grid(n, kL0Threads), kL0Threads, 0, (hipStream_t)stream>>>(u, seed, offset, n);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
