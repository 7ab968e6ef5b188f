// Finishing kernels of the semi-unitary initialiser (cplxmodule/nn/init.py:90-123 cplx_trabelsi_independent_; host side:
// cplxmodule_amd/nn/init.py).  The reference takes a host SVD of a random matrix Z and keeps U V^H; here the unitary polar
// factor of Z comes from the Newton-Schulz recurrence X <- X (1.5 I - 0.5 X^H X), whose two complex GEMMs per step are the
// library's own (cplxamd_cgemm_fl in exact float32, cplxamd_gemm_f64).  What is left around them is three passes:
//   init_moments      [sum re, sum im, sum (re^2 + im^2)] of two planes   (||X||_F before the first step, std at the end)
//   init_ns_poly      P = a I + b G of the k x k Gram matrix and ||G - I||_F^2   (the step's polynomial and its residual)
//   init_scale_store  out = in * f with f derived ON THE DEVICE from a moments triple (no host round trip), optionally
//                     as the hermitian transpose, cast to the parameter's dtype
// All three are bandwidth-bound single passes (moments: 8 B per complex float32 element read; ns_poly: 16 B; scale_store:
// 8 B read + 4..16 B written) next to 16 n k^2 flop of GEMM per step.  Sums are accumulated per thread in float64, reduced
// by wave shuffles and per block, and finished by ONE block over the per-block partials in a fixed order: the grid depends
// on the size alone, so the same input gives the same bits whatever the launch timing (no atomics).
#include "common.h"

namespace cplxamd {

constexpr int kIT = 256;
constexpr int kInitMaxBlocks = 1024;
constexpr int kInitTile = 32;                 // transposing store: 32 x 32 elements per block through LDS

template <typename T> struct in_t;
template <> struct in_t<float> { static __device__ __forceinline__ double ld(const float* p) { return (double)*p; } };
template <> struct in_t<double> { static __device__ __forceinline__ double ld(const double* p) { return *p; } };

template <typename T> struct out_t;
template <> struct out_t<float> { static __device__ __forceinline__ void st(float* p, double v) { *p = (float)v; } };
template <> struct out_t<double> { static __device__ __forceinline__ void st(double* p, double v) { *p = v; } };
// float64 -> bf16 with ONE rounding: to float32 by round-to-odd (an inexact result gets its last bit set, so no tie of the
// second rounding is manufactured by the first), then to nearest even
template <> struct out_t<bf16_t> {
  static __device__ __forceinline__ void st(bf16_t* p, double v) {
    float f = (float)v;
    const double back = (double)f;
    if (back != v && back - back == 0.0) {               // inexact and finite
      uint32_t b = __float_as_uint(f);
      if (fabs(back) > fabs(v)) b -= 1;                  // rounded away from zero: one step back is the truncation
      f = __uint_as_float(b | 1u);
    }
    *p = f32_to_bf16(f);
  }
};

// 16 bytes of a plane per lane (4 float32 / 2 float64) where the base pointer allows it, single elements otherwise
template <typename T, int V> struct __attribute__((aligned(sizeof(T) * V))) vec_t { T v[V]; };

// sum of NV values per thread over the block -> partial[blockIdx.x * NV + j] (thread 0)
template <int NV>
__device__ __forceinline__ void block_partials(const double (&acc)[NV], double* partial) {
  __shared__ double red[kIT / 64];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double s = block_sum<double, kIT>(acc[j], red);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * NV + j] = s;
  }
}

// one block: out[j] = sum_b partial[b * nv + j], b in a fixed order
__global__ __launch_bounds__(kIT) void init_final_kernel(const double* partial, int m, int nv, double* out) {
  __shared__ double red[kIT / 64];
  for (int j = 0; j < nv; ++j) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < m; i += kIT) acc += partial[(int64_t)i * nv + j];
    const double s = block_sum<double, kIT>(acc, red);
    if (threadIdx.x == 0) out[j] = s;
  }
}

template <typename T, int V>
__global__ __launch_bounds__(kIT) void init_moments_kernel(const T* re, const T* im, int64_t n, double* partial) {
  const int64_t nv = n / V, stride = (int64_t)gridDim.x * kIT;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kIT + threadIdx.x; i < nv; i += stride) {
    const vec_t<T, V> a = *reinterpret_cast<const vec_t<T, V>*>(re + i * V);
    const vec_t<T, V> b = *reinterpret_cast<const vec_t<T, V>*>(im + i * V);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double x = (double)a.v[j], y = (double)b.v[j];
      acc[0] += x;
      acc[1] += y;
      acc[2] += x * x + y * y;
    }
  }
  if (blockIdx.x == 0) {                      // the last n % V elements
    const int64_t e = nv * V + threadIdx.x;
    if (threadIdx.x < V && e < n) {
      const double x = in_t<T>::ld(re + e), y = in_t<T>::ld(im + e);
      acc[0] += x;
      acc[1] += y;
      acc[2] += x * x + y * y;
    }
  }
  block_partials<3>(acc, partial);
}

// P = a I + b G (the arithmetic of T: one fma on the diagonal, one product elsewhere) and sum |G - I|^2
template <typename T>
__global__ __launch_bounds__(kIT) void init_ns_poly_kernel(const T* gr, const T* gi, T* pr, T* pi, int k, T a, T b,
                                                           double* partial) {
  const int64_t n = (int64_t)k * k, stride = (int64_t)gridDim.x * kIT;
  double acc[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * kIT + threadIdx.x; i < n; i += stride) {
    const bool diag = (i / k) == (i % k);
    const T x = gr[i], y = gi[i];
    pr[i] = diag ? fma(b, x, a) : b * x;
    pi[i] = b * y;
    const double dx = (double)x - (diag ? 1.0 : 0.0), dy = (double)y;
    acc[0] += dx * dx + dy * dy;
  }
  block_partials<1>(acc, partial);
}

// the factor of init_scale_store; false: the denominator is 0, negative or not finite
__device__ __forceinline__ bool scale_factor(int mode, double target, const double* mom, double n, double& f) {
  if (mode == CPLXAMD_INIT_SCALE_CONST) {
    f = target;
    return true;
  }
  const double m0 = mom[0], m1 = mom[1], m2 = mom[2];
  const double d2 = mode == CPLXAMD_INIT_SCALE_NORM ? m2 : m2 / n - (m0 * m0 + m1 * m1) / (n * n);
  if (!(d2 > 0.0) || !(d2 < INFINITY)) return false;       // (NaN fails both comparisons)
  f = target / sqrt(d2);
  return f == f && fabs(f) < INFINITY;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kIT) void init_scale_kernel(const TI* ir, const TI* ii, TO* or_, TO* oi, int64_t n, int mode,
                                                         double target, const double* mom, double* status) {
  double f;
  const bool ok = scale_factor(mode, target, mom, (double)n, f);
  if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = ok ? 0.0 : 1.0;
  if (!ok) return;
  const int64_t stride = (int64_t)gridDim.x * kIT;
  for (int64_t i = (int64_t)blockIdx.x * kIT + threadIdx.x; i < n; i += stride) {
    out_t<TO>::st(or_ + i, in_t<TI>::ld(ir + i) * f);
    out_t<TO>::st(oi + i, in_t<TI>::ld(ii + i) * f);
  }
}

// out[c][r] = conj(in[r][c]) * f: in is [rows, cols], out [cols, rows], both dense; a 32 x 32 tile per block goes through
// LDS so that reads and writes both run along the fastest dimension.  Block b: tile b % tiles_c along cols, b / tiles_c
// along rows.
template <typename TI, typename TO>
__global__ __launch_bounds__(kIT) void init_scale_t_kernel(const TI* ir, const TI* ii, TO* or_, TO* oi, int64_t rows,
                                                           int64_t cols, int tiles_c, int mode, double target,
                                                           const double* mom, double* status) {
  __shared__ double tr[kInitTile][kInitTile + 1], ti[kInitTile][kInitTile + 1];
  double f;
  const bool ok = scale_factor(mode, target, mom, (double)rows * (double)cols, f);
  if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = ok ? 0.0 : 1.0;
  if (!ok) return;
  const int tx = threadIdx.x % kInitTile, ty = threadIdx.x / kInitTile;      // ty in [0, 8)
  const int64_t c0 = (int64_t)(blockIdx.x % tiles_c) * kInitTile, r0 = (int64_t)(blockIdx.x / tiles_c) * kInitTile;
#pragma unroll
  for (int j = 0; j < kInitTile; j += kIT / kInitTile) {
    const int64_t r = r0 + ty + j, c = c0 + tx;
    if (r < rows && c < cols) {
      tr[ty + j][tx] = in_t<TI>::ld(ir + r * cols + c) * f;
      ti[ty + j][tx] = -(in_t<TI>::ld(ii + r * cols + c) * f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kInitTile; j += kIT / kInitTile) {
    const int64_t c = c0 + ty + j, r = r0 + tx;
    if (r < rows && c < cols) {
      out_t<TO>::st(or_ + c * rows + r, tr[tx][ty + j]);
      out_t<TO>::st(oi + c * rows + r, ti[tx][ty + j]);
    }
  }
}

// blocks of a reducing launch: the workspace holds kInitMaxBlocks partial triples, the rest is grid-stride
static int init_grid(int64_t work_items) {
  const int64_t g = (work_items + kIT - 1) / kIT;
  return (int)(g < 1 ? 1 : (g > kInitMaxBlocks ? kInitMaxBlocks : g));
}

template <typename T>
static int launch_moments(const void* re, const void* im, int64_t n, double* out, double* ws, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const bool al = ((reinterpret_cast<uintptr_t>(re) | reinterpret_cast<uintptr_t>(im)) & 15) == 0;
  const int grid = init_grid(n / (al ? V : 1));
  if (al) init_moments_kernel<T, V><<<grid, kIT, 0, st>>>((const T*)re, (const T*)im, n, ws);
  else init_moments_kernel<T, 1><<<grid, kIT, 0, st>>>((const T*)re, (const T*)im, n, ws);
  CPLXAMD_CHECK_LAUNCH();
  init_final_kernel<<<1, kIT, 0, st>>>(ws, grid, 3, out);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int launch_ns_poly(const void* gr, const void* gi, void* pr, void* pi, int k, double a, double b, double* resid2,
                          double* ws, hipStream_t st) {
  const int grid = init_grid((int64_t)k * k);
  init_ns_poly_kernel<T><<<grid, kIT, 0, st>>>((const T*)gr, (const T*)gi, (T*)pr, (T*)pi, k, (T)a, (T)b, ws);
  CPLXAMD_CHECK_LAUNCH();
  init_final_kernel<<<1, kIT, 0, st>>>(ws, grid, 1, resid2);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO>
static int launch_scale(const void* ir, const void* ii, void* or_, void* oi, int64_t rows, int64_t cols, int transpose,
                        int mode, double target, const double* mom, double* status, hipStream_t st) {
  if (transpose) {
    const int64_t gx = (cols + kInitTile - 1) / kInitTile, gy = (rows + kInitTile - 1) / kInitTile;
    if (gx * gy > 2147483647LL) return CPLXAMD_ESHAPE;
    init_scale_t_kernel<TI, TO><<<(unsigned)(gx * gy), kIT, 0, st>>>((const TI*)ir, (const TI*)ii, (TO*)or_, (TO*)oi, rows, cols,
                                                                    (int)gx, mode, target, mom, status);
  } else {
    const int64_t n = rows * cols;
    init_scale_kernel<TI, TO><<<stream_grid(n, kIT), kIT, 0, st>>>((const TI*)ir, (const TI*)ii, (TO*)or_, (TO*)oi, n, mode, target,
                                                                   mom, status);
  }
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

static bool init_plane_dtype(int dtype) { return dtype == CPLXAMD_F32 || dtype == CPLXAMD_F64; }

}  // namespace cplxamd

using namespace cplxamd;

extern "C" {

int64_t cplxamd_init_ws_bytes(void) { return (int64_t)kInitMaxBlocks * 3 * sizeof(double); }

int cplxamd_init_moments(const void* re, const void* im, int64_t n, int dtype, double* out, void* ws, void* stream) {
  if (!re || !im || !out || !ws || n <= 0 || !init_plane_dtype(dtype)) return CPLXAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F32) return launch_moments<float>(re, im, n, out, (double*)ws, st);
  return launch_moments<double>(re, im, n, out, (double*)ws, st);
}

int cplxamd_init_ns_poly(const void* g_r, const void* g_i, void* p_r, void* p_i, int k, double a, double b, int dtype,
                         double* resid2, void* ws, void* stream) {
  if (!g_r || !g_i || !p_r || !p_i || !resid2 || !ws || k <= 0 || !init_plane_dtype(dtype)) return CPLXAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F32) return launch_ns_poly<float>(g_r, g_i, p_r, p_i, k, a, b, resid2, (double*)ws, st);
  return launch_ns_poly<double>(g_r, g_i, p_r, p_i, k, a, b, resid2, (double*)ws, st);
}

int cplxamd_init_scale_store(const void* in_r, const void* in_i, void* out_r, void* out_i, int64_t rows, int64_t cols,
                             int transpose, int mode, double target, const double* moments, double* status, int in_dtype,
                             int out_dtype, void* stream) {
  if (!in_r || !in_i || !out_r || !out_i || rows <= 0 || cols <= 0 || rows > 2147483647LL || cols > 2147483647LL ||
      !init_plane_dtype(in_dtype) || mode < CPLXAMD_INIT_SCALE_NORM || mode > CPLXAMD_INIT_SCALE_CONST ||
      (mode != CPLXAMD_INIT_SCALE_CONST && !moments) || !(target == target))
    return CPLXAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define INIT_GO(TI, TO) launch_scale<TI, TO>(in_r, in_i, out_r, out_i, rows, cols, transpose, mode, target, moments, status, st)
  // the casts a parameter needs: float32 arithmetic serves float32 and bfloat16 tensors, float64 serves float64
  if (in_dtype == CPLXAMD_F32 && out_dtype == CPLXAMD_F32) return INIT_GO(float, float);
  if (in_dtype == CPLXAMD_F32 && out_dtype == CPLXAMD_BF16) return INIT_GO(float, bf16_t);
  if (in_dtype == CPLXAMD_F64 && out_dtype == CPLXAMD_F64) return INIT_GO(double, double);
  return CPLXAMD_EINVAL;
#undef INIT_GO
}

}  // extern "C"
