// The complex elementary functions of cplxmodule/cplx.py:482-541 (exp, log, sin, cos, tan, sinh, cosh, tanh) and their
// backward, one elementwise launch each way.  The reference spells each as a chain of real torch ops (tan: ~10 kernels
// forward, each an HBM round trip over planes as large as the activations); here one pass reads z (and g) and writes
// the result.  Traffic per complex element (fp32): forward 16 B, backward 24 B; bf16 half of that.
//
// Numerics: float32 arithmetic for both dtypes (bf16 is widened on load and rounded once on store), full-precision
// device math (sincosf / expf / expm1f / tanf / atan2f / log1pf, not the __expf-style intrinsics), and forms that
// neither cancel nor overflow where the true value is representable -- per PART: e^x cos y is finite for x well past
// 88.72 (where e^x overflows) when y is near an odd multiple of pi / 2, so past 88 the exponential enters as two
// factors e^{x/2} with the trigonometric factor multiplied in between them:
//   exp   e^x (cos y, sin y);  x > 88: (e^{x/2} cos y) e^{x/2}, (e^{x/2} sin y) e^{x/2}
//   log   (log|z|, atan2(y, x)), log|z| = log a + log1p((b / a)^2) / 2 with a = max(|x|, |y|), b = min: no overflow or
//         underflow anywhere in the float32 range; log 0 = -inf + i atan2(y, x)
//   sin   (sin x cosh y,  cos x sinh y)      cos  (cos x cosh y, -sin x sinh y)
//   sinh  (sinh x cos y,  cosh x sin y)      cosh (cosh x cos y,  sinh x sin y)
//         cosh / sinh of a real argument from ONE expm1f (e = 1 + expm1 t), so sinh stays accurate for |t| < 1;
//         |t| > 88: cosh t p = sinh |t| p = ((e^{|t|/2} / 2) p) e^{|t|/2} for the trigonometric factor p
//   tanh  Kahan: t = tan y, s = sinh x, beta = 1 + t^2, rho = sqrt(1 + s^2):  (beta rho s + i t) / (1 + beta s^2);
//         for |x| > kSat (tanh x rounds to +-1): (sign x, 4 sin y cos y e^{-2|x|})
//   tan   -i tanh(iz)
// Backward dz = conj(f'(z)) g with f' recomputed from the saved input: exp z, 1/z, cos z, -sin z, cosh z, sinh z,
// sec^2 z, sech^2 z; sech^2 z = (conj(cosh z) / |cosh z|^2)^2 with |cosh z|^2 = sinh^2 x + cos^2 y, and past kSat
// 4 e^{-2|x|} e^{-2 i sign(x) y} -- never 1 - tanh^2, which cancels where |f'| ~ 4 e^{-2|x|}.
#include "common.h"

// One rounding per written operation.  Left to contract a * b + c * d into a fused multiply-add, the compiler fuses the
// unrolled vector body and the scalar tail of the kernel differently, and a value then depends (in its last bit) on where
// in the tensor it stands; the accuracy statements above are for the unfused forms.
#pragma clang fp contract(off)

namespace cplxamd {

constexpr int kFT = 256;
// |x| past which tanh x rounds to +-1 in float32 (1 - tanh 11 = 5.5e-10 < 2^-25) and e^{-2|x|} is negligible next to 1
constexpr float kSat = 11.0f;

struct CF { float re, im; };

// (cosh t, sinh t) from one exponential
__device__ __forceinline__ void chsh(float t, float& c, float& s) {
  const float a = fabsf(t);
  if (a <= 88.0f) {
    const float em = expm1f(a), e = em + 1.0f;
    c = 0.5f * e + 0.5f / e;
    s = 0.5f * (em + em / e);
  } else {            // e^a overflows before cosh a does: (e^{a/2} / 2) e^{a/2}; NaN lands here too
    const float h = expf(0.5f * a);
    c = s = (0.5f * h) * h;
  }
  s = copysignf(s, t);
}

// (cosh t * p, sinh t * q): chsh followed by the two products for |t| <= 88 (the same bits); past it the factor goes in
// before the second e^{|t|/2}, so a product that is representable is finite although cosh t alone is not
__device__ __forceinline__ void chsh_mul(float t, float p, float q, float& cp, float& sq) {
  const float a = fabsf(t);
  if (a <= 88.0f) {
    float c, s;
    chsh(t, c, s);
    cp = c * p;
    sq = s * q;
  } else {            // NaN lands here too
    const float h = expf(0.5f * a), hh = 0.5f * h;
    cp = (hh * p) * h;
    sq = (copysignf(hh, t) * q) * h;
  }
}

__device__ __forceinline__ CF f_exp(float x, float y) {
  float s, c;
  sincosf(y, &s, &c);
  if (x > 88.0f) {    // e^x overflows at 88.72, e^x cos y need not
    const float h = expf(0.5f * x);
    return {(h * c) * h, (h * s) * h};
  }
  const float e = expf(x);
  return {e * c, e * s};
}

__device__ __forceinline__ CF f_log(float x, float y) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float a = fmaxf(ax, ay), b = fminf(ax, ay);
  float re;
  if (x != x || y != y) re = x + y;                      // NaN (fmax / fmin would drop it)
  else if (a == INFINITY) re = INFINITY;
  else if (a == 0.0f) re = -INFINITY;
  else {
    const float r = b / a;
    re = logf(a) + 0.5f * log1pf(r * r);
  }
  return {re, atan2f(y, x)};
}

__device__ __forceinline__ CF f_sin(float x, float y) {
  float sx, cx, ch, sh;
  sincosf(x, &sx, &cx);
  chsh_mul(y, sx, cx, ch, sh);
  return {ch, sh};
}

__device__ __forceinline__ CF f_cos(float x, float y) {
  float sx, cx, ch, sh;
  sincosf(x, &sx, &cx);
  chsh_mul(y, cx, sx, ch, sh);
  return {ch, -sh};
}

__device__ __forceinline__ CF f_sinh(float x, float y) {
  float sy, cy, ch, sh;
  sincosf(y, &sy, &cy);
  chsh_mul(x, sy, cy, ch, sh);
  return {sh, ch};
}

__device__ __forceinline__ CF f_cosh(float x, float y) {
  float sy, cy, ch, sh;
  sincosf(y, &sy, &cy);
  chsh_mul(x, cy, sy, ch, sh);
  return {ch, sh};
}

__device__ __forceinline__ CF f_tanh(float x, float y) {
  if (fabsf(x) > kSat) {
    float sy, cy;
    sincosf(y, &sy, &cy);
    return {copysignf(1.0f, x), 4.0f * sy * cy * expf(-2.0f * fabsf(x))};
  }
  float ch, s;
  chsh(x, ch, s);
  const float t = tanf(y);
  const float beta = 1.0f + t * t, rho = sqrtf(1.0f + s * s);
  const float den = 1.0f + beta * s * s;
  return {beta * rho * s / den, t / den};
}

__device__ __forceinline__ CF f_tan(float x, float y) {
  const CF w = f_tanh(-y, x);                            // tan z = -i tanh(iz), iz = -y + ix
  return {w.im, -w.re};
}

// sech^2 z
__device__ __forceinline__ CF sech2(float x, float y) {
  float sy, cy;
  sincosf(y, &sy, &cy);
  if (fabsf(x) > kSat) {                                 // cosh z = e^{|x|} e^{i sign(x) y} / 2 (1 + O(e^{-2|x|}))
    const float m = 4.0f * expf(-2.0f * fabsf(x)), sg = copysignf(1.0f, x);
    const float c2 = (cy - sy) * (cy + sy), s2 = 2.0f * sy * cy;
    return {m * c2, -sg * m * s2};
  }
  float ch, sh;
  chsh(x, ch, sh);
  const float d = sh * sh + cy * cy;                     // |cosh z|^2
  const float wr = ch * cy / d, wi = -(sh * sy) / d;     // 1 / cosh z
  return {(wr - wi) * (wr + wi), 2.0f * wr * wi};
}

template <int FN>
__device__ __forceinline__ CF fn_fwd(float x, float y) {
  if constexpr (FN == CPLXAMD_FN_EXP) return f_exp(x, y);
  if constexpr (FN == CPLXAMD_FN_LOG) return f_log(x, y);
  if constexpr (FN == CPLXAMD_FN_SIN) return f_sin(x, y);
  if constexpr (FN == CPLXAMD_FN_COS) return f_cos(x, y);
  if constexpr (FN == CPLXAMD_FN_TAN) return f_tan(x, y);
  if constexpr (FN == CPLXAMD_FN_SINH) return f_sinh(x, y);
  if constexpr (FN == CPLXAMD_FN_COSH) return f_cosh(x, y);
  return f_tanh(x, y);
}

// f'(z)
template <int FN>
__device__ __forceinline__ CF fn_deriv(float x, float y) {
  if constexpr (FN == CPLXAMD_FN_EXP) return f_exp(x, y);
  if constexpr (FN == CPLXAMD_FN_LOG) {                  // 1 / z = conj(z) / |z|^2, scaled by a power of two first
    const float a = fmaxf(fabsf(x), fabsf(y));
    const int k = (a > 0.0f && a < INFINITY) ? -ilogbf(a) : 0;
    const float xs = ldexpf(x, k), ys = ldexpf(y, k);
    const float d = xs * xs + ys * ys;
    return {ldexpf(xs / d, k), ldexpf(-ys / d, k)};
  }
  if constexpr (FN == CPLXAMD_FN_SIN) return f_cos(x, y);
  if constexpr (FN == CPLXAMD_FN_COS) { const CF s = f_sin(x, y); return {-s.re, -s.im}; }
  if constexpr (FN == CPLXAMD_FN_TAN) return sech2(-y, x);  // sec^2 z = sech^2(iz)
  if constexpr (FN == CPLXAMD_FN_SINH) return f_cosh(x, y);
  if constexpr (FN == CPLXAMD_FN_COSH) return f_sinh(x, y);
  return sech2(x, y);
}

// conj(f'(z)) g
template <int FN>
__device__ __forceinline__ CF fn_bwd(float x, float y, float gr, float gi) {
  const CF d = fn_deriv<FN>(x, y);
  return {d.re * gr + d.im * gi, d.re * gi - d.im * gr};
}

// one 16-byte access: 4 float32 or 8 bf16 values
template <typename T> struct v16 { static constexpr int N = 16 / sizeof(T); float v[N]; };
__device__ __forceinline__ v16<float> ldv(const float* p) { const f4 a = ld4(p); return {{a.v[0], a.v[1], a.v[2], a.v[3]}}; }
__device__ __forceinline__ void stv(float* p, const v16<float>& a) { st4(p, f4{{a.v[0], a.v[1], a.v[2], a.v[3]}}); }
__device__ __forceinline__ v16<bf16_t> ldv(const bf16_t* p) {
  const f8 a = ld8(p);
  return {{a.h[0].v[0], a.h[0].v[1], a.h[0].v[2], a.h[0].v[3], a.h[1].v[0], a.h[1].v[1], a.h[1].v[2], a.h[1].v[3]}};
}
__device__ __forceinline__ void stv(bf16_t* p, const v16<bf16_t>& a) {
  st8(p, f8{{f4{{a.v[0], a.v[1], a.v[2], a.v[3]}}, f4{{a.v[4], a.v[5], a.v[6], a.v[7]}}}});
}

// forward (BWD false: g unused) or backward; grid-stride over 16-byte vectors, the last n % V elements in block 0
template <typename T, int FN, bool BWD>
__global__ __launch_bounds__(kFT) void cplx_fn_kernel(const T* zr, const T* zi, const T* gr, const T* gi, T* or_, T* oi,
                                                      int64_t n) {
  constexpr int V = v16<T>::N;
  const int64_t nv = n / V, stride = (int64_t)gridDim.x * kFT;
  for (int64_t i = (int64_t)blockIdx.x * kFT + threadIdx.x; i < nv; i += stride) {
    const int64_t o = i * V;
    const v16<T> a = ldv(zr + o), b = ldv(zi + o);
    v16<T> u, w, x, y;
    if (BWD) { u = ldv(gr + o); w = ldv(gi + o); }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const CF r = BWD ? fn_bwd<FN>(a.v[j], b.v[j], u.v[j], w.v[j]) : fn_fwd<FN>(a.v[j], b.v[j]);
      x.v[j] = r.re;
      y.v[j] = r.im;
    }
    stv(or_ + o, x);
    stv(oi + o, y);
  }
  if (blockIdx.x == 0) {
    const int64_t e = nv * V + threadIdx.x;
    if (threadIdx.x < V && e < n) {
      const float a = io<T>::ld(zr + e), b = io<T>::ld(zi + e);
      const CF r = BWD ? fn_bwd<FN>(a, b, io<T>::ld(gr + e), io<T>::ld(gi + e)) : fn_fwd<FN>(a, b);
      io<T>::st(or_ + e, r.re);
      io<T>::st(oi + e, r.im);
    }
  }
}

template <typename T, bool BWD>
static int launch_fn(const void* zr, const void* zi, const void* gr, const void* gi, void* or_, void* oi, int64_t n, int fn,
                     hipStream_t st) {
  const int grid = stream_grid(n / v16<T>::N + 1, kFT);
#define CF_CASE(F)                                                                                                   \
  case F:                                                                                                            \
    cplx_fn_kernel<T, F, BWD><<<grid, kFT, 0, st>>>((const T*)zr, (const T*)zi, (const T*)gr, (const T*)gi, (T*)or_, \
                                                    (T*)oi, n);                                                      \
    break;
  switch (fn) {
    CF_CASE(CPLXAMD_FN_EXP)
    CF_CASE(CPLXAMD_FN_LOG)
    CF_CASE(CPLXAMD_FN_SIN)
    CF_CASE(CPLXAMD_FN_COS)
    CF_CASE(CPLXAMD_FN_TAN)
    CF_CASE(CPLXAMD_FN_SINH)
    CF_CASE(CPLXAMD_FN_COSH)
    CF_CASE(CPLXAMD_FN_TANH)
    default: return CPLXAMD_EINVAL;
  }
#undef CF_CASE
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

static bool fn_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int fn_args_ok(int64_t n, int fn, int dtype) {
  return n >= 0 && fn >= CPLXAMD_FN_EXP && fn <= CPLXAMD_FN_TANH && (dtype == CPLXAMD_F32 || dtype == CPLXAMD_BF16);
}

}  // namespace cplxamd

using namespace cplxamd;

extern "C" {

int cplxamd_cplx_fn_fwd(const void* z_r, const void* z_i, void* y_r, void* y_i, int64_t n, int fn, int dtype,
                        void* stream) {
  if (!fn_args_ok(n, fn, dtype) || (n > 0 && (!z_r || !z_i || !y_r || !y_i))) return CPLXAMD_EINVAL;
  if (n == 0) return 0;
  if (!fn_al16(z_r) || !fn_al16(z_i) || !fn_al16(y_r) || !fn_al16(y_i)) return CPLXAMD_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F32) return launch_fn<float, false>(z_r, z_i, nullptr, nullptr, y_r, y_i, n, fn, st);
  return launch_fn<bf16_t, false>(z_r, z_i, nullptr, nullptr, y_r, y_i, n, fn, st);
}

int cplxamd_cplx_fn_bwd(const void* z_r, const void* z_i, const void* g_r, const void* g_i, void* dz_r, void* dz_i,
                        int64_t n, int fn, int dtype, void* stream) {
  if (!fn_args_ok(n, fn, dtype) || (n > 0 && (!z_r || !z_i || !g_r || !g_i || !dz_r || !dz_i))) return CPLXAMD_EINVAL;
  if (n == 0) return 0;
  if (!fn_al16(z_r) || !fn_al16(z_i) || !fn_al16(g_r) || !fn_al16(g_i) || !fn_al16(dz_r) || !fn_al16(dz_i))
    return CPLXAMD_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F32) return launch_fn<float, true>(z_r, z_i, g_r, g_i, dz_r, dz_i, n, fn, st);
  return launch_fn<bf16_t, true>(z_r, z_i, g_r, g_i, dz_r, dz_i, n, fn, st);
}

}  // extern "C"
