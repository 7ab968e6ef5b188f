// K3: complex 3-d convolution (cross-correlation, planar [B, C, D, H, W], groups, stride, padding, dilation) forward,
// dgrad and wgrad as implicit GEMMs on the exact-f32 matrix cores -- the 3-d version of conv.hip's generic kernel.
// Operand tiles are gathered on the fly into LDS (im2col is never materialised) and contracted with
// v_mfma_f32_32x32x2_f32; complex = 4 MFMA chains sharing one K loop.  Operands (float32 or bf16) are converted to
// float32 on load, sums are float32, one rounding on store.
//
//   FWD    Y[b,co,od,oh,ow]  = sum_{ci,kd,kh,kw} X[b,ci,od*s-p+kd*d, ..] * W[co,ci,kd,kh,kw]
//          GEMM: M = Co/g, N = B*Do*Ho*Wo, K = Ci/g*KD*KH*KW
//   DGRAD  dX[b,ci,id,ih,iw] = sum_{co,kd,kh,kw} G[b,co,od,oh,ow] * conj(W[co,ci,kd,kh,kw]) (+ bias[ci]),
//          od = (id+p-kd*d)/s;  GEMM: M = Ci/g, N = B*D*H*W, K = Co/g*KD*KH*KW
//   WGRAD  dW[co,ci,kd,kh,kw] = sum_{b,od,oh,ow} G[b,co,od,oh,ow] * conj(X[b,ci,od*s-p+kd*d, ..])
//          GEMM: M = Co/g, N = Ci/g*KD*KH*KW, K = B*Do*Ho*Wo, split-K into fp32 partial slabs that a second kernel
//          sums in a fixed order (no atomics: the same bits on every run).
//
// DGRAD is the forward pass of CplxConvTranspose3d (conv3d.py), which is why it takes the bias: it joins the float32
// sums before their one rounding.
//
// Tiling: 64 x 64 outputs per workgroup of four waves (2 x 2, a 32 x 32 MFMA block each), K in steps of 16,
// double-buffered in LDS: the gathers of step t + 1 are in flight while the MFMAs of step t run.  Layers with M <= 32
// (a decoder's 64 -> 32 channels) run a 32-ROW tile, 32 x 128 (waves 1 x 4), not the 64-row tile padded: on the padded
// tile half of every MFMA multiplies zero rows, and the kernel is bound by its MFMAs there (measured: 64 -> 32 channels,
// kernel 4, stride 2 ran at 0.25 of the float32 matrix peak in NEEDED products, i.e. 0.5 in issued ones).  Same waves,
// same K step, same LDS scheme; the index maps differ only in the tile constants.
//
// Index arithmetic: pixel and tap indices are 32-bit and split with multiply-shift divisions; offsets into the tensors
// are 64-bit.  Every GEMM dimension and every pixel count is checked against one limit before any launch.  Every gather
// is predicated on its own coordinates in all three dimensions, every store on the tile's real extent.
#include "common.h"

namespace cplxamd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TBK = 16;
constexpr int tile_m(int64_t M) { return M <= 32 ? 32 : 64; }
constexpr int tile_n(int tm) { return tm == 32 ? 128 : 64; }   // (always 4 waves of one 32 x 32 block each)

// Division by a launch-constant divisor of indices below 2^31: q = (x * mul) >> (32 + sh), mul = floor(2^(31 + s) / d) + 1,
// s = ceil(log2 d), sh = s - 1 (Granlund-Montgomery round-up multiplier, exact for x < 2^31); d <= 1 passes x through.
struct Div3 { uint32_t mul, sh, d; };

Div3 make_div3(int64_t d64) {
  Div3 f{0u, 0u, (uint32_t)d64};
  if (d64 <= 1) { f.d = 1; return f; }
  uint32_t s = 0;
  while ((1ull << s) < (uint64_t)d64) ++s;
  f.mul = (uint32_t)(((1ull << (31 + s)) / (uint64_t)d64) + 1);
  f.sh = s - 1;
  return f;
}

__device__ __forceinline__ int div3(int x, const Div3& f) {       // x >= 0
  return f.d == 1 ? x : (int)(__umulhi((uint32_t)x, f.mul) >> f.sh);
}

template <typename T>
__device__ __forceinline__ float ld3(const void* p, int64_t off) {
  return io<T>::ld(reinterpret_cast<const T*>(p) + off);
}

struct Conv3P {
  int B, Ci, Co, D, H, W, KD, KH, KW, Do, Ho, Wo, sd, sh, sw, pd, ph, pw, dd, dh, dw, G;
  int Cg, Cog;                        // channels per group (in / out)
  int k3, khw, o3, howo, i3, hw;      // KD*KH*KW, KH*KW, Do*Ho*Wo, Ho*Wo, D*H*W, H*W
  Div3 f_k3, f_khw, f_kw, f_o3, f_howo, f_wo, f_i3, f_hw, f_w, f_sd, f_sh, f_sw;
};

enum { M3_FWD = 0, M3_DGRAD = 1, M3_WGRAD = 2 };

// Strided data gradient by PHASES (conv.hip, plan_dgrad_phases, with a depth axis).  Input voxel (id, ih, iw) receives tap
// (kd, kh, kw) only if (id + pd - kd dd) is a multiple of sd, and likewise in h and w: at stride 2 in three dimensions seven
// taps of eight multiply structural zeros in the plain implicit GEMM.  The voxels are split into sd x sh x sw classes by
// ((id + pd) mod sd, (ih + ph) mod sh, (iw + pw) mod sw); inside a class the valid taps are the same for every voxel -- an
// arithmetic progression kd = kd0 + a kds, a < nd, per dimension -- and the class is its own GEMM: N = voxels of the class,
// K = Co/g x nd x nh x nw.  blockIdx.z carries the class.  A class without a valid tap has K = 0: its K loop does not
// run and the epilogue stores the bias (or zeros), so every voxel of dX is written exactly once.
struct Dgrad3Phase {
  int id0, ih0, iw0, Dp, Hp, Wp;      // first plane / row / column of the class, and how many of each
  int kd0, kh0, kw0, nd, nh, nw;      // first valid tap and number of valid taps per dimension
  int N, K;                           // GEMM dims of the class
  int hpwp, n3, nhw;                  // Hp*Wp, nd*nh*nw, nh*nw
  Div3 f_p3, f_hpwp, f_wp, f_n3, f_nhw, f_nw;
};
constexpr int kMaxPhases3 = 8;

struct Conv3Args {
  const void* xr; const void* xi;     // FWD: input      DGRAD: grad out   WGRAD: grad out
  const void* wr; const void* wi;     // FWD: weight     DGRAD: weight     WGRAD: input
  const float* bias_r; const float* bias_i;   // DGRAD only: [Ci] (nullable pair)
  void* yr; void* yi;                 // output (WGRAD: fp32 partial slabs [splits][Co*Cg*KD*KH*KW])
  Conv3P p;
  int M, N, K;                        // GEMM dims per group (all below 2^31: checked at launch)
  int splits, kchunk;                 // WGRAD: split-K factor (1 otherwise), K elements per split
  int nph;                            // DGRAD: number of phases (0 = plain path)
  int kds, khs, kws;                  // DGRAD phases: tap steps
  Dgrad3Phase phase[kMaxPhases3];
};

// Operand elements per thread and K step: A (TM x 16): k = t & 15, rows (t >> 4) + 16 j; B (TN x 16): pixels fastest (FWD,
// DGRAD: row t % TN fixed, k = t / TN + (256 / TN) j -- the same for all lanes of a wave, so the split of k into channel and
// tap runs on the scalar unit) or k fastest (WGRAD: k = t & 15, rows (t >> 4) + 16 j).  Whatever is fixed per thread is
// decomposed once in front of the K loop.
template <typename T, int MODE, int TM>
__global__ __launch_bounds__(256) void conv3_kernel(Conv3Args a) {
  static_assert(TM == 64 || TM == 32, "tile rows");
  constexpr int TN = tile_n(TM), KBS = 256 / TN;               // B, pixels fastest: k stride between a thread's elements
  constexpr int ALD = TM + 1, BLD = TN + 1, AJ = TM / 16, BJ = TBK / KBS, WJ = TN / 16;
  __shared__ float As_r[2][TBK][ALD], As_i[2][TBK][ALD], Bs_r[2][TBK][BLD], Bs_i[2][TBK][BLD];
  const Conv3P& p = a.p;
  const int t = threadIdx.x;
  const bool phased = MODE == M3_DGRAD && a.nph > 0;
  const int zz = phased ? blockIdx.z / a.nph : blockIdx.z;
  const Dgrad3Phase& P = a.phase[phased ? blockIdx.z % a.nph : 0];
  const int g = zz / a.splits, split = zz % a.splits;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int Nn = phased ? P.N : a.N;                           // this launch's (class's) pixels
  if (n0 >= Nn) return;                                        // (phases: the grid is sized for the largest class)
  const int lane = t & 63, wid = t >> 6;
  const int wm = TM == 64 ? (wid >> 1) * 32 : 0, wn = TM == 64 ? (wid & 1) * 32 : wid * 32, l31 = lane & 31, lk = lane >> 5;
  const int kbeg = split * a.kchunk;
  int kend = kbeg + a.kchunk;
  if (kend > a.K) kend = a.K;
  if (phased) kend = P.K;
  // conjugation: DGRAD conj(W) is the A operand, WGRAD conj(X) is the B operand
  const float sa = (MODE == M3_DGRAD) ? -1.f : 1.f, sb = (MODE == M3_WGRAD) ? -1.f : 1.f;
  const void* a_r = MODE == M3_WGRAD ? a.xr : a.wr;
  const void* a_i = MODE == M3_WGRAD ? a.xi : a.wi;
  const void* b_r = MODE == M3_WGRAD ? a.wr : a.xr;
  const void* b_i = MODE == M3_WGRAD ? a.wi : a.xi;

  // ---- per-thread constants of the gathers
  const int ka = t & 15, ra0 = t >> 4;                         // A: k lane, first row
  const int rb = t % TN, kb0 = t / TN;                         // B (pixels fastest): row, first k
  // B row = output voxel (FWD) / input voxel (DGRAD): image, and the window origin
  bool b_ok = false;
  int b_d0 = 0, b_h0 = 0, b_w0 = 0;
  int64_t b_base = 0;
  if (MODE != M3_WGRAD) {
    const int n = n0 + rb;
    b_ok = n < Nn;
    if (b_ok) {
      if (phased) {
        const int b = div3(n, P.f_p3), r = n - b * (P.Dp * P.hpwp);
        const int tq = div3(r, P.f_hpwp), r2 = r - tq * P.hpwp;
        const int uq = div3(r2, P.f_wp), vq = r2 - uq * P.Wp;
        b_d0 = P.id0 + tq * p.sd + p.pd; b_h0 = P.ih0 + uq * p.sh + p.ph; b_w0 = P.iw0 + vq * p.sw + p.pw;
        b_base = ((int64_t)b * p.Co + (int64_t)g * p.Cog) * p.o3;
      } else if (MODE == M3_FWD) {
        const int b = div3(n, p.f_o3), r = n - b * p.o3;
        const int od = div3(r, p.f_howo), r2 = r - od * p.howo;
        const int oh = div3(r2, p.f_wo), ow = r2 - oh * p.Wo;
        b_d0 = od * p.sd - p.pd; b_h0 = oh * p.sh - p.ph; b_w0 = ow * p.sw - p.pw;
        b_base = ((int64_t)b * p.Ci + (int64_t)g * p.Cg) * p.i3;
      } else {
        const int b = div3(n, p.f_i3), r = n - b * p.i3;
        const int id = div3(r, p.f_hw), r2 = r - id * p.hw;
        const int ih = div3(r2, p.f_w), iw = r2 - ih * p.W;
        b_d0 = id + p.pd; b_h0 = ih + p.ph; b_w0 = iw + p.pw;
        b_base = ((int64_t)b * p.Co + (int64_t)g * p.Cog) * p.o3;
      }
    }
  }
  // WGRAD: B rows = (ci, kd, kh, kw) taps
  int w_ci[WJ], w_dd[WJ], w_dh[WJ], w_dw[WJ];
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    w_ci[j] = -1; w_dd[j] = w_dh[j] = w_dw[j] = 0;
    if (MODE == M3_WGRAD) {
      const int n = n0 + ra0 + 16 * j;
      if (n < a.N) {
        const int ci = div3(n, p.f_k3), rk = n - ci * p.k3;
        const int kd = div3(rk, p.f_khw), rk2 = rk - kd * p.khw;
        const int kh = div3(rk2, p.f_kw), kw = rk2 - kh * p.KW;
        w_ci[j] = ci; w_dd[j] = kd * p.dd - p.pd; w_dh[j] = kh * p.dh - p.ph; w_dw[j] = kw * p.dw - p.pw;
      }
    }
  }

  constexpr int NB = MODE == M3_WGRAD ? WJ : BJ;               // B elements per thread and K step
  float ar_[AJ], ai_[AJ], br_[NB], bi_[NB];
  auto fetch_both = [&](int k0) __attribute__((always_inline)) {
    // ---- A: weights (FWD: k contiguous; DGRAD: gathered) / grad-out (WGRAD: k = voxels, contiguous)
    const int gk = k0 + ka;
    const bool kok = gk < kend;
    int64_t abase = 0, astride = 0;                              // element (row m, this k) = abase + m * astride
    int wb = 0, wod = 0, woh = 0, wow = 0;                       // WGRAD: voxel of this k
    if (MODE == M3_FWD) {
      abase = (int64_t)g * p.Cog * a.K + gk; astride = a.K;
    } else if (MODE == M3_DGRAD) {
      int co, r;
      if (phased) {
        co = kok ? div3(gk, P.f_n3) : 0;
        const int rk = gk - co * P.n3, ta = kok ? div3(rk, P.f_nhw) : 0;
        const int rk2 = rk - ta * P.nhw, tb = kok ? div3(rk2, P.f_nw) : 0;
        r = ((P.kd0 + ta * a.kds) * p.KH + P.kh0 + tb * a.khs) * p.KW + P.kw0 + (rk2 - tb * P.nw) * a.kws;
      } else {
        co = kok ? div3(gk, p.f_k3) : 0; r = gk - co * p.k3;
      }
      abase = ((int64_t)g * p.Cog + co) * p.Cg * p.k3 + r; astride = p.k3;
    } else {
      wb = kok ? div3(gk, p.f_o3) : 0;
      const int r = gk - wb * p.o3;
      wod = kok ? div3(r, p.f_howo) : 0;
      const int r2 = r - wod * p.howo;
      woh = kok ? div3(r2, p.f_wo) : 0; wow = r2 - woh * p.Wo;
      abase = ((int64_t)wb * p.Co + (int64_t)g * p.Cog) * p.o3 + r; astride = p.o3;
    }
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int m = m0 + ra0 + 16 * j;
      float vr = 0.f, vi = 0.f;
      if (kok && m < a.M) {
        const int64_t off = abase + (int64_t)m * astride;
        vr = ld3<T>(a_r, off);
        vi = ld3<T>(a_i, off);
      }
      ar_[j] = vr; ai_[j] = vi;
    }
    if (MODE == M3_WGRAD) {
      // ---- B, k fastest: the same k (voxel), rows = taps
      const int idb = wod * p.sd, ihb = woh * p.sh, iwb = wow * p.sw;
      const int64_t xb = ((int64_t)wb * p.Ci + (int64_t)g * p.Cg) * p.i3;
#pragma unroll
      for (int j = 0; j < WJ; ++j) {
        float vr = 0.f, vi = 0.f;
        const int id = idb + w_dd[j], ih = ihb + w_dh[j], iw = iwb + w_dw[j];
        if (kok && w_ci[j] >= 0 && id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
          const int64_t off = xb + (((int64_t)w_ci[j] * p.D + id) * p.H + ih) * p.W + iw;
          vr = ld3<T>(b_r, off);
          vi = ld3<T>(b_i, off);
        }
        br_[j] = vr; bi_[j] = vi;
      }
    } else {
      // ---- B, pixels fastest
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        const int k = __builtin_amdgcn_readfirstlane(k0 + kb0 + KBS * j);
        float vr = 0.f, vi = 0.f;
        if (b_ok && k < kend) {
          int c, kd, kh, kw;                                     // c: input channel (FWD) / output channel (DGRAD)
          if (phased) {
            c = div3(k, P.f_n3);
            const int rk = k - c * P.n3, ta = div3(rk, P.f_nhw);
            const int rk2 = rk - ta * P.nhw, tb = div3(rk2, P.f_nw);
            kd = P.kd0 + ta * a.kds; kh = P.kh0 + tb * a.khs; kw = P.kw0 + (rk2 - tb * P.nw) * a.kws;
          } else {
            c = div3(k, p.f_k3);
            const int rk = k - c * p.k3;
            kd = div3(rk, p.f_khw);
            const int rk2 = rk - kd * p.khw;
            kh = div3(rk2, p.f_kw); kw = rk2 - kh * p.KW;
          }
          if (MODE == M3_FWD) {
            const int id = b_d0 + kd * p.dd, ih = b_h0 + kh * p.dh, iw = b_w0 + kw * p.dw;
            if (id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) {
              const int64_t off = b_base + (((int64_t)c * p.D + id) * p.H + ih) * p.W + iw;
              vr = ld3<T>(b_r, off);
              vi = ld3<T>(b_i, off);
            }
          } else {
            const int td = b_d0 - kd * p.dd, th = b_h0 - kh * p.dh, tw = b_w0 - kw * p.dw;
            if (td >= 0 && th >= 0 && tw >= 0) {
              const int od = div3(td, p.f_sd), oh = div3(th, p.f_sh), ow = div3(tw, p.f_sw);
              if (od * p.sd == td && oh * p.sh == th && ow * p.sw == tw && od < p.Do && oh < p.Ho && ow < p.Wo) {
                const int64_t off = b_base + (((int64_t)c * p.Do + od) * p.Ho + oh) * p.Wo + ow;
                vr = ld3<T>(b_r, off);
                vi = ld3<T>(b_i, off);
              }
            }
          }
        }
        br_[j] = vr; bi_[j] = vi;
      }
    }
  };
  auto commit = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      As_r[buf][ka][ra0 + 16 * j] = ar_[j];
      As_i[buf][ka][ra0 + 16 * j] = ai_[j];
    }
    if (MODE == M3_WGRAD) {
#pragma unroll
      for (int j = 0; j < WJ; ++j) {
        Bs_r[buf][ka][ra0 + 16 * j] = br_[j];
        Bs_i[buf][ka][ra0 + 16 * j] = bi_[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < BJ; ++j) {
        Bs_r[buf][kb0 + KBS * j][rb] = br_[j];
        Bs_i[buf][kb0 + KBS * j][rb] = bi_[j];
      }
    }
  };

  f32x16 acc_r = {0}, acc_i = {0};
  if (kbeg < kend) fetch_both(kbeg);
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += TBK, buf ^= 1) {
    commit(buf);
    __syncthreads();                         // tile visible; the other buffer is free again
    if (k0 + TBK < kend) fetch_both(k0 + TBK);
#pragma unroll
    for (int kk = 0; kk < TBK; kk += 2) {
      const int kr = kk + lk;
      const float ar = As_r[buf][kr][wm + l31];
      const float br = Bs_r[buf][kr][wn + l31];
      const float ai = sa * As_i[buf][kr][wm + l31];
      const float bi = sb * Bs_i[buf][kr][wn + l31];
      acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, acc_r, 0, 0, 0);
      acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, bi, acc_r, 0, 0, 0);
      acc_i = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, acc_i, 0, 0, 0);
      acc_i = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, acc_i, 0, 0, 0);
    }
  }

  // epilogue: col = lane & 31 runs along N, rows (M) across registers
  const int n = n0 + wn + l31;
  if (n >= Nn) return;
  int64_t out_base, out_mstride;
  if (MODE == M3_FWD) {
    const int b = div3(n, p.f_o3), r = n - b * p.o3;
    out_base = ((int64_t)b * p.Co + (int64_t)g * p.Cog) * p.o3 + r;
    out_mstride = p.o3;
  } else if (MODE == M3_DGRAD) {
    int b, r;
    if (phased) {
      b = div3(n, P.f_p3);
      const int rr = n - b * (P.Dp * P.hpwp), tq = div3(rr, P.f_hpwp);
      const int r2 = rr - tq * P.hpwp, uq = div3(r2, P.f_wp), vq = r2 - uq * P.Wp;
      r = ((P.id0 + tq * p.sd) * p.H + P.ih0 + uq * p.sh) * p.W + P.iw0 + vq * p.sw;
    } else {
      b = div3(n, p.f_i3); r = n - b * p.i3;
    }
    out_base = ((int64_t)b * p.Ci + (int64_t)g * p.Cg) * p.i3 + r;
    out_mstride = p.i3;
  } else {
    const int64_t wsz = (int64_t)p.Co * p.Cg * p.k3;
    out_base = (int64_t)split * wsz + (int64_t)g * p.Cog * a.N + n;
    out_mstride = a.N;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
    if (m >= a.M) continue;
    const int64_t o = out_base + (int64_t)m * out_mstride;
    float vr = acc_r[r], vi = acc_i[r];
    if (MODE == M3_DGRAD && a.bias_r) {      // joins the float32 sums before their one rounding
      vr += a.bias_r[g * p.Cg + m];
      vi += a.bias_i[g * p.Cg + m];
    }
    if (MODE == M3_WGRAD) {
      reinterpret_cast<float*>(a.yr)[o] = vr;
      reinterpret_cast<float*>(a.yi)[o] = vi;
    } else {
      io<T>::st(reinterpret_cast<T*>(a.yr) + o, vr);
      io<T>::st(reinterpret_cast<T*>(a.yi) + o, vi);
    }
  }
}

// out[i] = sum_s slab[s][i], s ascending: one thread per element (coalesced across the block), fixed order.
// blockIdx.y = plane.
__global__ __launch_bounds__(256) void slab_sum3_kernel(const float* slabs0, const float* slabs1, int splits, int64_t n,
                                                        float* out0, float* out1) {
  const float* slabs = blockIdx.y ? slabs1 : slabs0;
  float* out = blockIdx.y ? out1 : out0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int s = 0; s < splits; ++s) acc += slabs[(int64_t)s * n + i];
  out[i] = acc;
}

int gcd3(int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; }

// first valid tap, number of valid taps of residue r: taps k < K with (k d) mod s == r
void taps3(int K, int d, int s, int r, int& k0, int& n) {
  k0 = 0; n = 0;
  for (int k = 0; k < K; ++k)
    if ((k * d) % s == r) { if (!n) k0 = k; ++n; }
}

// DGRAD: the phase plan for strides of 1 or 2 per dimension with at least one 2; leaves a.nph = 0 (plain path) otherwise
void plan_dgrad3_phases(Conv3Args& a) {
  const Conv3P& p = a.p;
  a.nph = 0;
  if ((p.sd == 1 && p.sh == 1 && p.sw == 1) || p.sd > 2 || p.sh > 2 || p.sw > 2) return;
  a.kds = p.sd / gcd3(p.dd, p.sd);
  a.khs = p.sh / gcd3(p.dh, p.sh);
  a.kws = p.sw / gcd3(p.dw, p.sw);
  int n = 0;
  for (int rd = 0; rd < p.sd; ++rd)
    for (int rh = 0; rh < p.sh; ++rh)
      for (int rw = 0; rw < p.sw; ++rw) {
        Dgrad3Phase& q = a.phase[n++];
        q.id0 = ((rd - p.pd) % p.sd + p.sd) % p.sd;
        q.ih0 = ((rh - p.ph) % p.sh + p.sh) % p.sh;
        q.iw0 = ((rw - p.pw) % p.sw + p.sw) % p.sw;
        q.Dp = q.id0 < p.D ? (p.D - q.id0 + p.sd - 1) / p.sd : 0;
        q.Hp = q.ih0 < p.H ? (p.H - q.ih0 + p.sh - 1) / p.sh : 0;
        q.Wp = q.iw0 < p.W ? (p.W - q.iw0 + p.sw - 1) / p.sw : 0;
        taps3(p.KD, p.dd, p.sd, rd, q.kd0, q.nd);
        taps3(p.KH, p.dh, p.sh, rh, q.kh0, q.nh);
        taps3(p.KW, p.dw, p.sw, rw, q.kw0, q.nw);
        q.hpwp = q.Hp * q.Wp; q.nhw = q.nh * q.nw; q.n3 = q.nd * q.nhw;
        q.N = p.B * q.Dp * q.hpwp;                               // (<= B*D*H*W, which fill_geom3 has checked)
        q.K = p.Cog * q.n3;                                      // (<= Cog*KD*KH*KW, likewise)
        q.f_p3 = make_div3((int64_t)q.Dp * q.hpwp); q.f_hpwp = make_div3(q.hpwp); q.f_wp = make_div3(q.Wp);
        q.f_n3 = make_div3(q.n3); q.f_nhw = make_div3(q.nhw); q.f_nw = make_div3(q.nw);
      }
  a.nph = n;
}

template <typename T, int MODE>
int conv3_launch(Conv3Args& a, hipStream_t st) {
  int64_t nmax = a.N;                                          // DGRAD by phases: the largest class sizes the grid
  const bool phased = MODE == M3_DGRAD && a.nph > 0;
  if (phased) {
    nmax = 0;
    for (int i = 0; i < a.nph; ++i) nmax = a.phase[i].N > nmax ? a.phase[i].N : nmax;
  }
  const int tm = tile_m(a.M), tn = tile_n(tm);
  const int64_t gy = ((int64_t)a.M + tm - 1) / tm, gz = (int64_t)a.p.G * a.splits * (phased ? a.nph : 1);
  if (gy > 65535 || gz > 65535) return CPLXAMD_ESHAPE;
  dim3 grid((unsigned)((nmax + tn - 1) / tn), (unsigned)gy, (unsigned)gz);
  if (tm == 32) conv3_kernel<T, MODE, 32><<<grid, 256, 0, st>>>(a);
  else conv3_kernel<T, MODE, 64><<<grid, 256, 0, st>>>(a);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

int out_extent3(int64_t L, int64_t k, int64_t s, int64_t p, int64_t d) {
  const int64_t num = L + 2 * p - d * (k - 1) - 1;
  if (num < 0) return 0;
  const int64_t o = num / s + 1;
  return o > 0x7fffffff ? 0 : (int)o;
}

int fill_geom3(const int* g, Conv3P& p) {
  // g = {B, Ci, Co, D, H, W, KD, KH, KW, sd, sh, sw, pd, ph, pw, dd, dh, dw, groups}
  p.B = g[0]; p.Ci = g[1]; p.Co = g[2]; p.D = g[3]; p.H = g[4]; p.W = g[5]; p.KD = g[6]; p.KH = g[7]; p.KW = g[8];
  p.sd = g[9]; p.sh = g[10]; p.sw = g[11]; p.pd = g[12]; p.ph = g[13]; p.pw = g[14];
  p.dd = g[15]; p.dh = g[16]; p.dw = g[17]; p.G = g[18];
  if (p.G <= 0 || p.sd <= 0 || p.sh <= 0 || p.sw <= 0 || p.dd <= 0 || p.dh <= 0 || p.dw <= 0) return CPLXAMD_EINVAL;
  if (p.B < 0 || p.pd < 0 || p.ph < 0 || p.pw < 0) return CPLXAMD_EINVAL;
  if (p.Ci <= 0 || p.Co <= 0 || p.D <= 0 || p.H <= 0 || p.W <= 0 || p.KD <= 0 || p.KH <= 0 || p.KW <= 0)
    return CPLXAMD_ESHAPE;
  if (p.Ci % p.G != 0 || p.Co % p.G != 0) return CPLXAMD_ESHAPE;
  p.Do = out_extent3(p.D, p.KD, p.sd, p.pd, p.dd);
  p.Ho = out_extent3(p.H, p.KH, p.sh, p.ph, p.dh);
  p.Wo = out_extent3(p.W, p.KW, p.sw, p.pw, p.dw);
  if (p.Do <= 0 || p.Ho <= 0 || p.Wo <= 0) return CPLXAMD_ESHAPE;
  p.Cg = p.Ci / p.G; p.Cog = p.Co / p.G;
  // the gathers index voxels and taps in 32 bits (offsets into the tensors stay 64-bit): the limit of conv.hip's
  // fill_geom (room for the split-K chunk rounding), on every GEMM dimension and every voxel count
  const int64_t lim = 0x7fe00000;
  const int64_t nb = p.B > 0 ? p.B : 1;
  const int64_t k3 = (int64_t)p.KD * p.KH * p.KW;
  if (k3 > lim) return CPLXAMD_ESHAPE;
  const int64_t hw = (int64_t)p.H * p.W, howo = (int64_t)p.Ho * p.Wo;
  if (hw > lim || howo > lim) return CPLXAMD_ESHAPE;
  const int64_t i3 = hw * p.D, o3 = howo * p.Do;
  if (i3 > lim || o3 > lim || nb * i3 > lim || nb * o3 > lim || p.Cg * k3 > lim || p.Cog * k3 > lim) return CPLXAMD_ESHAPE;
  // (window coordinates: od * s - p + kd * d and id + p stay far inside 32 bits only if the terms do)
  if ((int64_t)p.KD * p.dd > lim || (int64_t)p.KH * p.dh > lim || (int64_t)p.KW * p.dw > lim ||
      (int64_t)p.D + p.pd > lim || (int64_t)p.H + p.ph > lim || (int64_t)p.W + p.pw > lim)
    return CPLXAMD_ESHAPE;
  p.k3 = (int)k3; p.khw = p.KH * p.KW; p.o3 = (int)o3; p.howo = (int)howo; p.i3 = (int)i3; p.hw = (int)hw;
  p.f_k3 = make_div3(k3); p.f_khw = make_div3(p.khw); p.f_kw = make_div3(p.KW);
  p.f_o3 = make_div3(o3); p.f_howo = make_div3(howo); p.f_wo = make_div3(p.Wo);
  p.f_i3 = make_div3(i3); p.f_hw = make_div3(hw); p.f_w = make_div3(p.W);
  p.f_sd = make_div3(p.sd); p.f_sh = make_div3(p.sh); p.f_sw = make_div3(p.sw);
  return 0;
}

// split-K factor of the weight gradient: ~3 workgroups per CU, at least four K steps per split
int wgrad3_splits(const Conv3P& p) {
  const int64_t K = (int64_t)p.B * p.o3;
  const int tm = tile_m(p.Cog), tn = tile_n(tm);
  const int64_t tiles = (int64_t)((p.Cog + tm - 1) / tm) * (((int64_t)p.Cg * p.k3 + tn - 1) / tn) * p.G;
  int64_t s = (768 + tiles - 1) / tiles;
  const int64_t maxs = (K + 4 * TBK - 1) / (4 * TBK);
  if (s > maxs) s = maxs;
  if (s * p.G > 65535) s = 65535 / p.G;
  if (s < 1) s = 1;
  return (int)s;
}

}  // namespace
}  // namespace cplxamd

using namespace cplxamd;

extern "C" {

int cplxamd_conv3d_out_shape(const int* geom, int* dout, int* ho, int* wo) {
  if (!geom || !dout || !ho || !wo) return CPLXAMD_EINVAL;
  Conv3P p;
  const int rc = fill_geom3(geom, p);
  if (rc) return rc;
  *dout = p.Do; *ho = p.Ho; *wo = p.Wo;
  return 0;
}

int cplxamd_conv3d_fwd(const void* xr, const void* xi, const void* wr, const void* wi, void* yr, void* yi,
                       const int* geom, int dtype, void* stream) {
  if (!xr || !xi || !wr || !wi || !yr || !yi || !geom) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  Conv3Args a{};
  const int rc = fill_geom3(geom, a.p);
  if (rc) return rc;
  if (a.p.B == 0) return 0;                                    // empty batch: nothing to write
  a.xr = xr; a.xi = xi; a.wr = wr; a.wi = wi; a.yr = yr; a.yi = yi;
  a.M = a.p.Cog; a.N = a.p.B * a.p.o3; a.K = a.p.Cg * a.p.k3;
  a.splits = 1; a.kchunk = a.K;
  hipStream_t st = (hipStream_t)stream;
  return dtype == CPLXAMD_F32 ? conv3_launch<float, M3_FWD>(a, st) : conv3_launch<bf16_t, M3_FWD>(a, st);
}

int cplxamd_conv3d_dgrad(const void* gr, const void* gi, const void* wr, const void* wi, const float* bias_r,
                         const float* bias_i, void* dxr, void* dxi, const int* geom, int dtype, int flags, void* stream) {
  if (!gr || !gi || !wr || !wi || !dxr || !dxi || !geom) return CPLXAMD_EINVAL;
  if (flags & ~CPLXAMD_CONV3D_PLAIN) return CPLXAMD_EINVAL;
  if ((bias_r == nullptr) != (bias_i == nullptr)) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  Conv3Args a{};
  const int rc = fill_geom3(geom, a.p);
  if (rc) return rc;
  if (a.p.B == 0) return 0;
  a.xr = gr; a.xi = gi; a.wr = wr; a.wi = wi; a.bias_r = bias_r; a.bias_i = bias_i; a.yr = dxr; a.yi = dxi;
  a.M = a.p.Cg; a.N = a.p.B * a.p.i3; a.K = a.p.Cog * a.p.k3;
  a.splits = 1; a.kchunk = a.K;
  if (!(flags & CPLXAMD_CONV3D_PLAIN)) plan_dgrad3_phases(a);
  hipStream_t st = (hipStream_t)stream;
  return dtype == CPLXAMD_F32 ? conv3_launch<float, M3_DGRAD>(a, st) : conv3_launch<bf16_t, M3_DGRAD>(a, st);
}

int64_t cplxamd_conv3d_wgrad_ws_bytes(const int* geom) {
  if (!geom) return -1;
  Conv3P p;
  if (fill_geom3(geom, p)) return -1;
  const int64_t wsz = (int64_t)p.Co * p.Cg * p.k3;
  // [planes][splits] slabs of wsz floats
  return ((int64_t)wgrad3_splits(p) * wsz * (int64_t)sizeof(float) * 2 + 255) / 256 * 256;
}

int cplxamd_conv3d_wgrad(const void* gr, const void* gi, const void* xr, const void* xi, float* dwr, float* dwi,
                         const int* geom, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!gr || !gi || !xr || !xi || !dwr || !dwi || !geom || !ws) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  Conv3Args a{};
  int rc = fill_geom3(geom, a.p);
  if (rc) return rc;
  const int64_t wsz = (int64_t)a.p.Co * a.p.Cg * a.p.k3;
  if ((wsz + 255) / 256 > 0x7fffffff) return CPLXAMD_ESHAPE;   // (the slab sum's grid)
  hipStream_t st = (hipStream_t)stream;
  if (a.p.B == 0) {                                          // empty batch: the gradient is zero
    hipError_t e = hipMemsetAsync(dwr, 0, wsz * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(dwi, 0, wsz * sizeof(float), st);
    return (int)e;
  }
  if (ws_bytes < cplxamd_conv3d_wgrad_ws_bytes(geom)) return CPLXAMD_EWS;
  a.splits = wgrad3_splits(a.p);
  a.M = a.p.Cog; a.N = a.p.Cg * a.p.k3; a.K = a.p.B * a.p.o3;
  a.xr = gr; a.xi = gi; a.wr = xr; a.wi = xi;
  a.yr = ws; a.yi = (float*)ws + (int64_t)a.splits * wsz;
  a.kchunk = (int)((((int64_t)a.K + a.splits - 1) / a.splits + TBK - 1) / TBK * TBK);
  rc = dtype == CPLXAMD_F32 ? conv3_launch<float, M3_WGRAD>(a, st) : conv3_launch<bf16_t, M3_WGRAD>(a, st);
  if (rc) return rc;
  slab_sum3_kernel<<<dim3((unsigned)((wsz + 255) / 256), 2), 256, 0, st>>>((const float*)a.yr, (const float*)a.yi, a.splits,
                                                                         wsz, dwr, dwi);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
