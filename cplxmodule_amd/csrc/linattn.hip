// Linear attention with a per-step complex decay: the recurrence whose state is a matrix (cplx.linear_attention; DESIGN
// section 30).  In processing order p (row p, or T - 1 - p in reverse), with S an E x Ev complex matrix:
//
//   S[p] = exp(mu[p]) S[p - 1] + k[p]^H (x) v[p],   o[p] = scale q[p] S[p]
//        = scale sum_{s <= p} exp(M[p] - M[s]) (q[p] k[s]^H) v[s] + scale exp(M[p]) q[p] S[-1],   M = prefix sum of mu
//
// ONE launch.  A workgroup of four waves owns one batch entry and SV = 32 columns of v (and of S), and walks the row in
// chunks of C = 32 steps.  Per chunk, every product runs on v_mfma_f32_32x32x2_f32, complex products as chains of depth
// 2 x (inner size) over the concatenated planes [re | im]:
//   phase A  one chain per wave:  Re P, Im P of P = Q K^H (C x C)  and  Re, Im of Q S (C x SV), accumulators to LDS
//   phase B  pointwise, 256 threads: P[t][s] *= exp(M[t] - M[s]) for s <= t, 0 above the diagonal;
//            Vw[s] = exp(M[C - 1] - M[s]) v[s] (times scale under SCALE_IN); w[t] = exp(M[t])
//   phase C  tile jobs dealt to the waves: the DE / 32 row tiles of S <- exp(M[C - 1]) S + K^H Vw (read, updated and
//            written back by the lane that owns the entry), then Re O and Im O of O = P V + diag(w) Q S, stored from
//            the accumulator (lane = column: a wave's store covers whole 128-byte rows)
// S lives in LDS as float32 for the whole row and is never rounded.  M is the in-chunk inclusive prefix of mu, one
// scan of wave 0 in float64 (64 values per chunk); every exponent is a DIFFERENCE of two prefixes, reduced to
// [-pi, pi] in its imaginary part and rounded once to float32, then cexp.h's f_exp: for Re lambda <= 0 no exponent has
// a positive real part and no ratio of large numbers is formed.  Without a decay (DECAY = false) the instance holds no
// exponential and every weight is exactly 1.  The global loads of chunk c + 1 are issued (into registers) before the
// products of chunk c; bf16 operands are widened to float32 when they are committed to LDS, o is rounded once.
// E rounds up to the compiled head DE (32, 64, 128) and a ragged last chunk to C by zero fill at the commit (predicated
// loads); no MFMA step is branched around.  No atomics, no spin loops, no workspace, no scratch (DESIGN
// 30.3); the same input gives the same bits.  Workgroups whose value slices differ recompute P and Q S's share of the
// loads of q and k.
#include <cmath>

#include "common.h"
#include "launch.h"
#include "prims.h"
#include "runs.h"

namespace cplxamd {
#include "cexp.h"
namespace la {

constexpr int C = 32;                         // steps per chunk
constexpr int SV = 32;                        // value columns per workgroup
constexpr int LV = 2 * SV + 1;                // row of [v_r | v_i], of Vw and of [S_r | S_i] (odd: rows fall into distinct banks)
constexpr int LP = C + 1;                     // row of a C x C (or C x SV) accumulator tile

struct Args {
  const void *q_r, *q_i, *k_r, *k_i, *v_r, *v_i;
  const float *l_r, *l_i, *s_r, *s_i;
  void *o_r, *o_i;
  float *f_r, *f_i;
  int T, E, Ev, slices, reverse, conj, lag, scale_in;
  float scale;
  int64_t size[3];
  int64_t bq[3], bk[3], bv[3], bl[3], bs[3], bo[3], bf[3];
  int64_t rq, rk, rv, ro, rs, rf;
};

// the LDS of an instance, in floats (the 2 C doubles of the prefix come first)
template <int DE>
struct Lay {
  static constexpr int LQ = 2 * DE + 1;       // row of [q_r | q_i] and of [k_r | k_i]
  static constexpr int Q = 4 * C, K = Q + C * LQ, V = K + C * LQ, VW = V + C * LV, P = VW + C * LV, O = P + 2 * C * LP,
                       S = O + 2 * C * LP, W = S + DE * LV, END = W + 2 * C;
  static constexpr int LDS = END * 4;
};

__device__ __forceinline__ int64_t batch_off(const Args& g, int64_t b, const int64_t (&st)[3]) {
  const int64_t i2 = b % g.size[2], w = b / g.size[2], i1 = w % g.size[1], i0 = w / g.size[1];
  return i0 * st[0] + i1 * st[1] + i2 * st[2];
}

__device__ __forceinline__ f32x16 mma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// D[row][col] = sum_x a0[row][x] b0[x][col] + sa1 sb1 sum_x a1[row][x] b1[x][col], x < DEPTH: the lane's pointers are at
// its row of a (x strides by `as`) and at its column of b (x strides by `bs`)
template <int DEPTH>
__device__ __forceinline__ f32x16 chain(const float* a0, const float* a1, int as, float sa1, const float* b0, const float* b1,
                                        int bs, float sb1, int lk) {
  f32x16 c = f32x16{0};
#pragma unroll 8
  for (int s = 0; s < DEPTH / 2; ++s) c = mma(a0[(2 * s + lk) * as], b0[(2 * s + lk) * bs], c);
#pragma unroll 8
  for (int s = 0; s < DEPTH / 2; ++s) c = mma(sa1 * a1[(2 * s + lk) * as], sb1 * b1[(2 * s + lk) * bs], c);
  return c;
}

// exp of a difference of two prefixes: the imaginary part is brought to [-pi, pi] before it is rounded to float32
__device__ __forceinline__ CF wexp(double re, double im) {
  constexpr double kTwoPi = 6.283185307179586476925286766559;
  im -= kTwoPi * rint(im * (1.0 / kTwoPi));
  return f_exp((float)re, (float)im);
}

template <typename T, int DE, bool DECAY>
__global__ __launch_bounds__(256) void linattn_kernel(Args g) {
  using L = Lay<DE>;
  constexpr int LQ = L::LQ, NE = DE / 32, QCH = C * 2 * DE / 256, VCH = C * 2 * SV / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sM = reinterpret_cast<double*>(smem);       // [re | im][C]: the inclusive prefix of mu inside the chunk
  float* sm = reinterpret_cast<float*>(smem);
  float *sQ = sm + L::Q, *sK = sm + L::K, *sV = sm + L::V, *sVw = sm + L::VW, *sP = sm + L::P, *sO = sm + L::O,
        *sS = sm + L::S, *sW = sm + L::W;

  const int v0 = (int)(blockIdx.x % (uint32_t)g.slices) * SV;
  const int64_t b = blockIdx.x / (uint32_t)g.slices;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l31 = lane & 31, lk = lane >> 5;
  const int64_t qo = batch_off(g, b, g.bq), ko = batch_off(g, b, g.bk), vo = batch_off(g, b, g.bv);
  const T *qr = reinterpret_cast<const T*>(g.q_r) + qo, *qi = reinterpret_cast<const T*>(g.q_i) + qo;
  const T *kr = reinterpret_cast<const T*>(g.k_r) + ko, *ki = reinterpret_cast<const T*>(g.k_i) + ko;
  const T *vr = reinterpret_cast<const T*>(g.v_r) + vo, *vi = reinterpret_cast<const T*>(g.v_i) + vo;

  // ---- the state that enters step 0 (zeros past E and Ev, and without one)
  {
    const int64_t so = g.s_r ? batch_off(g, b, g.bs) : 0;
    for (int idx = threadIdx.x; idx < DE * 2 * SV; idx += 256) {
      const int e = idx / (2 * SV), rem = idx % (2 * SV), pl = rem / SV, col = rem % SV;
      const bool ok = g.s_r && e < g.E && v0 + col < g.Ev;
      sS[e * LV + pl * SV + col] = ok ? (pl ? g.s_i : g.s_r)[so + (int64_t)e * g.rs + v0 + col] : 0.0f;
    }
  }

  // ---- global -> registers: chunk rows p0 .. p0 + C - 1 of q, k and the v slice, and mu; zeros past T, E and Ev
  float rq[QCH], rk[QCH], rv[VCH], rlr = 0.0f, rli = 0.0f;
  auto fetch = [&](int p0) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));     // addresses are rebuilt per chunk, not kept in registers across the loop
#pragma unroll
    for (int n = 0; n < QCH; ++n) {
      const int c = tid + 256 * n, col = c % DE, rest = c / DE, pl = rest & 1, p = p0 + (rest >> 1);
      const bool ok = p < g.T && col < g.E;
      const int64_t tt = g.reverse ? g.T - 1 - p : p;
      rq[n] = ok ? io<T>::ld((pl ? qi : qr) + tt * g.rq + col) : 0.0f;
      rk[n] = ok ? io<T>::ld((pl ? ki : kr) + tt * g.rk + col) : 0.0f;
    }
#pragma unroll
    for (int n = 0; n < VCH; ++n) {
      const int c = tid + 256 * n, col = c % SV, rest = c / SV, pl = rest & 1, p = p0 + (rest >> 1);
      const bool ok = p < g.T && v0 + col < g.Ev;
      const int64_t tt = g.reverse ? g.T - 1 - p : p;
      rv[n] = ok ? io<T>::ld((pl ? vi : vr) + tt * g.rv + v0 + col) : 0.0f;
    }
    if constexpr (DECAY) {
      if (tid < C) {                  // mu of step p: lambda of step p, or of step p - 1 under LAG (step 0: none)
        const int p = p0 + tid, pp = g.lag ? p - 1 : p;
        const bool ok = p < g.T && pp >= 0;
        const int64_t at = batch_off(g, b, g.bl) + (g.reverse ? g.T - 1 - pp : pp);
        rlr = ok ? g.l_r[at] : 0.0f;
        rli = ok && g.l_i ? g.l_i[at] : 0.0f;
        if (g.conj) rli = -rli;
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int n = 0; n < QCH; ++n) {
      const int c = threadIdx.x + 256 * n, col = c % DE, rest = c / DE, pl = rest & 1, row = rest >> 1;
      sQ[row * LQ + pl * DE + col] = rq[n];
      sK[row * LQ + pl * DE + col] = rk[n];
    }
#pragma unroll
    for (int n = 0; n < VCH; ++n) {
      const int c = threadIdx.x + 256 * n, col = c % SV, rest = c / SV, pl = rest & 1, row = rest >> 1;
      sV[row * LV + pl * SV + col] = rv[n];
    }
    if constexpr (DECAY) {
      if (wid == 0) {                 // the inclusive prefix over the chunk: one scan of 32 lanes, in float64
        double mr = rlr, mi = rli;
#pragma unroll
        for (int d = 1; d < C; d *= 2) {
          const double ur = __shfl_up(mr, d, 32), ui = __shfl_up(mi, d, 32);
          if (l31 >= d) {
            mr += ur;
            mi += ui;
          }
        }
        if (lane < C) {
          sM[lane] = mr;
          sM[C + lane] = mi;
        }
      }
    }
  };

  const int64_t oo = batch_off(g, b, g.bo);
  const int nchunks = (g.T + C - 1) / C;
  fetch(0);
  for (int c = 0; c < nchunks; ++c) {
    commit();
    __syncthreads();
    if (c + 1 < nchunks) fetch((c + 1) * C);

    // ---- phase A: wave 0 Re P, wave 1 Im P, wave 2 Re Q S, wave 3 Im Q S
    {
      const float* qrow = sQ + l31 * LQ;
      const bool imag = wid & 1, carry = wid >= 2;
      // Re P = [q_r | q_i] . [k_r | k_i],  Im P = [q_i | -q_r] . [k_r | k_i]
      // Re QS = [q_r | q_i] . [S_r ; -S_i],  Im QS = [q_r | q_i] . [S_i ; S_r]
      const float* a0 = !carry && imag ? qrow + DE : qrow;
      const float* a1 = !carry && imag ? qrow : qrow + DE;
      const float sa1 = !carry && imag ? -1.0f : 1.0f;
      const float* b0 = carry ? sS + (imag ? SV : 0) + l31 : sK + l31 * LQ;
      const float* b1 = carry ? sS + (imag ? 0 : SV) + l31 : sK + l31 * LQ + DE;
      const float sb1 = carry && !imag ? -1.0f : 1.0f;
      const f32x16 acc = chain<DE>(a0, a1, 1, sa1, b0, b1, carry ? LV : 1, sb1, lk);
      float* dst = (carry ? sO : sP) + (imag ? C * LP : 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2) + 4 * lk) * LP + l31] = acc[r];
    }
    __syncthreads();

    // ---- phase B: the weights.  Thread (t, j) owns P[t][j + 8 m] and Vw[t][j + 8 m]
    {
      const int t = threadIdx.x >> 3, j = threadIdx.x & 7;
      double mtr = 0.0, mti = 0.0;
      if constexpr (DECAY) {
        mtr = sM[t];
        mti = sM[C + t];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int s = j + 8 * m, at = t * LP + s;
        float pr = sP[at], pi = sP[C * LP + at];
        if (s > t) {
          pr = pi = 0.0f;
        } else if constexpr (DECAY) {
          const CF e = wexp(mtr - sM[s], mti - sM[C + s]);
          const float nr = pr * e.re - pi * e.im;
          pi = pr * e.im + pi * e.re;
          pr = nr;
        }
        sP[at] = pr;
        sP[C * LP + at] = pi;
      }
      float dr = 1.0f, di = 0.0f;     // what is left of step t's update at the end of the chunk
      if constexpr (DECAY) {
        const CF e = wexp(sM[C - 1] - mtr, sM[2 * C - 1] - mti);
        dr = e.re;
        di = e.im;
      }
      if (g.scale_in) {
        dr *= g.scale;
        di *= g.scale;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int col = j + 8 * m;
        const float xr = sV[t * LV + col], xi = sV[t * LV + SV + col];
        sVw[t * LV + col] = DECAY ? dr * xr - di * xi : dr * xr;
        sVw[t * LV + SV + col] = DECAY ? dr * xi + di * xr : dr * xi;
      }
      if constexpr (DECAY) {
        if (threadIdx.x < C) {
          const CF w = wexp(sM[threadIdx.x], sM[C + threadIdx.x]);
          sW[threadIdx.x] = w.re;
          sW[C + threadIdx.x] = w.im;
        }
      }
    }
    __syncthreads();

    // ---- phase C: jobs 0 .. NE - 1 are the row tiles of S, jobs NE and NE + 1 are Re O and Im O
#pragma unroll
    for (int jj = 0; jj < (NE + 2 + 3) / 4; ++jj) {
      const int job = wid + 4 * jj;
      if (job >= NE + 2) break;
      if (job < NE) {
        // Re += k_r^T Vw_r + k_i^T Vw_i,  Im += k_r^T Vw_i - k_i^T Vw_r
        const float *a0 = sK + 32 * job + l31, *a1 = a0 + DE;
        const f32x16 ar = chain<C>(a0, a1, LQ, 1.0f, sVw + l31, sVw + SV + l31, LV, 1.0f, lk);
        const f32x16 ai = chain<C>(a0, a1, LQ, 1.0f, sVw + SV + l31, sVw + l31, LV, -1.0f, lk);
        const float wr = DECAY ? sW[C - 1] : 1.0f, wi = DECAY ? sW[2 * C - 1] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int at = (32 * job + (r & 3) + 8 * (r >> 2) + 4 * lk) * LV + l31;
          const float sr = sS[at], si = sS[at + SV];
          sS[at] = (DECAY ? wr * sr - wi * si : sr) + ar[r];
          sS[at + SV] = (DECAY ? wr * si + wi * sr : si) + ai[r];
        }
      } else {
        // Re O = [P_r | P_i] . [v_r ; -v_i],  Im O = [P_r | P_i] . [v_i ; v_r];  then + w[t] (Q S)[t]
        const bool imag = job > NE;
        const float *a0 = sP + l31 * LP, *a1 = a0 + C * LP;
        const f32x16 acc = chain<C>(a0, a1, 1, 1.0f, sV + (imag ? SV : 0) + l31, sV + (imag ? 0 : SV) + l31, LV,
                                    imag ? 1.0f : -1.0f, lk);
        T* dst = reinterpret_cast<T*>(imag ? g.o_i : g.o_r) + oo + v0 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int t = (r & 3) + 8 * (r >> 2) + 4 * lk, p = c * C + t;
          const float xr = sO[t * LP + l31], xi = sO[C * LP + t * LP + l31];
          float carry = imag ? xi : xr;
          if constexpr (DECAY) {
            const float wr = sW[t], wi = sW[C + t];
            carry = imag ? wr * xi + wi * xr : wr * xr - wi * xi;
          }
          // (under SCALE_IN the carried state holds the factor already; this chunk's own updates do not)
          const float val = g.scale_in ? g.scale * acc[r] + carry : g.scale * (acc[r] + carry);
          if (p < g.T && v0 + l31 < g.Ev) io<T>::st(dst + (g.reverse ? (int64_t)g.T - 1 - p : (int64_t)p) * g.ro, val);
        }
      }
    }
    __syncthreads();                  // the next commit rewrites what these products read
  }

  // ---- the state after the last step, not rounded
  if (g.f_r) {
    const int64_t fo = batch_off(g, b, g.bf);
    for (int idx = threadIdx.x; idx < DE * 2 * SV; idx += 256) {
      const int e = idx / (2 * SV), rem = idx % (2 * SV), pl = rem / SV, col = rem % SV;
      if (e < g.E && v0 + col < g.Ev) (pl ? g.f_i : g.f_r)[fo + (int64_t)e * g.rf + v0 + col] = sS[e * LV + pl * SV + col];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
static int head_bucket(int64_t E) { return E <= 32 ? 32 : E <= 64 ? 64 : 128; }
static int lds_bytes(int de) { return de == 32 ? Lay<32>::LDS : de == 64 ? Lay<64>::LDS : Lay<128>::LDS; }
static bool sizes_ok(int64_t T, int64_t E, int64_t Ev) { return T >= 0 && E >= 1 && Ev >= 1 && E <= 128 && Ev <= 128; }

template <typename T, int DE, bool DECAY>
static int launch(const Args& g, int64_t grid, hipStream_t st) {
  static PerDeviceOnce once;
  constexpr int lds = Lay<DE>::LDS;
  if (const int rc = set_max_dyn_lds(once, linattn_kernel<T, DE, DECAY>, lds)) return rc;
  hipLaunchKernelGGL((linattn_kernel<T, DE, DECAY>), dim3((uint32_t)grid), dim3(256), lds, st, g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}
template <typename T, bool DECAY>
static int launch_head(const Args& g, int de, int64_t grid, hipStream_t st) {
  if (de == 32) return launch<T, 32, DECAY>(g, grid, st);
  if (de == 64) return launch<T, 64, DECAY>(g, grid, st);
  return launch<T, 128, DECAY>(g, grid, st);
}

}  // namespace la
}  // namespace cplxamd

using namespace cplxamd;

static_assert(sizeof(cplxamd_linattn_desc) == 280, "cplxamd_linattn_desc is 280 bytes");

extern "C" int cplxamd_linattn_plan(int64_t T, int64_t E, int64_t Ev, int64_t batch, int dtype, int64_t* plan) {
  if (!plan || batch < 0 || (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) || !la::sizes_ok(T, E, Ev)) return CPLXAMD_EINVAL;
  if (T > INT32_MAX - 2 * la::C) return CPLXAMD_ESHAPE;
  const int de = la::head_bucket(E);
  const int64_t slices = (Ev + la::SV - 1) / la::SV;
  int64_t grid;
  if (__builtin_mul_overflow(batch, slices, &grid) || grid > INT32_MAX) return CPLXAMD_ESHAPE;
  plan[CPLXAMD_LINATTN_CHUNK] = la::C;
  plan[CPLXAMD_LINATTN_HEAD_E] = de;
  plan[CPLXAMD_LINATTN_HEAD_V] = slices * la::SV;
  plan[CPLXAMD_LINATTN_SLICE] = la::SV;
  plan[CPLXAMD_LINATTN_SLICES] = slices;
  plan[CPLXAMD_LINATTN_CHUNKS] = (T + la::C - 1) / la::C;
  plan[CPLXAMD_LINATTN_GRID] = grid;
  plan[CPLXAMD_LINATTN_LDS_BYTES] = la::lds_bytes(de);
  plan[CPLXAMD_LINATTN_THREADS] = 256;
  return 0;
}

extern "C" int cplxamd_linattn(const void* q_r, const void* q_i, const void* k_r, const void* k_i, const void* v_r,
                               const void* v_i, const float* l_r, const float* l_i, const float* s_r, const float* s_i,
                               void* o_r, void* o_i, float* f_r, float* f_i, const cplxamd_linattn_desc* d, int dtype,
                               void* stream) {
  if (!q_r || !q_i || !k_r || !k_i || !v_r || !v_i || !o_r || !o_i || !d) return CPLXAMD_EINVAL;
  if ((l_i && !l_r) || (s_r != nullptr) != (s_i != nullptr) || (f_r != nullptr) != (f_i != nullptr)) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16) return CPLXAMD_EINVAL;
  if (!la::sizes_ok(d->T, d->E, d->Ev) || !std::isfinite(d->scale)) return CPLXAMD_EINVAL;
  if (d->flags & ~(CPLXAMD_LINATTN_REVERSE | CPLXAMD_LINATTN_CONJ | CPLXAMD_LINATTN_LAG | CPLXAMD_LINATTN_SCALE_IN))
    return CPLXAMD_EINVAL;
  if (d->q_rs < 0 || d->k_rs < 0 || d->v_rs < 0 || d->o_rs < d->Ev || d->s_rs < 0 || (f_r && d->f_rs < d->Ev)) return CPLXAMD_EINVAL;
  la::Args g{};
  using D = cplxamd_linattn_desc;
  const sp::RunStride<D> f[7] = {{&D::q_stride, g.bq}, {&D::k_stride, g.bk}, {&D::v_stride, g.bv}, {&D::l_stride, g.bl},
                                 {&D::s_stride, g.bs}, {&D::o_stride, g.bo}, {&D::f_stride, g.bf}};
  int64_t batch = 0, plan[CPLXAMD_LINATTN_PLAN_FIELDS];
  if (const int rc = sp::decode_runs(*d, f, g.size, batch)) return rc;
  if (const int rc = cplxamd_linattn_plan(d->T, d->E, d->Ev, batch, dtype, plan)) return rc;
  if (batch == 0 || d->T == 0) return 0;
  g.q_r = q_r; g.q_i = q_i; g.k_r = k_r; g.k_i = k_i; g.v_r = v_r; g.v_i = v_i;
  g.l_r = l_r; g.l_i = l_i; g.s_r = s_r; g.s_i = s_i;
  g.o_r = o_r; g.o_i = o_i; g.f_r = f_r; g.f_i = f_i;
  g.T = (int)d->T;
  g.E = (int)d->E;
  g.Ev = (int)d->Ev;
  g.slices = (int)plan[CPLXAMD_LINATTN_SLICES];
  g.reverse = (d->flags & CPLXAMD_LINATTN_REVERSE) != 0;
  g.conj = (d->flags & CPLXAMD_LINATTN_CONJ) != 0;
  g.lag = (d->flags & CPLXAMD_LINATTN_LAG) != 0;
  g.scale_in = (d->flags & CPLXAMD_LINATTN_SCALE_IN) != 0;
  g.scale = (float)d->scale;
  g.rq = d->q_rs; g.rk = d->k_rs; g.rv = d->v_rs; g.ro = d->o_rs; g.rs = d->s_rs; g.rf = d->f_rs;
  const int de = (int)plan[CPLXAMD_LINATTN_HEAD_E];
  const int64_t grid = plan[CPLXAMD_LINATTN_GRID];
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_BF16)
    return l_r ? la::launch_head<bf16_t, true>(g, de, grid, st) : la::launch_head<bf16_t, false>(g, de, grid, st);
  return l_r ? la::launch_head<float, true>(g, de, grid, st) : la::launch_head<float, false>(g, de, grid, st);
}
