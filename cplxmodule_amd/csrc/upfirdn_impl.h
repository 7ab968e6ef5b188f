// Rational rate change on direct-form polyphase kernels: the plan, the kernels and the checks of upfirdn.hip (which
// describes them) and upfirdn_wgrad.hip, as a header so that the two build side by side.  The batch runs are runs.h's;
// the weight gradient's chunking constants are fftconv_impl.h's.
#pragma once
#include "fftconv_impl.h"
#include "runs.h"

namespace cplxamd {
namespace sp {

constexpr int64_t kUpFusedK = 4096;                       // longer filters: composed from cplxamd_fftconv
constexpr int64_t kUpLdsBudget = 76 << 10;                // bytes per workgroup: two workgroups in a CU's 160 KiB
constexpr int kUpTileMax = 1024;                          // outputs per workgroup: four per thread
constexpr int kUpThreads = 256;
constexpr int kUpOut = kUpTileMax / kUpThreads;           // accumulators per thread
constexpr int kUpVecMax = 64;                             // packed rows per workgroup
constexpr int64_t kUpRateMax = 1ll << 30;                 // up, down
constexpr int64_t kUpLenMax = 1ll << 40;                  // operand lengths
constexpr int64_t kUpOffMax = 1ll << 48;                  // |off|: n down + off stays below 2^71 / 2^8 ... within 64 bits
constexpr int kUpWgradKb = 1024;                          // taps per workgroup of the weight gradient: four per thread
constexpr int kUpWgradAcc = kUpWgradKb / kUpThreads;

struct UpPlan {
  int path;
  int64_t T, tiles, vpw, span, phases, J, jseg, segs, lds, threads, grid;        // cplxamd_upfirdn
  int64_t Tn, wtiles, kb, kblocks, wspan, wlds, pairs, chunks, per_chunk, wbytes;   // cplxamd_upfirdn_wgrad
};

inline int64_t pad64(int64_t i) { return i + (i >> 4); }
inline int64_t halve64(int64_t t) { return t <= 128 ? (t > 64 ? 64 : t / 2) : ((t / 2 + 63) / 64) * 64; }

// words (of the compute type) of one tile's slice: the planes of a's span, then the planes of the filter segment
inline int64_t up_slice_words(int64_t span, int64_t taps, int xw, int hw) {
  return xw * (pad64(span) + 1) + hw * (pad64(taps) + 1);
}
inline int64_t up_span(int64_t T, int64_t up, int64_t down, int64_t jseg) { return ((T - 1) * down + up - 1) / up + jseg; }

// A: entries of a, K: taps, C: results (P1) / entries of c (P2)
inline int up_plan_for(int64_t A, int64_t K, int64_t C, int64_t up, int64_t down, int64_t off, int64_t rows, int64_t filters,
                       int dtype, int conj, int a_cplx, int b_cplx, UpPlan& p) {
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (A < 1 || K < 1 || C < 1 || up < 1 || down < 1 || rows < 0 || filters < 0 || (conj != 0 && conj != 1) ||
      (a_cplx != 0 && a_cplx != 1) || (b_cplx != 0 && b_cplx != 1))
    return CPLXAMD_EINVAL;
  if (up > kUpRateMax || down > kUpRateMax || A > kUpLenMax || C > kUpLenMax || K > kUpLenMax || off > kUpOffMax ||
      off < -kUpOffMax)
    return CPLXAMD_ESHAPE;
  p = UpPlan{};
  if (K > kUpFusedK) {
    p.path = CPLXAMD_UPFIRDN_COMPOSED;
    return 0;
  }
  p.path = CPLXAMD_UPFIRDN_FUSED;
  const int64_t word = dtype == CPLXAMD_F64 ? 8 : 4, cap = kUpLdsBudget / word;
  const int xw = a_cplx ? 2 : 1, hw = b_cplx ? 2 : 1;
  // ---- P1: the largest tile whose span and filter fit; the taps in segments only when 64 outputs do not fit; a tile
  // below 64 outputs only when one tap per phase does not fit either
  p.phases = up < K ? up : K;
  p.J = ceil_div(K, up);
  auto fits = [&](int64_t T, int64_t V, int64_t jseg) {
    return V * up_slice_words(up_span(T, up, down, jseg), p.phases * jseg, xw, hw) <= cap;
  };
  int64_t T = C < kUpTileMax ? C : kUpTileMax, jseg = p.J;
  while (T > 64 && !fits(T, 1, jseg)) T = halve64(T);
  if (!fits(T, 1, jseg)) {
    while (T > 1 && !fits(T, 1, 1)) T = halve64(T);
    int64_t lo = 1, hi = p.J;                            // the most taps per phase that fit
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (fits(T, 1, mid)) lo = mid; else hi = mid - 1;
    }
    jseg = lo;
  }
  if (!fits(T, 1, jseg)) return CPLXAMD_ESHAPE;          // (one output, one tap per phase: at most 4096 + 2 entries)
  p.T = T;
  p.jseg = jseg;
  p.segs = ceil_div(p.J, jseg);
  p.tiles = ceil_div(C, T);
  int64_t V = 1;
  if (p.tiles == 1) {                                     // short rows: several to a workgroup
    V = kUpTileMax / T;
    if (V > kUpVecMax) V = kUpVecMax;
    if (rows > 0 && V > rows) V = rows;
    while (V > 1 && !fits(T, V, jseg)) --V;
  }
  p.vpw = V;
  p.span = up_span(T, up, down, jseg);
  p.lds = V * up_slice_words(p.span, p.phases * jseg, xw, hw) * word;
  p.threads = ((T * V + 63) / 64) * 64;
  if (p.threads > kUpThreads) p.threads = kUpThreads;
  int64_t vecs;
  if (__builtin_mul_overflow(rows, p.tiles, &vecs)) return CPLXAMD_ESHAPE;
  p.grid = ceil_div(vecs, V);
  if (p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  // ---- P2: blocks of at most 1024 taps, tiles of c as long as they fit with the span of a they meet
  p.kb = K < kUpWgradKb ? K : kUpWgradKb;
  p.kblocks = ceil_div(K, p.kb);
  auto wspan = [&](int64_t Tn) { return ((Tn - 1) * down + p.kb - 1) / up + 2; };
  auto wfits = [&](int64_t Tn) { return xw * (pad64(wspan(Tn)) + 1) + hw * (pad64(Tn) + 1) <= cap; };
  int64_t Tn = C < kUpTileMax ? C : kUpTileMax;
  while (Tn > 1 && !wfits(Tn)) Tn = halve64(Tn);
  if (!wfits(Tn)) return CPLXAMD_ESHAPE;
  p.Tn = Tn;
  p.wtiles = ceil_div(C, Tn);
  p.wspan = wspan(Tn);
  p.wlds = (xw * (pad64(p.wspan) + 1) + hw * (pad64(Tn) + 1)) * word;
  const int64_t nf = filters > 0 ? filters : 1;
  if (__builtin_mul_overflow(rows / nf, p.wtiles, &p.pairs)) return CPLXAMD_ESHAPE;
  int64_t chunks = ceil_div(kConvWgs, nf * p.kblocks);
  int64_t one;                                            // bytes of one partial per result
  if (__builtin_mul_overflow(nf, K * 2 * word, &one) || one > kConvWsMax) return CPLXAMD_ESHAPE;
  const int64_t most = kLargeWs / one;
  if (chunks > most) chunks = most;
  if (chunks > p.pairs) chunks = p.pairs;
  if (chunks < 1) chunks = 1;
  p.per_chunk = ceil_div(p.pairs > 0 ? p.pairs : 1, chunks);
  p.chunks = ceil_div(p.pairs > 0 ? p.pairs : 1, p.per_chunk);
  p.wbytes = al256(one * p.chunks);
  int64_t wgs;
  if (__builtin_mul_overflow(nf * p.chunks, p.kblocks, &wgs) || wgs > 0x7fffffffll) return CPLXAMD_ESHAPE;
  return 0;
}

__host__ __device__ inline int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return q * b > a ? q - 1 : q;
}

// ---- P1 ---------------------------------------------------------------------------------------------------------------
template <typename TI>
struct UpIo {
  const TI* ar; const TI* ai; const TI* br; const TI* bi; TI* yr; TI* yi;
  int64_t A, K, C, up, down, off, a_es, b_es, tiles, total;
  Sub ay, b;                                              // (a, y) strides; b.p: the filter's
  int T, V, span, phases, J, jseg, segs;
  bool conj, small;                                       // small: T down + up < 2^31, 32-bit phase arithmetic
};

// Workgroup: V tiles of T outputs.  Tile u = vec - blockIdx V covers y[row][jt T .. jt T + T) with q = n down + off:
//   convolution  i0 = floor(q / up), p = q - i0 up:     y[n] = sum_j b[p + j up] a[i0 - j]
//   correlation  i0 = ceil(q / up),  p = i0 up - q:     y[n] = sum_j conj(b[p + j up]) a[i0 + j]
// over the j with p + j up < K.  Per segment of jseg values of j the slice of a tile holds a[ibase .. ibase + span) (zero
// outside the row; ibase = i0 of the tile's first output, minus the segment's last j / plus its first) and the filter's
// taps (j0 + j) up + p at pad(p jseg + j): the taps of a phase are contiguous.  Both are padded by one word per 16
// (pad()), which spreads the power-of-two strides of neighbouring lanes (jseg words between phases, down / up samples
// between outputs) over the banks; lanes that share a phase or a sample read one address (a broadcast).
template <typename TI, typename T, bool XC, bool HC>
__global__ __launch_bounds__(kUpThreads) void upfirdn_lds(UpIo<TI> g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int64_t s_ao[kUpVecMax], s_bo[kUpVecMax], s_yo[kUpVecMax], s_i0[kUpVecMax], s_c0[kUpVecMax];
  __shared__ int s_left[kUpVecMax];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int taps = g.phases * g.jseg;
  const int xplane = pad(g.span) + 1, hplane = pad(taps) + 1;
  const int slice = (XC ? 2 : 1) * xplane + (HC ? 2 : 1) * hplane;
  T* lds = (T*)smem;
  if (tid < g.V) {
    const int64_t vec = (int64_t)blockIdx.x * g.V + tid;
    int64_t ao = 0, yo = 0, bo = 0, unused, i0 = 0, c0 = 0;
    int left = 0;                                         // a partly filled last workgroup: zeros in, no stores
    if (vec < g.total) {
      const int64_t row = vec / g.tiles, jt = vec - row * g.tiles;
      sub_offsets(g.ay, row, ao, yo);
      sub_offsets(g.b, row, bo, unused);
      const int64_t n0 = jt * g.T, q0 = n0 * g.down + g.off;
      yo += n0;
      left = g.C - n0 < g.T ? (int)(g.C - n0) : g.T;
      if (!g.conj) {
        i0 = floor_div(q0, g.up);
        c0 = q0 - i0 * g.up;
      } else {
        i0 = -floor_div(-q0, g.up);
        c0 = g.up - 1 - (i0 * g.up - q0);
      }
    }
    s_ao[tid] = ao, s_bo[tid] = bo, s_yo[tid] = yo, s_i0[tid] = i0, s_c0[tid] = c0, s_left[tid] = left;
  }
  T acc_re[kUpOut], acc_im[kUpOut];
#pragma unroll
  for (int e = 0; e < kUpOut; ++e) acc_re[e] = acc_im[e] = 0;
  const T sg = g.conj ? (T)-1 : (T)1;
  for (int seg = 0; seg < g.segs; ++seg) {
    const int j0 = seg * g.jseg;
    __syncthreads();                                      // the tiles' offsets; the previous segment's reads
    for (int u = 0; u < g.V; ++u) {
      T* xre = lds + u * slice;
      T* xim = xre + xplane;
      T* hre = xre + (XC ? 2 : 1) * xplane;
      T* him = hre + hplane;
      const bool ok = s_left[u] > 0;
      const int64_t ibase = g.conj ? s_i0[u] + j0 : s_i0[u] - (j0 + g.jseg - 1), ao = s_ao[u], bo = s_bo[u];
      for (int s = tid; s < g.span; s += nt) {
        const int64_t i = ibase + s;
        const bool in = ok && i >= 0 && i < g.A;          // zeros are never read
        xre[pad(s)] = in ? (T)ld<TI>::at(g.ar + ao + i * g.a_es) : (T)0;
        if constexpr (XC) xim[pad(s)] = in ? (T)ld<TI>::at(g.ai + ao + i * g.a_es) : (T)0;
      }
      for (int e = tid; e < taps; e += nt) {
        const int j = e / g.phases, ph = e - j * g.phases;
        const int64_t k = (int64_t)(j0 + j) * g.up + ph;
        const bool in = ok && k < g.K;
        const int at = pad(ph * g.jseg + j);
        hre[at] = in ? (T)ld<TI>::at(g.br + bo + k * g.b_es) : (T)0;
        if constexpr (HC) him[at] = in ? sg * (T)ld<TI>::at(g.bi + bo + k * g.b_es) : (T)0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kUpOut; ++e) {
      const int o = tid + e * nt;
      if (o >= g.V * g.T) continue;
      const int u = o / g.T, m = o - u * g.T;
      if (m >= s_left[u]) continue;
      int64_t di, rem;
      if (g.small) {
        const uint32_t t = (uint32_t)m * (uint32_t)g.down + (uint32_t)s_c0[u];
        di = t / (uint32_t)g.up;
        rem = t - (uint32_t)di * (uint32_t)g.up;
      } else {
        const uint64_t t = (uint64_t)m * (uint64_t)g.down + (uint64_t)s_c0[u];
        di = (int64_t)(t / (uint64_t)g.up);
        rem = (int64_t)(t - (uint64_t)di * (uint64_t)g.up);
      }
      const int64_t ph = g.conj ? g.up - 1 - rem : rem;
      if (ph >= g.K) continue;                            // no tap lands on this output
      const int jp = (int)((g.K - ph + g.up - 1) / g.up);     // taps of this phase (ph < 4096 here)
      const int jhi = j0 + g.jseg < jp ? j0 + g.jseg : jp;
      const T* xre = lds + u * slice;
      const T* xim = xre + xplane;
      const T* hre = xre + (XC ? 2 : 1) * xplane;
      const T* him = hre + hplane;
      const int hb = (int)ph * g.jseg - j0;
      // a's index: (di + jseg - 1 + j0) - j for the convolution, (di - j0) + j for the correlation
      int sx = g.conj ? (int)di : (int)di + g.jseg - 1;
      const int dx = g.conj ? 1 : -1;
      T re = acc_re[e], im = acc_im[e];
      for (int j = j0; j < jhi; ++j, sx += dx) {
        const T hr = hre[pad(hb + j)], xr = xre[pad(sx)];
        if constexpr (XC && HC) {
          const T hi = him[pad(hb + j)], xi = xim[pad(sx)];   // hi carries the correlation's sign
          re += hr * xr - hi * xi;
          im += hr * xi + hi * xr;
        } else if constexpr (XC) {
          re += hr * xr;
          im += hr * xim[pad(sx)];
        } else if constexpr (HC) {
          re += hr * xr;
          im += him[pad(hb + j)] * xr;
        } else {
          re += hr * xr;
        }
      }
      acc_re[e] = re, acc_im[e] = im;
    }
  }
#pragma unroll
  for (int e = 0; e < kUpOut; ++e) {
    const int o = tid + e * nt;
    if (o >= g.V * g.T) continue;
    const int u = o / g.T, m = o - u * g.T;
    if (m >= s_left[u]) continue;
    st_t(g.yr + s_yo[u] + m, acc_re[e]);
    if (g.yi) st_t(g.yi + s_yo[u] + m, acc_im[e]);        // a null plane is not stored
  }
}

// ---- P2 ---------------------------------------------------------------------------------------------------------------
template <typename TI>
struct UpWgradIo {
  const TI* ar; const TI* ai; const TI* cr; const TI* ci;
  int64_t A, K, C, up, down, off, a_es, c_es, wtiles, pairs, per_chunk, chunks;
  int64_t g, upg, downg, inv;                             // gcd(up, down), up / g, down / g, (down / g)^-1 mod up / g
  Sub kept, red;                                          // (a, c) strides of the result's runs and of the reduced runs
  int Tn, span, kb, kblocks;
};

// workgroup (f, chunk, kb): part[f][chunk][k] for its block of taps = sum over the chunk's (reduced row, tile) pairs,
// ascending, and over the tile's n, ascending, of conj(a[i]) c[n] where i up = n down + off - k.  For a tap k those n are
// one residue class modulo up / g (none unless g divides k - off): thread k finds it once, then steps n by up / g and i by
// down / g through the staged tile of c and span of a.
template <typename TI, typename T, bool AC, bool CC>
__global__ __launch_bounds__(kUpThreads) void upfirdn_wgrad_part(UpWgradIo<TI> g, C2<T>* part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int aplane = pad(g.span) + 1, cplane = pad(g.Tn) + 1;
  T* are = (T*)smem;
  T* aim = are + aplane;
  T* cre = are + (AC ? 2 : 1) * aplane;
  T* cim = cre + cplane;
  const int64_t kbi = blockIdx.x % g.kblocks, fc = blockIdx.x / g.kblocks, f = fc / g.chunks, ch = fc - f * g.chunks;
  const int64_t k0 = kbi * g.kb, k1 = k0 + g.kb < g.K ? k0 + g.kb : g.K;   // this workgroup's taps [k0, k1)
  int64_t a0, c0;
  sub_offsets(g.kept, f, a0, c0);
  // per tap: nk = the residue of its n modulo up / g, ik = the i of n = nk
  bool live[kUpWgradAcc];
  int64_t nk[kUpWgradAcc], ik[kUpWgradAcc];
  T acc_re[kUpWgradAcc], acc_im[kUpWgradAcc];
#pragma unroll
  for (int e = 0; e < kUpWgradAcc; ++e) {
    const int64_t k = k0 + tid + e * kUpThreads;
    acc_re[e] = acc_im[e] = 0;
    nk[e] = ik[e] = 0;
    live[e] = false;
    if (k < k1) {
      const int64_t r = k - g.off, rq = floor_div(r, g.g);
      if (rq * g.g == r) {
        const int64_t rm = rq - floor_div(rq, g.upg) * g.upg;
        nk[e] = (rm * g.inv) % g.upg;
        ik[e] = (nk[e] * g.down - r) / g.up;              // exact
        live[e] = true;
      }
    }
  }
  const int64_t q0 = ch * g.per_chunk, q1 = q0 + g.per_chunk < g.pairs ? q0 + g.per_chunk : g.pairs;
  for (int64_t q = q0; q < q1; ++q) {                     // the same range for every thread: the barriers are uniform
    const int64_t rr = q / g.wtiles, jt = q - rr * g.wtiles;
    int64_t ao, co;
    sub_offsets(g.red, rr, ao, co);
    ao += a0;
    co += c0;
    const int64_t n_lo = jt * g.Tn;
    const int cnt = g.C - n_lo < g.Tn ? (int)(g.C - n_lo) : g.Tn;
    // the least i any (n, k) of this tile and block meets: ceil((n_lo down + off - (k1 - 1)) / up)
    const int64_t ibase = -floor_div(-(n_lo * g.down + g.off - (k1 - 1)), g.up);
    if (q > q0) __syncthreads();
    for (int s = tid; s < g.span; s += kUpThreads) {
      const int64_t i = ibase + s;
      const bool in = i >= 0 && i < g.A;
      are[pad(s)] = in ? (T)ld<TI>::at(g.ar + ao + i * g.a_es) : (T)0;
      if constexpr (AC) aim[pad(s)] = in ? (T)ld<TI>::at(g.ai + ao + i * g.a_es) : (T)0;
    }
    for (int m = tid; m < g.Tn; m += kUpThreads) {
      const bool in = m < cnt;
      cre[pad(m)] = in ? (T)ld<TI>::at(g.cr + co + (n_lo + m) * g.c_es) : (T)0;
      if constexpr (CC) cim[pad(m)] = in ? (T)ld<TI>::at(g.ci + co + (n_lo + m) * g.c_es) : (T)0;
    }
    __syncthreads();
    const int64_t nq = n_lo / g.upg, nr = n_lo - nq * g.upg;
#pragma unroll
    for (int e = 0; e < kUpWgradAcc; ++e) {
      if (!live[e]) continue;
      const int64_t z = nq + (nk[e] < nr ? 1 : 0);        // the first n >= n_lo of the class: z up / g + nk
      const int64_t m0 = z * g.upg + nk[e] - n_lo, s0 = ik[e] + z * g.downg - ibase;
      if (m0 >= cnt) continue;
      T re = acc_re[e], im = acc_im[e];
      int s = (int)s0;
      for (int64_t m = m0; m < cnt; m += g.upg, s += (int)g.downg) {
        const T xr = are[pad(s)], yr = cre[pad((int)m)];
        if constexpr (AC && CC) {
          const T xi = aim[pad(s)], yi = cim[pad((int)m)];
          re += xr * yr + xi * yi;
          im += xr * yi - xi * yr;
        } else if constexpr (AC) {
          re += xr * yr;
          im -= aim[pad(s)] * yr;
        } else if constexpr (CC) {
          re += xr * yr;
          im += xr * cim[pad((int)m)];
        } else {
          re += xr * yr;
        }
      }
      acc_re[e] = re, acc_im[e] = im;
    }
  }
  C2<T>* dst = part + fc * g.K;
#pragma unroll
  for (int e = 0; e < kUpWgradAcc; ++e) {
    const int64_t k = k0 + tid + e * kUpThreads;
    if (k < k1) dst[k] = {acc_re[e], acc_im[e]};
  }
}

// y[f][k] = sum over chunks, ascending, of part[f][chunk][k], rounded once: one thread per entry
template <typename TO, typename T>
__global__ __launch_bounds__(kET) void upfirdn_wgrad_finish(const C2<T>* part, int64_t filters, int64_t chunks, int64_t K,
                                                             TO* yr, TO* yi, Sub ys) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < filters * K; i += (int64_t)gridDim.x * kET) {
    const int64_t f = i / K, k = i - f * K;
    const C2<T>* src = part + f * chunks * K + k;
    C2<T> s = src[0];
    for (int64_t c = 1; c < chunks; ++c) s = {s.re + src[c * K].re, s.im + src[c * K].im};
    int64_t yo, unused;
    sub_offsets(ys, f, yo, unused);
    st_t(yr + yo + k, s.re);
    if (yi) st_t(yi + yo + k, s.im);
  }
}

// the checks both launchers share; the plan of the call
inline int up_check(const void* a_r, const void* a_i, const void* b_r, const void* b_i, const void* y_r,
                    const cplxamd_upfirdn_desc* d, int dtype, bool wgrad, ConvRuns& r, int64_t& filters, int (&kept)[3],
                    UpPlan& p) {
  if (!a_r || !b_r || !y_r || !d) return CPLXAMD_EINVAL;
  if (d->a_es < 0 || d->b_es < 0 || (wgrad && d->conj != 0)) return CPLXAMD_EINVAL;
  using D = cplxamd_upfirdn_desc;
  const RunStride<D> f[] = {{&D::a_stride, r.as}, {&D::b_stride, r.bs}, {&D::y_stride, r.ys}};
  if (const int e = decode_runs(*d, f, r.size, r.rows)) return e;
  filters = select_runs(r, wgrad ? r.ys : r.bs, true, kept);
  if (const int e = up_plan_for(d->a_len, d->k, d->c_len, d->up, d->down, d->off, r.rows, filters, dtype, d->conj,
                                a_i != nullptr, b_i != nullptr, p))
    return e;
  if (p.path != CPLXAMD_UPFIRDN_FUSED) return CPLXAMD_EINVAL;
  return 0;
}

}  // namespace sp
}  // namespace cplxamd
