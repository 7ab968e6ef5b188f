// The polyphase filter bank along the last dim (cplx.pfb_analysis, cplx.pfb_synthesis: cplxmodule_amd/pfb.py; DESIGN
// section 28): M channels (a power of two up to 4096), K = P M real taps, a frame every `hop` samples, the phase referred
// to the start of the frame.
//   analysis    y[f][k] = sum_{n < K} h[n] x[f hop + n] e^{-2 pi i k n / M} = FFT_M(u[f])[k],
//               u[f][r] = sum_{p < P} h[p M + r] x[f hop + p M + r]
//   synthesis   o[t] = sum_{f ascending} g[t - f hop] v[f][(t - f hop) mod M],   v[f] = M IFFT_M(y[f])
// One kernel, pfb_tile, serves both: a workgroup owns a tile of FT consecutive frames of one row and runs the engine's
// fft_run on V of them at a time (V = kVecs: 256 threads hold 256 / kNT frames up to 1024 points, one frame above), so the
// twiddle table -- built in LDS by the workgroup itself, the entries of fft_engine.h's `tables` -- is paid once per tile
// and the call needs no workspace.  What differs is the loader and the store:
//   STAGED   the tile's (FT - 1) hop + K samples go through LDS once, as float32, one plane behind the other; the loader
//            forms u[f][r] from there.  A stage's lanes hold consecutive r, so the P reads of a lane are P conflict-free
//            rows; the taps h[p M + r] are coalesced reads of a table that stays in L1.  u is never stored.
//   DIRECT   the span does not fit beside the transform (160 KiB): the same sum over global memory, P loads per point,
//            coalesced along r; neighbouring frames overlap in L2.
//   INVERSE  (synthesis) the loader reads y[f][k] where it lies, the store writes v[f] as float32 into the workspace.
// The spectrum leaves the registers in the engine's own order: a thread's values are M / 8 apart, so the widest store
// the layout allows is one word per lane, consecutive lanes on consecutive channels (whole lines per wave).
// The synthesis gather, pfb_overlap_add, sums the at most ceil(K / hop) frames that cover an output sample in ascending
// order: no atomics, the same bits on every run.  pfb_plan_for is the pure host function behind cplxamd_pfb_plan.
#include "fft_engine.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

constexpr int kPfbLogMax = 12;                            // 4096 channels: 8 values per thread, at most 512 threads
constexpr int kPfbLdsWords = 160 * 1024 / 4;              // a CU's LDS
constexpr int kPfbSpanWords = 12 * 1024;                  // the span a tile aims at: 48 KiB, three workgroups per CU
constexpr int kPfbDirectFrames = 64;                      // frames per tile where nothing is staged
constexpr int64_t kPfbWantWgs = 1024;                     // tiles shrink until the grid has this many workgroups

enum { kStaged = 0, kDirect = 1, kInverse = 2 };

template <int LOGM> constexpr int kPfbV = LOGM <= kLogPackMax ? kVecs<LOGM> : 1;
template <int LOGM> constexpr int kPfbFftWords = kPfbV<LOGM> > 1 ? kPfbV<LOGM> * kSlice<LOGM> : 2 * (pad(1 << LOGM) + 1);
template <int LOGM> constexpr int kPfbTwWords = LOGM > 3 ? 2 << LOGM : 0;   // up to 8 points no twiddle is read

struct PfbPlan {
  bool staged;
  int logM, V, threads, lds;
  int64_t ft, tiles, grid, span, ws;
};

struct PfbArgs {
  const void* xr; const void* xi;                         // the input planes (xi may be null: zeros, never read)
  const float* h;
  void* yr; void* yi;                                     // the result [rows][frames][M], dense (yi null: not stored)
  Batch b;                                                // the rows: b.xs their strides in the input
  int64_t frames, ft, tiles, es, fs, span;                // es: stride of a sample / channel, fs: of a frame (inverse)
  int hop, P;
};

// ---- the tile kernel ---------------------------------------------------------------------------------------------------
template <typename TI, typename TO, int LOGM, int MODE>
__global__ __launch_bounds__(kPfbV<LOGM> * kNT<LOGM>) void pfb_tile(PfbArgs a) {
  constexpr int M = 1 << LOGM, NT = kNT<LOGM>, V = kPfbV<LOGM>, E = kEOf<LOGM>, THREADS = V * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* base = (float*)smem;
  C2<float>* tw = (C2<float>*)(base + kPfbFftWords<LOGM>);
  float* sr = base + kPfbFftWords<LOGM> + kPfbTwWords<LOGM>;
  float* si = sr + a.span;
  const int u = V == 1 ? 0 : threadIdx.x / NT;
  const int t = V == 1 ? threadIdx.x : threadIdx.x % NT;
  float* sre = base + (V == 1 ? 0 : u * kSlice<LOGM>);
  float* sim = sre + pad(M) + 1;
  const int64_t row = blockIdx.x / a.tiles, f0 = (blockIdx.x % a.tiles) * a.ft;
  const int nf = (int)(a.frames - f0 < a.ft ? a.frames - f0 : a.ft);
  int64_t xo, yo;
  batch_offsets(a.b, row, xo, yo);
  const TI* xr = (const TI*)a.xr + xo;
  const TI* xi = a.xi ? (const TI*)a.xi + xo : nullptr;
  if constexpr (LOGM > 3)
    for (int q = threadIdx.x; q < M; q += THREADS) tw[q] = cis<float>(-1.0f, q, M);
  if constexpr (MODE == kStaged) {
    const int span = (nf - 1) * a.hop + a.P * M;           // <= a.span, and f0 hop + span <= the row's length
    const int64_t s0 = f0 * a.hop;
    for (int i = threadIdx.x; i < span; i += THREADS) {
      sr[i] = ld<TI>::at(xr + (s0 + i) * a.es);
      if (xi) si[i] = ld<TI>::at(xi + (s0 + i) * a.es);
    }
  }
  __syncthreads();
  for (int g0 = 0; g0 < nf; g0 += V) {                    // nf is the workgroup's: every thread runs every stage
    const int fl = g0 + u;
    const bool ok = fl < nf;
    C2<float> v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = {0, 0};
    auto load = [&](int p) -> C2<float> {
      C2<float> s{0, 0};
      if (!ok) return s;
      if constexpr (MODE == kStaged) {
        const float* cr = sr + fl * a.hop + p;
        const float* ci = si + fl * a.hop + p;
        for (int q = 0; q < a.P; ++q) {
          const float w = a.h[q * M + p];
          s.re += w * cr[q * M];
          if (xi) s.im += w * ci[q * M];
        }
      } else if constexpr (MODE == kDirect) {
        const int64_t j = (f0 + fl) * a.hop + p;
        for (int q = 0; q < a.P; ++q) {
          const float w = a.h[q * M + p];
          const int64_t o = (j + q * M) * a.es;
          s.re += w * ld<TI>::at(xr + o);
          if (xi) s.im += w * ld<TI>::at(xi + o);
        }
      } else {
        const int64_t o = (f0 + fl) * a.fs + p * a.es;
        s.re = ld<TI>::at(xr + o);
        if (xi) s.im = ld<TI>::at(xi + o);
      }
      return s;
    };
    fft_run<float, LOGM>(v, sre, sim, t, MODE == kInverse ? 1.0f : -1.0f, tw, LOGM, load);
    if (ok) {
      const int64_t o = (row * a.frames + f0 + fl) * M;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        int k;
        if (out_k<LOGM>(e, t, k)) {
          st_t((TO*)a.yr + o + k, v[e].re);
          if (a.yi) st_t((TO*)a.yi + o + k, v[e].im);
        }
      }
    }
  }
}

// o[row][t] = sum_{f ascending, 0 <= t - f hop < K} g[t - f hop] v[row][f][(t - f hop) mod M], rounded once; a null o_i
// (and vi) is the real plane only
template <typename TO>
__global__ __launch_bounds__(kET) void pfb_overlap_add(const float* vr, const float* vi, const float* g, TO* o_r, TO* o_i,
                                                      int64_t rows, int64_t frames, int64_t M, int64_t K, int64_t hop,
                                                      int64_t length) {
  for (int64_t i = (int64_t)blockIdx.x * kET + threadIdx.x; i < rows * length; i += (int64_t)gridDim.x * kET) {
    const int64_t row = i / length, t = i - row * length;
    int64_t f = t >= K ? (t - K) / hop + 1 : 0;
    const int64_t f1 = t / hop < frames - 1 ? t / hop : frames - 1;
    float re = 0, im = 0;
    for (; f <= f1; ++f) {
      const int64_t n = t - f * hop, o = (row * frames + f) * M + (n & (M - 1));
      re += g[n] * vr[o];
      if (o_i) im += g[n] * vi[o];
    }
    st_t(o_r + i, re);
    if (o_i) st_t(o_i + i, im);
  }
}

// ---- plan --------------------------------------------------------------------------------------------------------------
// every field of a descriptor; `analysis`: the frames must lie inside the signal
int pfb_check(const cplxamd_pfb_desc& d, bool analysis) {
  const int64_t M = d.channels;
  if (M < 2 || M > (1 << kPfbLogMax) || (M & (M - 1)) || d.taps < 1 || d.taps > 64 || d.hop < 1 || d.hop > d.taps * M ||
      d.frames < 0 || d.frames > 0x7fffffffll || d.length < 0 || d.length > (1ll << 48) || d.sig_es < 0 || d.spec_fs < 0 ||
      d.spec_es < 0 || d.flags != 0)
    return CPLXAMD_EINVAL;
  if (analysis && d.frames > 0 && (d.frames - 1) * d.hop + d.taps * M > d.length) return CPLXAMD_EINVAL;
  return 0;
}

// the rows of a descriptor: the input's strides into b.xs (`analysis`: the signal's, else the spectrum's); the result is
// dense, b.ys stays zero
int pfb_rows(const cplxamd_pfb_desc& d, bool analysis, Batch& b) {
  using D = cplxamd_pfb_desc;
  int64_t size[3];
  b = Batch{};
  const RunStride<D> f[] = {{analysis ? &D::sig_stride : &D::spec_stride, b.xs}};
  if (const int e = decode_runs(d, f, size, b.total)) return e;
  b.s1 = size[1] > 0 ? size[1] : 1;
  b.s2 = size[2] > 0 ? size[2] : 1;
  return 0;
}

// `staging`: the analysis, which may stage its span; the synthesis transform takes the direct plan's tiles
int pfb_plan_for(const cplxamd_pfb_desc& d, int64_t rows, bool cplx, bool staging, PfbPlan& p) {
  const int64_t M = d.channels, K = d.taps * M, F = d.frames, planes = cplx ? 2 : 1;
  p.logM = 63 - __builtin_clzll((unsigned long long)M);
  const int64_t nt = M / 8 > 0 ? M / 8 : 1;
  const int64_t V = p.logM <= kLogPackMax ? kPackT / nt : 1;
  p.V = (int)V;
  p.threads = (int)(V * nt);
  const int64_t slice = 2 * (pad((int)M) + 1);
  const int64_t fixed = (V > 1 ? V * (slice + 1) : slice) + (p.logM > 3 ? 2 * M : 0);
  const int64_t room = (kPfbLdsWords - fixed) / planes;   // words per plane beside the transform
  p.staged = staging && (V - 1) * d.hop + K <= room;
  int64_t ft;
  if (p.staged) {
    const int64_t fit = ((room - K) / d.hop + 1) / V * V;
    const int64_t aim = kPfbSpanWords / planes >= K ? ((kPfbSpanWords / planes - K) / d.hop + 1) / V * V : 0;
    ft = aim < V ? V : aim;
    // a tile that takes more than half a CU's LDS is alone on its CU whatever its size: then as many frames as fit, for
    // the fewest reads of the overlap between tiles
    if (ft > fit || 2 * (fixed + planes * ((ft - 1) * d.hop + K)) > kPfbLdsWords) ft = fit;
  } else {
    ft = kPfbDirectFrames / V * V;
    if (ft < V) ft = V;
  }
  const int64_t whole = ceil_div(F > 0 ? F : 1, V) * V;    // no more than the row has
  if (ft > whole) ft = whole;
  const int64_t need = ceil_div(kPfbWantWgs, rows > 0 ? rows : 1);
  if (need > 1) {                                         // few rows: smaller tiles, down to one pass
    int64_t cap = F / need / V * V;
    if (cap < V) cap = V;
    if (ft > cap) ft = cap;
  }
  p.ft = ft;
  p.tiles = ceil_div(F, ft);
  if (__builtin_mul_overflow(rows, p.tiles, &p.grid) || p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  p.span = p.staged ? (ft - 1) * d.hop + K : 0;
  p.lds = (int)(4 * (fixed + planes * p.span));
  int64_t ws;
  if (__builtin_mul_overflow(rows, F, &ws) || __builtin_mul_overflow(ws, M * 4 * planes, &ws)) return CPLXAMD_ESHAPE;
  p.ws = ws;
  return 0;
}

// ---- launch ------------------------------------------------------------------------------------------------------------
template <typename TI, typename TO, int MODE>
int pfb_launch(const PfbArgs& a, const PfbPlan& p, hipStream_t st) {
  return with_log<1, kPfbLogMax>(p.logM, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    static PerDeviceOnce once;
    if (const int e = set_max_dyn_lds(once, pfb_tile<TI, TO, LG, MODE>, kPfbLdsWords * 4)) return e;
    pfb_tile<TI, TO, LG, MODE><<<(unsigned)p.grid, kPfbV<LG> * kNT<LG>, p.lds, st>>>(a);
    CPLXAMD_CHECK_LAUNCH();
    return 0;
  });
}

template <typename TI>
int pfb_analysis_t(PfbArgs& a, const PfbPlan& p, hipStream_t st) {
  return p.staged ? pfb_launch<TI, TI, kStaged>(a, p, st) : pfb_launch<TI, TI, kDirect>(a, p, st);
}

template <typename TI>
int pfb_synthesis_t(PfbArgs& a, const PfbPlan& p, const cplxamd_pfb_desc& d, const float* g, void* o_r, void* o_i,
                    hipStream_t st) {
  const int64_t rows = a.b.total;
  if (p.grid > 0)
    if (const int e = pfb_launch<TI, float, kInverse>(a, p, st)) return e;
  if (rows * d.length == 0) return 0;
  pfb_overlap_add<TI><<<ew_grid(rows * d.length), kET, 0, st>>>((const float*)a.yr, (const float*)a.yi, g, (TI*)o_r, (TI*)o_i,
                                                               rows, d.frames, d.channels, d.taps * d.channels, d.hop,
                                                               d.length);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int cplxamd_pfb_plan(const cplxamd_pfb_desc* d, int cplx, int64_t* out) {
  if (!d || !out || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (const int e = pfb_check(*d, false)) return e;
  Batch b;
  if (const int e = pfb_rows(*d, true, b)) return e;
  PfbPlan p;
  if (const int e = pfb_plan_for(*d, b.total, cplx != 0, true, p)) return e;
  out[CPLXAMD_PFB_FRAMES_PER_TILE] = p.ft;
  out[CPLXAMD_PFB_TILES] = p.tiles;
  out[CPLXAMD_PFB_VECTORS] = p.V;
  out[CPLXAMD_PFB_SPAN] = p.span;
  out[CPLXAMD_PFB_LDS_BYTES] = p.lds;
  out[CPLXAMD_PFB_THREADS] = p.threads;
  out[CPLXAMD_PFB_GRID] = p.grid;
  out[CPLXAMD_PFB_WS_BYTES] = p.ws;
  return p.staged ? CPLXAMD_PFB_STAGED : CPLXAMD_PFB_DIRECT;
}

int cplxamd_pfb_analysis(const void* x_r, const void* x_i, const void* h, void* y_r, void* y_i, const cplxamd_pfb_desc* d,
                         int dtype, void* stream) {
  if (!x_r || !h || !y_r || !y_i || !d || (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16)) return CPLXAMD_EINVAL;
  if (const int e = pfb_check(*d, true)) return e;
  PfbArgs a{x_r, x_i, (const float*)h, y_r, y_i, {}, d->frames, 0, 0, d->sig_es, 0, 0, (int)d->hop, (int)d->taps};
  if (const int e = pfb_rows(*d, true, a.b)) return e;
  PfbPlan p;
  if (const int e = pfb_plan_for(*d, a.b.total, x_i != nullptr, true, p)) return e;
  if (p.grid == 0) return 0;
  a.ft = p.ft;
  a.tiles = p.tiles;
  a.span = p.span;
  hipStream_t st = (hipStream_t)stream;
  return dtype == CPLXAMD_BF16 ? pfb_analysis_t<bf16_t>(a, p, st) : pfb_analysis_t<float>(a, p, st);
}

int cplxamd_pfb_synthesis(const void* y_r, const void* y_i, const void* g, void* o_r, void* o_i, const cplxamd_pfb_desc* d,
                          int dtype, void* ws, int64_t ws_bytes, void* stream) {
  if (!y_r || !g || !o_r || !d || (dtype != CPLXAMD_F32 && dtype != CPLXAMD_BF16)) return CPLXAMD_EINVAL;
  if (const int e = pfb_check(*d, false)) return e;
  PfbArgs a{y_r, y_i, nullptr, nullptr, nullptr, {}, d->frames, 0, 0, d->spec_es, d->spec_fs, 0, (int)d->hop, (int)d->taps};
  if (const int e = pfb_rows(*d, false, a.b)) return e;
  PfbPlan p;
  if (const int e = pfb_plan_for(*d, a.b.total, o_i != nullptr, false, p)) return e;
  if (p.ws > 0 && (!ws || ws_bytes < p.ws)) return CPLXAMD_EWS;
  a.ft = p.ft;
  a.tiles = p.tiles;
  a.yr = ws;                                              // v: the real plane, then (two planes) the imaginary one
  a.yi = o_i ? (float*)ws + a.b.total * d->frames * d->channels : nullptr;
  hipStream_t st = (hipStream_t)stream;
  return dtype == CPLXAMD_BF16 ? pfb_synthesis_t<bf16_t>(a, p, *d, (const float*)g, o_r, o_i, st)
                               : pfb_synthesis_t<float>(a, p, *d, (const float*)g, o_r, o_i, st);
}

}  // extern "C"
