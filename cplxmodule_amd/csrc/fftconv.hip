// Linear convolution and correlation along the last dim by overlap-save on the engine of fft_engine.h
// (cplx.fftconvolve: cplxmodule_amd/fftconv.py).  Two primitives over rows of up to three batch runs, each the other's
// gradient:
//   P1  y[r][n] = sum_m a[r][n + start - m] b[r][m]            (conj: sum_m a[r][n + start + m] conj(b[r][m])),  n < c_len
//   P2  y[f][m] = sum_{rows of f} sum_n conj(a[r][n]) c[r][n + m + start],  m < k        (fftconv_wgrad.hip)
// with a (and c) reading as zero outside their rows.  The filter b has k <= 4096 taps.
//
// P1 is one launch of fftconv_lds after the filter spectra.  A block of L = 2^LOGL points is what fft_lds's Bluestein
// branch does between its chirps: load, forward transform, product with a table, to_lds, inverse transform, store -- a
// cyclic convolution of L points inside one workgroup's LDS, no round trip through memory.  Overlap-save makes it linear:
// with S = L - k + 1, block j of a row loads a[j S + in_shift + i], i < L (predicated on the row: zeros and a null
// imaginary plane are never read), and of its L cyclic results the S that no wrap-around touches are stored,
// y[j S + n] with n = (i - out_lo) mod L < S:
//     convolution   in_shift = start - (k - 1), out_lo = k - 1   (the first k - 1 entries of a block are the overlap)
//     correlation   in_shift = start,           out_lo = 0       (the last k - 1 are), times conj(H-hat)
// so one kernel serves both, and a gradient never flips or conjugates an operand in a pass of its own.  When L holds
// every product (L >= a_len + k - 1 and the window lies inside), ONE block per row loads the row at in_shift = 0 and the
// cyclic result is the linear one: lag q at entry q mod L (negative lags of a correlation wrap to the top), out_lo =
// start mod L.  The plan (conv_plan_for in fftconv_impl.h) gives L, S, the blocks per row and these offsets.
// Packing is fft_lds's: V = 2048 / L blocks (256 below 8 points) per 256-thread workgroup up to L = 1024, each in its
// odd-word LDS slice, one block per workgroup of kNT<LOGL> threads for 2^11 .. 2^13.  A workgroup's blocks are
// consecutive along a row and continue into the next row (block -> (row, j) is one division per block); a partly filled
// last workgroup loads zeros, runs every stage and skips the stores: nothing returns early before a barrier.
// H-hat[f] = FFT_L(b[f], zero-padded) / L per DISTINCT filter (runs whose b stride is 0 share one) comes from the
// transform kernel fft_lds itself with n_in = k and a loader policy for the taps' strides, into the caller's workspace
// next to the twiddles; rows find theirs through a filter-index stride per run.  float32 for bf16 planes.
// No atomics, no state in the library, nothing read on the host.  No kernel uses scratch
// (-Rpass-analysis=kernel-resource-usage; DESIGN section 20 has the table).
#include "fftconv_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI, typename T>
int fftconv_t(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
              const cplxamd_fftconv_desc& d, const ConvRuns& r, int64_t filters, const int (&kept)[3], const ConvPlan& p,
              int dtype, char* ws, hipStream_t st) {
  C2<T>* tw = (C2<T>*)(ws + p.off_tw);
  C2<T>* H = (C2<T>*)(ws + p.off_h);
  if (p.logL > 3) {                                       // up to 8 points: one register stage, no twiddle is read
    tables<T><<<ew_grid(p.L), kET, 0, st>>>(tw, p.L, nullptr, 0);
    CPLXAMD_CHECK_LAUNCH();
  }
  // filter index strides per run: the kept runs in row-major order
  int64_t hs[3] = {0, 0, 0}, acc = 1;
  for (int s = 2; s >= 0; --s)
    if (kept[s] >= 0) {
      hs[kept[s]] = acc;
      acc *= r.size[kept[s]];
    }
  {
    // the spectra: the transform kernel over the kept runs, interleaved C2 out (planes H.re / H.im, element stride 2)
    int64_t out[3];
    for (int s = 0; s < 3; ++s) out[s] = hs[s] * 2 * p.L;
    const Sub hb = sub_runs(r, kept, r.bs, out);
    const Batch b{filters, hb.s1, hb.s2, {hb.p[0], hb.p[1], hb.p[2]}, {hb.q[0], hb.q[1], hb.q[2]}};
    FftPlan fp;
    if (const int e = fft_plan_for(p.L, filters, dtype, fp)) return e;
    const Io<TI, T, T, FilterIn<TI, T>> io{(const TI*)b_r, (const TI*)b_i, (T*)H, (T*)H + 1, d.b_es, 2, p.L, d.k, nullptr,
                                            nullptr, false, (T)1 / (T)p.L, FilterIn<TI, T>{d.b_es}};
    if (const int e = fft_lds_any<TI, T, T, false, FilterIn<TI, T>>(fp, fp.vpw > 1, io, b, tw, st)) return e;
  }
  const int all[3] = {0, 1, 2};
  ConvIo<TI, TI, T> g{(const TI*)a_r, (const TI*)a_i, (TI*)y_r, (TI*)y_i, H, d.a_len, d.c_len, p.S, p.in_shift, p.blocks,
                      r.rows * p.blocks, d.a_es, sub_runs(r, all, r.as, r.ys), sub_runs(r, all, hs, hs), (int)p.out_lo,
                      (int)(p.n_valid < p.L ? p.n_valid : p.L), d.conj != 0};
  if (p.logL <= kLogPackMax)
    return with_log<0, kLogPackMax>(p.logL, [&](auto c) -> int {
      constexpr int LG = decltype(c)::value;
      return launch_conv<TI, TI, T, LG, kVecs<LG>>(g, tw, st);
    });
  return with_log<kLogPackMax + 1, kLogConvMax>(p.logL, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    return launch_conv<TI, TI, T, LG, 1>(g, tw, st);
  });
}

}  // namespace

extern "C" {

int cplxamd_fftconv_plan(int64_t a_len, int64_t k, int64_t start, int64_t c_len, int64_t rows, int64_t filters, int dtype,
                         int conj, int log_l, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  ConvPlan p;
  if (const int e = conv_plan_for(a_len, k, start, c_len, rows, filters, dtype, conj, log_l, p)) return e;
  out[CPLXAMD_FFTCONV_LOG_L] = p.logL;
  out[CPLXAMD_FFTCONV_S] = p.S;
  out[CPLXAMD_FFTCONV_BLOCKS] = p.blocks;
  out[CPLXAMD_FFTCONV_VPW] = p.vpw;
  out[CPLXAMD_FFTCONV_IN_SHIFT] = p.in_shift;
  out[CPLXAMD_FFTCONV_OUT_LO] = p.out_lo;
  out[CPLXAMD_FFTCONV_N_VALID] = p.n_valid;
  out[CPLXAMD_FFTCONV_WS_BYTES] = p.bytes;
  out[CPLXAMD_FFTCONV_WGRAD_LOG_L] = p.wlogL;
  out[CPLXAMD_FFTCONV_WGRAD_S] = p.Sw;
  out[CPLXAMD_FFTCONV_WGRAD_BLOCKS] = p.wblocks;
  out[CPLXAMD_FFTCONV_WGRAD_CHUNKS] = p.chunks;
  out[CPLXAMD_FFTCONV_WGRAD_PER_CHUNK] = p.per_chunk;
  out[CPLXAMD_FFTCONV_WGRAD_WS_BYTES] = p.wbytes;
  return p.path;
}

int cplxamd_fftconv(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                    const cplxamd_fftconv_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  ConvRuns r;
  ConvPlan p;
  int64_t filters;
  int kept[3];
  if (const int e = conv_check(a_r, b_r, y_r, d, ws, dtype, false, r, filters, kept, p)) return e;
  int64_t total;
  if (__builtin_mul_overflow(r.rows, p.blocks, &total) || total > 0x7fffffffll) return CPLXAMD_ESHAPE;
  if (ws_bytes < p.bytes) return CPLXAMD_EWS;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (dtype == CPLXAMD_F64) return fftconv_t<double, double>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, dtype, w, st);
  if (dtype == CPLXAMD_BF16) return fftconv_t<bf16_t, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, dtype, w, st);
  return fftconv_t<float, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, dtype, w, st);
}

}  // extern "C"
