// The second primitive of cplx.fftconvolve (fftconv.hip describes both): the correlation of two long rows that yields
// k taps, summed over the rows that share one result,
//     y[f][m] = sum_{rows of f} sum_{n < a_len} conj(a[r][n]) c[r][n + m + start],   m < k.
// A run of the batch whose y stride is 0 is reduced.  With S = L - k + 1, block j of a row pairs a[j S .. j S + S) (zero
// tail up to L) with c[j S + start .. + L): entry m < k of IFFT(conj(A-hat) C-hat) is that block's share, no wrap-around.
// The spectra are summed instead of the taps: workgroup (f, chunk) of fftconv_wgrad_lds walks its chunk of (reduced row,
// block) pairs in ascending order, transforms the a block into registers, the c block through the same LDS, and adds
// conj(A) C to an accumulator in registers, as the Welch kernels accumulate a spectrum over a chunk of segments; it
// writes one partial spectrum.  fftconv_wgrad_sum adds the partials of a result in ascending chunk order (one thread per
// entry), fftconv_wgrad_finish runs the one inverse transform and keeps k taps (scale 1 / L, one rounding).  Fixed
// orders, no atomics: reruns give the same bits.
// Chunks: enough workgroups to fill the device (about three per CU, as the 3-d convolution's split-K), the partials
// bounded as the engine bounds its batch buffers (kLargeWs).  L is this primitive's own (the plan's WGRAD fields): at
// least 2048 points where the row is that long, so that a workgroup has 256 threads.
#include "fftconv_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI, typename T>
int wgrad_t(const void* a_r, const void* a_i, const void* c_r, const void* c_i, void* y_r, void* y_i,
            const cplxamd_fftconv_desc& d, const ConvRuns& r, int64_t filters, const int (&kept)[3], const ConvPlan& p,
            char* ws, hipStream_t st) {
  C2<T>* tw = (C2<T>*)(ws + p.woff_tw);
  C2<T>* part = (C2<T>*)(ws + p.woff_part);
  if (p.wlogL > 3) {
    tables<T><<<ew_grid(p.Lw), kET, 0, st>>>(tw, p.Lw, nullptr, 0);
    CPLXAMD_CHECK_LAUNCH();
  }
  int red[3];
  select_runs(r, r.ys, false, red);
  const WgradIo<TI, T> g{(const TI*)a_r, (const TI*)a_i, (const TI*)c_r, (const TI*)c_i, d.a_len, d.c_len, p.Sw, d.start,
                         p.wblocks, p.pairs, p.per_chunk, p.chunks, d.a_es, d.b_es, sub_runs(r, kept, r.as, r.bs),
                         sub_runs(r, red, r.as, r.bs)};
  const Sub ys = sub_runs(r, kept, r.ys, r.ys);
  return with_log<0, kLogConvMax>(p.wlogL, [&](auto c) -> int {
    constexpr int LG = decltype(c)::value;
    static PerDeviceOnce once, once_finish;
    if (const int e = lds_attr(once, fftconv_wgrad_lds<TI, T, LG>)) return e;
    if (const int e = lds_attr(once_finish, fftconv_wgrad_finish<TI, T, LG>)) return e;
    fftconv_wgrad_lds<TI, T, LG><<<(unsigned)(filters * p.chunks), kNT<LG>, lds_bytes<T>(LG), st>>>(g, tw, part);
    CPLXAMD_CHECK_LAUNCH();
    if (p.chunks > 1) {
      fftconv_wgrad_sum<T><<<ew_grid(filters * p.Lw), kET, 0, st>>>(part, filters, p.chunks, p.Lw);
      CPLXAMD_CHECK_LAUNCH();
    }
    fftconv_wgrad_finish<TI, T, LG><<<(unsigned)filters, kNT<LG>, lds_bytes<T>(LG), st>>>(part, p.chunks, (TI*)y_r, (TI*)y_i, d.k,
                                                                                       (T)1 / (T)p.Lw, ys, tw);
    CPLXAMD_CHECK_LAUNCH();
    return 0;
  });
}

}  // namespace

extern "C" {

int cplxamd_fftconv_wgrad(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                          const cplxamd_fftconv_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  ConvRuns r;
  ConvPlan p;
  int64_t filters;
  int kept[3];
  if (const int e = conv_check(a_r, b_r, y_r, d, ws, dtype, true, r, filters, kept, p)) return e;
  int64_t wgs;
  if (__builtin_mul_overflow(filters, p.chunks, &wgs) || wgs > 0x7fffffffll) return CPLXAMD_ESHAPE;
  if (ws_bytes < p.wbytes) return CPLXAMD_EWS;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  if (dtype == CPLXAMD_F64) return wgrad_t<double, double>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, w, st);
  if (dtype == CPLXAMD_BF16) return wgrad_t<bf16_t, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, w, st);
  return wgrad_t<float, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, w, st);
}

}  // extern "C"
