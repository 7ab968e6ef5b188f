// The second primitive of cplx.upfirdn / cplx.resample_poly (upfirdn.hip describes both): the correlation of a row with
// a row at another rate that yields K taps, summed over the rows that share one result,
//     y[f][k] = sum_{rows of f} sum_{n < c_len} conj(au[r][n down + off - k]) c[r][n],   k < K,
// au being a upsampled by up.  A run of the batch whose y stride is 0 is reduced.  A term exists where
// i up = n down + off - k for a sample i of a: for one tap k those n are one residue class modulo up / gcd(up, down), so a
// thread that owns a tap steps n by up / g and i by down / g and multiplies no structural zero.  Workgroup (f, chunk,
// block of <= 1024 taps) of upfirdn_wgrad_part walks its chunk of (reduced row, tile of Tn entries of c) pairs in
// ascending order: it stages the tile and the span of a the tile meets over its taps, ((Tn - 1) down + 1023) / up + 2
// samples, into LDS, each thread adds to at most four accumulators in registers, and the workgroup writes one partial.
// upfirdn_wgrad_finish adds the partials of a result in ascending chunk order and rounds once.  Fixed orders, no atomics:
// reruns give the same bits.  Chunks: about three workgroups per CU, the partials bounded as fftconv_wgrad's.
#include "upfirdn_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// x^-1 modulo m for coprime x, m (0 for m = 1)
int64_t inverse_mod(int64_t x, int64_t m) {
  int64_t r0 = m, r1 = x % m, t0 = 0, t1 = 1;
  while (r1) {
    const int64_t q = r0 / r1, r2 = r0 - q * r1, t2 = t0 - q * t1;
    r0 = r1, r1 = r2, t0 = t1, t1 = t2;
  }
  return m == 1 ? 0 : ((t0 % m) + m) % m;
}

template <typename TI, typename T, bool AC, bool CC>
int wgrad_k(const UpWgradIo<TI>& g, const UpPlan& p, int64_t filters, TI* y_r, TI* y_i, const Sub& ys, int64_t K, C2<T>* part,
            hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = set_max_dyn_lds(once, upfirdn_wgrad_part<TI, T, AC, CC>, (int)kUpLdsBudget)) return e;
  upfirdn_wgrad_part<TI, T, AC, CC><<<(unsigned)(filters * p.chunks * p.kblocks), kUpThreads, (size_t)p.wlds, st>>>(g, part);
  CPLXAMD_CHECK_LAUNCH();
  upfirdn_wgrad_finish<TI, T><<<ew_grid(filters * K), kET, 0, st>>>(part, filters, p.chunks, K, y_r, y_i, ys);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename T>
int wgrad_t(const void* a_r, const void* a_i, const void* c_r, const void* c_i, void* y_r, void* y_i,
            const cplxamd_upfirdn_desc& d, const ConvRuns& r, int64_t filters, const int (&kept)[3], const UpPlan& p, void* ws,
            hipStream_t st) {
  int red[3];
  select_runs(r, r.ys, false, red);
  const int64_t gg = gcd64(d.up, d.down), upg = d.up / gg, downg = d.down / gg;
  const UpWgradIo<TI> g{(const TI*)a_r, (const TI*)a_i, (const TI*)c_r, (const TI*)c_i, d.a_len, d.k, d.c_len, d.up, d.down,
                        d.off, d.a_es, d.b_es, p.wtiles, p.pairs, p.per_chunk, p.chunks, gg, upg, downg,
                        inverse_mod(downg, upg), sub_runs(r, kept, r.as, r.bs), sub_runs(r, red, r.as, r.bs), (int)p.Tn,
                        (int)p.wspan, (int)p.kb, (int)p.kblocks};
  const Sub ys = sub_runs(r, kept, r.ys, r.ys);
  C2<T>* part = (C2<T>*)ws;
  if (a_i && c_i) return wgrad_k<TI, T, true, true>(g, p, filters, (TI*)y_r, (TI*)y_i, ys, d.k, part, st);
  if (a_i) return wgrad_k<TI, T, true, false>(g, p, filters, (TI*)y_r, (TI*)y_i, ys, d.k, part, st);
  if (c_i) return wgrad_k<TI, T, false, true>(g, p, filters, (TI*)y_r, (TI*)y_i, ys, d.k, part, st);
  return wgrad_k<TI, T, false, false>(g, p, filters, (TI*)y_r, (TI*)y_i, ys, d.k, part, st);
}

}  // namespace

extern "C" {

int cplxamd_upfirdn_wgrad(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                          const cplxamd_upfirdn_desc* d, int dtype, void* ws, int64_t ws_bytes, void* stream) {
  ConvRuns r;
  UpPlan p;
  int64_t filters;
  int kept[3];
  if (!ws) return CPLXAMD_EINVAL;
  if (const int e = up_check(a_r, a_i, b_r, b_i, y_r, d, dtype, true, r, filters, kept, p)) return e;
  if (ws_bytes < p.wbytes) return CPLXAMD_EWS;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F64) return wgrad_t<double, double>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, ws, st);
  if (dtype == CPLXAMD_BF16) return wgrad_t<bf16_t, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, ws, st);
  return wgrad_t<float, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, filters, kept, p, ws, st);
}

}  // extern "C"
