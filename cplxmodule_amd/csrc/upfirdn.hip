// Rational rate change along the last dim: upsample by `up`, FIR filter, downsample by `down`, as direct-form polyphase
// kernels (cplx.upfirdn, cplx.resample_poly: cplxmodule_amd/upfirdn.py).  Write au for a row of a upsampled by up
// (au[i up] = a[i], zero elsewhere and outside the row; never materialised).  Two primitives over rows of up to three
// batch runs, each the other's gradient with the rates swapped:
//   P1  y[r][n] = sum_k b[r][k] au[r][n down + off - k]       (conj: sum_k conj(b[r][k]) au[r][n down + off + k]),  n < c_len
//   P2  y[f][k] = sum_{rows of f} sum_n conj(au[r][n down + off - k]) c[r][n],  k < K            (upfirdn_wgrad.hip)
// The filter b has K <= 4096 taps.
//
// P1 is one launch of upfirdn_lds (upfirdn_impl.h).  With q = n down + off only the taps k = q mod up, + up, + 2 up, ...
// meet a sample of a: one polyphase branch of ceil(K / up) taps, a short dot product per output, and the structural zeros
// of au are never multiplied.  A workgroup takes a tile of T <= 1024 consecutive outputs of a row (four per thread; rows of
// one tile are packed up to 64 to a workgroup, each in its own LDS slice), stages the samples the tile touches,
// ((T - 1) down + up - 1) / up + ceil(K / up) of them, with coalesced loads (the loader writes the zeros outside the row),
// and the filter once, polyphase-major.  The plan (up_plan_for) picks T so that both fit 76 KiB, which leaves two
// workgroups per CU: a heavy decimation gets a smaller tile (down to 64 outputs), a filter that still does not fit is
// walked in segments of jseg taps per phase, ascending, the sums staying in registers, so the bits do not depend on
// the segmentation.  Real and complex operands are template instances: a real operand has no imaginary plane in LDS and
// costs no multiply.  Accumulation is float32 (float64 for float64 planes), one rounding on store.
// No atomics, no state in the library, no workspace, nothing read on the host.
#include "upfirdn_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI, typename T, bool XC, bool HC>
int upfirdn_k(const UpIo<TI>& g, const UpPlan& p, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = set_max_dyn_lds(once, upfirdn_lds<TI, T, XC, HC>, (int)kUpLdsBudget)) return e;
  upfirdn_lds<TI, T, XC, HC><<<(unsigned)p.grid, (unsigned)p.threads, (size_t)p.lds, st>>>(g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename T>
int upfirdn_t(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
              const cplxamd_upfirdn_desc& d, const ConvRuns& r, const UpPlan& p, hipStream_t st) {
  const int all[3] = {0, 1, 2};
  UpIo<TI> g{(const TI*)a_r, (const TI*)a_i, (const TI*)b_r, (const TI*)b_i, (TI*)y_r, (TI*)y_i, d.a_len, d.k, d.c_len,
             d.up, d.down, d.off, d.a_es, d.b_es, p.tiles, r.rows * p.tiles, sub_runs(r, all, r.as, r.ys),
             sub_runs(r, all, r.bs, r.bs), (int)p.T, (int)p.vpw, (int)p.span, (int)p.phases, (int)p.J, (int)p.jseg,
             (int)p.segs, d.conj != 0, p.T * d.down + d.up < 0x7fffffffll};
  if (a_i && b_i) return upfirdn_k<TI, T, true, true>(g, p, st);
  if (a_i) return upfirdn_k<TI, T, true, false>(g, p, st);
  if (b_i) return upfirdn_k<TI, T, false, true>(g, p, st);
  return upfirdn_k<TI, T, false, false>(g, p, st);
}

}  // namespace

extern "C" {

int cplxamd_upfirdn_plan(int64_t a_len, int64_t k, int64_t c_len, int64_t up, int64_t down, int64_t off, int64_t rows,
                         int64_t filters, int dtype, int conj, int a_cplx, int b_cplx, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  UpPlan p;
  if (const int e = up_plan_for(a_len, k, c_len, up, down, off, rows, filters, dtype, conj, a_cplx, b_cplx, p)) return e;
  out[CPLXAMD_UPFIRDN_T] = p.T;
  out[CPLXAMD_UPFIRDN_TILES] = p.tiles;
  out[CPLXAMD_UPFIRDN_VPW] = p.vpw;
  out[CPLXAMD_UPFIRDN_SPAN] = p.span;
  out[CPLXAMD_UPFIRDN_PHASES] = p.phases;
  out[CPLXAMD_UPFIRDN_JSEG] = p.jseg;
  out[CPLXAMD_UPFIRDN_SEGS] = p.segs;
  out[CPLXAMD_UPFIRDN_LDS_BYTES] = p.lds;
  out[CPLXAMD_UPFIRDN_THREADS] = p.threads;
  out[CPLXAMD_UPFIRDN_GRID] = p.grid;
  out[CPLXAMD_UPFIRDN_WGRAD_TN] = p.Tn;
  out[CPLXAMD_UPFIRDN_WGRAD_TILES] = p.wtiles;
  out[CPLXAMD_UPFIRDN_WGRAD_KB] = p.kb;
  out[CPLXAMD_UPFIRDN_WGRAD_KBLOCKS] = p.kblocks;
  out[CPLXAMD_UPFIRDN_WGRAD_SPAN] = p.wspan;
  out[CPLXAMD_UPFIRDN_WGRAD_LDS_BYTES] = p.wlds;
  out[CPLXAMD_UPFIRDN_WGRAD_CHUNKS] = p.chunks;
  out[CPLXAMD_UPFIRDN_WGRAD_PER_CHUNK] = p.per_chunk;
  out[CPLXAMD_UPFIRDN_WGRAD_WS_BYTES] = p.wbytes;
  return p.path;
}

int cplxamd_upfirdn(const void* a_r, const void* a_i, const void* b_r, const void* b_i, void* y_r, void* y_i,
                    const cplxamd_upfirdn_desc* d, int dtype, void* stream) {
  ConvRuns r;
  UpPlan p;
  int64_t filters;
  int kept[3];
  if (const int e = up_check(a_r, a_i, b_r, b_i, y_r, d, dtype, false, r, filters, kept, p)) return e;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F64) return upfirdn_t<double, double>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, p, st);
  if (dtype == CPLXAMD_BF16) return upfirdn_t<bf16_t, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, p, st);
  return upfirdn_t<float, float>(a_r, a_i, b_r, b_i, y_r, y_i, *d, r, p, st);
}

}  // extern "C"
