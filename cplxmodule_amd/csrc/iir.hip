// Recursive (IIR) filtering along the last dim: cascades of direct-form-II-transposed sections as ONE chunk-parallel
// kernel (cplx.lfilter, cplx.sosfilt: cplxmodule_amd/iir.py).  The primitive, for every (row, segment):
// take an entering state (zi, or zero), walk the segment's tiles in order carrying one state per section, optionally
// store y, optionally store the final state.  `reverse` runs the recurrence from the last sample to the first, `conj`
// conjugates the coefficients: the pair is the gradient of the plain run.
//
// A workgroup is ONE wave of 64 lanes; it takes (row, segment) and stages a tile of 64 L samples in LDS (L = 64; 32 for
// float64: 4096 / 2048 samples, about 40 KiB with the tables, so three or four workgroups share a CU).  The recurrence is
// linear, so inside the tile it is parallel in time:
//   1. lane c runs chunk c (L samples) from ZERO state, in place: a local response and a chunk-final state s_c.  Lane 0
//      starts from the carried state instead, so its chunk is final at once;
//   2. with M = A^L, the L-step transition of the section, the states at the chunk ends are P_c = M P_{c-1} + s_c, taken
//      IN ORDER over the 64 chunks: lane i carries component i, the components cross the lanes through scalar registers
//      (v_readlane: the workgroup is one wave, nothing waits on LDS inside the chain), s_{c+1} is fetched a step ahead.
//      Only M itself is ever applied: a log-depth scan would multiply states by M^2, M^4 ... M^32, whose entries grow
//      with the span for poles on the unit circle, and lose the exactness of step 2 on integer operands long before the
//      sequential recurrence does (measured: the double integrator failed at N = 2047 with such a scan);
//   3. lane c adds the zero-input response of its entering state P_{c-1}: y[c L + j] += sum_d zir[d][j] P_{c-1}[d];
//   4. the last lane's state is carried to the next tile (a part chunk at the end of a row: its local final state plus
//      its entering state run for as many zero-input steps as it has samples).
// In exact arithmetic this IS the sequential recurrence, and on integer operands every step is exact while the products
// of a state with a table entry (at most L + 1 for a double pole at 1) stay below 2^24.  A cascade repeats 1-4 per section
// on the tile in LDS: x is read once, y written once.  The tables (zir: D responses of L samples; M) are built by every
// workgroup in LDS from the coefficients, per call.  The lanes' chunks lie L + 1 words apart: no two lanes share a bank.
// Long rows with few rows are cut into segments (the plan): the caller runs the primitive for the segment-final states from
// zero entering state, once more on null input with unit entering states for the segment transition, scans the segments
// of each row with iir_scan, and runs the primitive again from the true entering states.  No workgroup waits for another
// inside a launch: the hand-off is the launch boundary.  No atomics, no state in the library, nothing read on the host.
#include "iir_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI, typename T, bool CX, int DK>
int iir_k(const IirIo<TI, T>& g, const IirPlan& p, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = set_max_dyn_lds(once, iir_chunks<TI, T, CX, DK>, (int)kIirLdsBudget)) return e;
  iir_chunks<TI, T, CX, DK><<<(unsigned)p.grid, (unsigned)p.threads, (size_t)p.lds, st>>>(g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename T>
int iir_t(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r, const void* zi_i, void* y_r,
          void* y_i, void* zf_r, void* zf_i, const cplxamd_iir_desc& d, const ConvRuns& r, const IirPlan& p, bool cplx,
          hipStream_t st) {
  const int all[3] = {0, 1, 2};
  IirIo<TI, T> g{(const TI*)x_r, (const TI*)x_i, (const TI*)c_r, (const TI*)c_i, (const T*)zi_r, (const T*)zi_i, (TI*)y_r,
                 (TI*)y_i, (T*)zf_r, (T*)zf_i, d.n, d.segments, d.seg_len, d.x_es, sub_runs(r, all, r.as, r.ys),
                 sub_runs(r, all, r.bs, r.bs), (int)d.order, (int)d.sections, (d.flags & CPLXAMD_IIR_REVERSE) != 0,
                 (d.flags & CPLXAMD_IIR_CONJ) != 0};
  if (p.bucket == 8) return cplx ? iir_k<TI, T, true, 8>(g, p, st) : iir_k<TI, T, false, 8>(g, p, st);
  return cplx ? iir_k<TI, T, true, 2>(g, p, st) : iir_k<TI, T, false, 2>(g, p, st);
}

template <typename T>
int scan_t(const void* z_r, const void* z_i, const void* m_r, const void* m_i, const void* zi_r, const void* zi_i, void* e_r,
           void* e_i, int64_t rows, int64_t rpf, int64_t segs, int w, bool cplx, hipStream_t st) {
  const unsigned grid = (unsigned)ceil_div(rows, kET);
  if (cplx)
    iir_scan<T, true><<<grid, kET, 0, st>>>((const T*)z_r, (const T*)z_i, (const T*)m_r, (const T*)m_i, (const T*)zi_r,
                                            (const T*)zi_i, (T*)e_r, (T*)e_i, rows, rpf, segs, w);
  else
    iir_scan<T, false><<<grid, kET, 0, st>>>((const T*)z_r, nullptr, (const T*)m_r, nullptr, (const T*)zi_r, nullptr,
                                             (T*)e_r, nullptr, rows, rpf, segs, w);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int cplxamd_iir_plan(int64_t n, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype, int cplx,
                     int64_t force_segments, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  IirPlan p;
  if (const int e = iir_plan_for(n, order, sections, rows, filters, dtype, cplx, force_segments, p)) return e;
  out[CPLXAMD_IIR_CHUNK] = p.chunk;
  out[CPLXAMD_IIR_LANES] = p.lanes;
  out[CPLXAMD_IIR_TILE] = p.tile;
  out[CPLXAMD_IIR_TILES] = p.tiles;
  out[CPLXAMD_IIR_SEGMENTS] = p.segments;
  out[CPLXAMD_IIR_SEG_LEN] = p.seg_len;
  out[CPLXAMD_IIR_BUCKET] = p.bucket;
  out[CPLXAMD_IIR_LDS_BYTES] = p.lds;
  out[CPLXAMD_IIR_THREADS] = p.threads;
  out[CPLXAMD_IIR_GRID] = p.grid;
  out[CPLXAMD_IIR_WS_BYTES] = p.ws;
  return p.path;
}

int cplxamd_iir(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r, const void* zi_i,
                void* y_r, void* y_i, void* zf_r, void* zf_i, const cplxamd_iir_desc* d, int cplx, int dtype, void* stream) {
  if (!c_r || !d || (!y_r && !zf_r) || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (!cplx && (x_i || c_i || zi_i || y_i || zf_i)) return CPLXAMD_EINVAL;
  if (cplx && ((y_r && !y_i) || (zf_r && !zf_i))) return CPLXAMD_EINVAL;
  if ((x_i && !x_r) || (zi_i && !zi_r) || (y_i && !y_r) || (zf_i && !zf_r)) return CPLXAMD_EINVAL;
  if (d->x_es < 0 || (d->flags & ~(CPLXAMD_IIR_REVERSE | CPLXAMD_IIR_CONJ)) != 0) return CPLXAMD_EINVAL;
  if (d->segments < 1 || d->seg_len < 1 || d->n < 1 || d->segments > d->n) return CPLXAMD_EINVAL;
  ConvRuns r;
  using D = cplxamd_iir_desc;
  const RunStride<D> f[] = {{&D::x_stride, r.as}, {&D::c_stride, r.bs}, {&D::y_stride, r.ys}};
  if (const int e = decode_runs(*d, f, r.size, r.rows)) return e;
  IirPlan p;
  if (const int e = iir_plan_for(d->n, d->order, d->sections, r.rows, 1, dtype, cplx, d->segments, p)) return e;
  // the descriptor's own cut of the row: every sample in exactly one non-empty segment
  if (d->seg_len > d->n || d->segments != ceil_div(d->n, d->seg_len)) return CPLXAMD_EINVAL;
  if (__builtin_mul_overflow(r.rows, d->segments, &p.grid) || p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F64)
    return iir_t<double, double>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, p, cplx != 0, st);
  if (dtype == CPLXAMD_BF16)
    return iir_t<bf16_t, float>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, p, cplx != 0, st);
  return iir_t<float, float>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, p, cplx != 0, st);
}

int cplxamd_iir_scan(const void* z_r, const void* z_i, const void* m_r, const void* m_i, const void* zi_r,
                     const void* zi_i, void* e_r, void* e_i, int64_t rows, int64_t rows_per_filter, int64_t segments,
                     int64_t width, int cplx, int dtype, void* stream) {
  if (!z_r || !m_r || !e_r || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (dtype != CPLXAMD_F32 && dtype != CPLXAMD_F64) return CPLXAMD_EINVAL;
  if (!cplx && (z_i || m_i || zi_i || e_i)) return CPLXAMD_EINVAL;
  if (cplx && (!z_i || !e_i)) return CPLXAMD_EINVAL;
  if (zi_i && !zi_r) return CPLXAMD_EINVAL;
  if (rows < 0 || rows_per_filter < 1 || segments < 1 || width < 1 || width > kIirScanWidth) return CPLXAMD_EINVAL;
  if (ceil_div(rows, kET) > 0x7fffffffll) return CPLXAMD_ESHAPE;
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F64)
    return scan_t<double>(z_r, z_i, m_r, m_i, zi_r, zi_i, e_r, e_i, rows, rows_per_filter, segments, (int)width, cplx != 0, st);
  return scan_t<float>(z_r, z_i, m_r, m_i, zi_r, zi_i, e_r, e_i, rows, rows_per_filter, segments, (int)width, cplx != 0, st);
}

}  // extern "C"
