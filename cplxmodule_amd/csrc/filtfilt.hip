// Zero-phase filtering (cplx.filtfilt, cplx.sosfiltfilt: cplxmodule_amd/filtfilt.py): the EXTENDED pass
// of iir.hip's recurrence.  There is one kernel body, iir_chunks (iir_impl.h); this unit instantiates it with the EXT
// policy, which adds
//   1. a loader that forms the edge extension of scipy's filtfilt(method="pad") from x where it lies: logical sample m
//      of the row of n + 2 e samples is x[j], x[k] or 2 x[k] - x[j] by the index map iir_ext_src, the two anchors x[0]
//      and x[n - 1] fetched once per workgroup into LDS (two words per plane).  No padded copy exists anywhere;
//   2. the entering state as a UNIT state per filter (lfilter_zi / sosfilt_zi) times the first sample in processing order;
//   3. a store that keeps a window of the logical samples, in an element type of its own.
// Zero-phase filtering is two launches: x -> workspace (compute type, all n + 2 e samples; bf16 operands are never
// rounded in between), workspace reversed -> y (the interior only, the operands' dtype).  Every rule of iir.hip holds:
// one wave per workgroup, no workgroup waits for another, no atomics, no library state, nothing read on the host.
#include "iir_impl.h"
#include "runs.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

constexpr int kFlagsAll = CPLXAMD_FILTFILT_REVERSE | CPLXAMD_FILTFILT_SCALE;

// iir_plan_for over the extended row, the anchors added to the LDS bytes
int ext_plan_for(int64_t n, int64_t edge, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype, int cplx,
                 int64_t force, IirPlan& p) {
  if (n < 1 || edge < 0 || edge >= n) return CPLXAMD_EINVAL;
  if (n > kIirLenMax) return CPLXAMD_ESHAPE;
  if (const int e = iir_plan_for(n + 2 * edge, order, sections, rows, filters, dtype, cplx, force, p)) return e;
  p.lds += (cplx ? 2 : 1) * 2 * (dtype == CPLXAMD_F64 ? 8 : 4);
  return p.lds > kIirLdsBudget ? CPLXAMD_ESHAPE : 0;
}

template <typename TI, typename TO, typename T, bool CX, int DK>
int ext_k(const IirIo<TI, T, TO, T>& g, const IirPlan& p, hipStream_t st) {
  static PerDeviceOnce once;
  if (const int e = set_max_dyn_lds(once, iir_chunks<TI, T, CX, DK, TO, T, true>, (int)kIirLdsBudget)) return e;
  iir_chunks<TI, T, CX, DK, TO, T, true><<<(unsigned)p.grid, (unsigned)p.threads, (size_t)p.lds, st>>>(g);
  CPLXAMD_CHECK_LAUNCH();
  return 0;
}

template <typename TI, typename TO, typename T>
int ext_t(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r, const void* zi_i, void* y_r,
          void* y_i, void* zf_r, void* zf_i, const cplxamd_filtfilt_desc& d, const ConvRuns& r, const int64_t* zs,
          const IirPlan& p, bool cplx, hipStream_t st) {
  const int all[3] = {0, 1, 2};
  IirIo<TI, T, TO, T> g{(const TI*)x_r, (const TI*)x_i, (const T*)c_r, (const T*)c_i, (const T*)zi_r, (const T*)zi_i, (TO*)y_r,
                        (TO*)y_i, (T*)zf_r, (T*)zf_i, d.n, d.segments, d.seg_len, d.x_es, sub_runs(r, all, r.as, r.ys),
                        sub_runs(r, all, r.bs, zs), (int)d.order, (int)d.sections,
                        (d.flags & CPLXAMD_FILTFILT_REVERSE) != 0, false, d.edge, d.y_lo, d.y_n, (int)d.mode,
                        (d.flags & CPLXAMD_FILTFILT_SCALE) != 0};
  if (p.bucket == 8) return cplx ? ext_k<TI, TO, T, true, 8>(g, p, st) : ext_k<TI, TO, T, false, 8>(g, p, st);
  return cplx ? ext_k<TI, TO, T, true, 2>(g, p, st) : ext_k<TI, TO, T, false, 2>(g, p, st);
}

bool mode_ok(int mode) {
  return mode == CPLXAMD_FILTFILT_ODD || mode == CPLXAMD_FILTFILT_EVEN || mode == CPLXAMD_FILTFILT_CONSTANT;
}

}  // namespace

extern "C" {

int cplxamd_filtfilt_plan(int64_t n, int64_t edge, int64_t order, int64_t sections, int64_t rows, int64_t filters, int dtype,
                          int cplx, int64_t force_segments, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  IirPlan p;
  if (const int e = ext_plan_for(n, edge, order, sections, rows, filters, dtype, cplx, force_segments, p)) return e;
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
  out[CPLXAMD_FILTFILT_LEN] = n + 2 * edge;
  int64_t bytes;
  if (__builtin_mul_overflow(rows, (n + 2 * edge) * (cplx ? 2 : 1) * (dtype == CPLXAMD_F64 ? 8 : 4), &bytes))
    return CPLXAMD_ESHAPE;
  out[CPLXAMD_FILTFILT_SIGNAL_BYTES] = bytes;
  return p.path;
}

int cplxamd_filtfilt_src(int64_t m, int64_t n, int64_t edge, int mode, int64_t* out) {
  if (!out || n < 1 || edge < 0 || edge >= n || m < 0 || m >= n + 2 * edge || !mode_ok(mode)) return CPLXAMD_EINVAL;
  const IirSrc s = iir_ext_src(m, n, edge, mode);
  out[0] = s.j;
  out[1] = s.k;
  return 0;
}

int cplxamd_filtfilt_pass(const void* x_r, const void* x_i, const void* c_r, const void* c_i, const void* zi_r,
                          const void* zi_i, void* y_r, void* y_i, void* zf_r, void* zf_i, const cplxamd_filtfilt_desc* d,
                          int cplx, int in_dtype, int out_dtype, void* stream) {
  if (!c_r || !d || (!y_r && !zf_r) || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (!cplx && (x_i || c_i || zi_i || y_i || zf_i)) return CPLXAMD_EINVAL;
  if (cplx && ((y_r && !y_i) || (zf_r && !zf_i))) return CPLXAMD_EINVAL;
  if ((x_i && !x_r) || (zi_i && !zi_r) || (y_i && !y_r) || (zf_i && !zf_r)) return CPLXAMD_EINVAL;
  const bool f32 = in_dtype == CPLXAMD_F32 && (out_dtype == CPLXAMD_F32 || out_dtype == CPLXAMD_BF16);
  const bool b16 = in_dtype == CPLXAMD_BF16 && out_dtype == CPLXAMD_F32;
  const bool f64 = in_dtype == CPLXAMD_F64 && out_dtype == CPLXAMD_F64;
  if (!f32 && !b16 && !f64) return CPLXAMD_EINVAL;
  if (d->x_es < 0 || (d->flags & ~kFlagsAll) != 0 || d->reserved != 0 || !mode_ok(d->mode)) return CPLXAMD_EINVAL;
  if (d->n < 1 || d->edge < 0 || d->edge >= d->n || d->n > kIirLenMax) return CPLXAMD_EINVAL;
  const int64_t nlog = d->n + 2 * d->edge;
  if (d->segments < 1 || d->seg_len < 1 || d->segments > nlog) return CPLXAMD_EINVAL;
  if (y_r && (d->y_lo < 0 || d->y_n < 1 || d->y_lo > nlog || d->y_n > nlog - d->y_lo)) return CPLXAMD_EINVAL;
  if ((d->flags & CPLXAMD_FILTFILT_SCALE) && (!zi_r || d->segments != 1)) return CPLXAMD_EINVAL;
  using D = cplxamd_filtfilt_desc;
  ConvRuns r;
  int64_t zs[3];
  const RunStride<D> f[] = {{&D::x_stride, r.as}, {&D::c_stride, r.bs}, {&D::z_stride, zs}, {&D::y_stride, r.ys}};
  if (const int e = decode_runs(*d, f, r.size, r.rows)) return e;
  IirPlan p;
  if (const int e = ext_plan_for(d->n, d->edge, d->order, d->sections, r.rows, 1, in_dtype, cplx, d->segments, p)) return e;
  // the descriptor's own cut of the extended row: every sample in exactly one non-empty segment
  if (d->seg_len > nlog || d->segments != ceil_div(nlog, d->seg_len)) return CPLXAMD_EINVAL;
  if (__builtin_mul_overflow(r.rows, d->segments, &p.grid) || p.grid > 0x7fffffffll) return CPLXAMD_ESHAPE;
  if (r.rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool cx = cplx != 0;
  if (f64) return ext_t<double, double, double>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, zs, p, cx, st);
  if (b16) return ext_t<bf16_t, float, float>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, zs, p, cx, st);
  if (out_dtype == CPLXAMD_BF16)
    return ext_t<float, bf16_t, float>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, zs, p, cx, st);
  return ext_t<float, float, float>(x_r, x_i, c_r, c_i, zi_r, zi_i, y_r, y_i, zf_r, zf_i, *d, r, zs, p, cx, st);
}

}  // extern "C"
