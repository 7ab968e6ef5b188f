// The first-order linear recurrence with a coefficient per step, h[t] = a[t] h[t-1] + x[t] along the last dim, as ONE
// time-parallel kernel (cplx.linear_recurrence, cplx.cumsum, cplx.cumprod: cplxmodule_amd/scan.py).
// One primitive with three flags: `reverse` runs from the last sample, `conj` conjugates the coefficients, `lag` takes
// the coefficient that multiplies the travelling state from the position the state comes from (the adjoint's
// lambda[t] = g[t] + conj(a[t+1]) lambda[t+1], without a shifted copy of a).
//
// The unit of work is a chunk of L consecutive steps whose a and x stay in registers (L = 16; 8 for float64):
//   1. the chunk from zero state: its coefficient product P and local final state s, two multiply-adds per step;
//   2. the maps h -> P h + s in order, (P2, s2) o (P1, s1) = (P2 P1, P2 s1 + s2), give every chunk its true entering state;
//   3. the chunk again from that state, one multiply-add per step, and the store.
// No correction table and no second read of memory: the stored values come from the sequential recurrence started at the
// chunk's entering state, so a[t] = 0 and tiny |a| need nothing special.  Step 2 does form products of consecutive
// coefficients, over one tile (one segment in the split path): cplxamd.h states the limit.
//
// Two plans, from the strides (scan_plan_for).  ROW: time has stride 1 in the result; a chunk is a thread, a workgroup of
// four waves covers a tile of 256 L steps of one row with 16-byte accesses per lane; step 2 is a log-depth scan over the
// lanes of a wave (shuffles), then the four waves' totals in order through LDS; the state is carried to the row's next
// tile.  COLUMN: time is strided and a batch run has stride 1 (the [B, T, D] layout seen through a transpose): lanes lie
// along that run, so every load is one line; a chunk is a wave's L steps of 64 channels, the four waves take consecutive
// chunks of a tile of 4 L steps, step 2 runs in order over the waves through LDS.
// Long rows with few rows: time is cut into segments of whole tiles and the call is two launches.  The first writes one
// map (P, s) per (unit, segment) from zero state; in the second every workgroup composes the maps of the segments before
// its own, in order, and runs its segment from that state.  No workgroup waits for another, no atomics, every loop bound
// is known at launch, nothing is read on the host.
#include "scan_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI, typename T>
int scan_t(const void* a_r, const void* a_i, const void* x_r, const void* x_i, const void* h_r, const void* h_i, void* y_r,
           void* y_i, const cplxamd_scan_desc& d, const ScanRuns& s, const ScanPlan& p, bool cplx, void* ws, hipStream_t st) {
  const int rows[3] = {0, 1, 2}, outer[3] = {-1, 0, 1};
  const int(&sel)[3] = p.column ? outer : rows;
  ScanIo<TI, T> g{(const TI*)a_r, (const TI*)a_i, (const TI*)x_r, (const TI*)x_i, (const TI*)h_r, (const TI*)h_i,
                  (TI*)y_r, (TI*)y_i, (T*)ws, d.n, p.segments, p.seg_len, d.a_es, d.x_es, d.y_es,
                  sub_runs(s.r, sel, s.r.as, s.r.bs), sub_runs(s.r, sel, s.hs, s.r.ys), p.channels, p.cblocks,
                  s.r.as[2], s.hs[2], (d.flags & CPLXAMD_SCAN_REVERSE) != 0, (d.flags & CPLXAMD_SCAN_CONJ) != 0,
                  (d.flags & CPLXAMD_SCAN_LAG) != 0, false};
  for (int pass = p.segments > 1 ? 0 : 1; pass < 2; ++pass) {
    g.pairs = pass == 0;
    const unsigned grid = (unsigned)(p.units * (g.pairs ? p.segments - 1 : p.segments));
    if (cplx && p.column) scan_chunks<TI, T, true, true><<<grid, kScanThreads, 0, st>>>(g);
    else if (cplx) scan_chunks<TI, T, true, false><<<grid, kScanThreads, 0, st>>>(g);
    else if (p.column) scan_chunks<TI, T, false, true><<<grid, kScanThreads, 0, st>>>(g);
    else scan_chunks<TI, T, false, false><<<grid, kScanThreads, 0, st>>>(g);
    CPLXAMD_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" {

int cplxamd_scan_plan(const cplxamd_scan_desc* d, int dtype, int cplx, int64_t* out) {
  if (!d || !out) return CPLXAMD_EINVAL;
  ScanRuns s;
  if (const int e = scan_decode(*d, s)) return e;
  ScanPlan p;
  if (const int e = scan_plan_for(*d, s, dtype, cplx, p)) return e;
  out[CPLXAMD_SCAN_CHUNK] = p.chunk;
  out[CPLXAMD_SCAN_TILE] = p.tile;
  out[CPLXAMD_SCAN_TILES] = p.tiles;
  out[CPLXAMD_SCAN_SEGMENTS] = p.segments;
  out[CPLXAMD_SCAN_SEG_LEN] = p.seg_len;
  out[CPLXAMD_SCAN_WINDOW] = p.window;
  out[CPLXAMD_SCAN_UNITS] = p.units;
  out[CPLXAMD_SCAN_LDS_BYTES] = p.lds;
  out[CPLXAMD_SCAN_THREADS] = p.threads;
  out[CPLXAMD_SCAN_GRID] = p.grid;
  out[CPLXAMD_SCAN_WS_BYTES] = p.ws;
  return p.column ? CPLXAMD_SCAN_COLUMN : CPLXAMD_SCAN_ROW;
}

int cplxamd_scan(const void* a_r, const void* a_i, const void* x_r, const void* x_i, const void* h_r, const void* h_i,
                 void* y_r, void* y_i, const cplxamd_scan_desc* d, int cplx, int dtype, void* ws, int64_t ws_bytes,
                 void* stream) {
  if (!a_r || !y_r || !d || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (!cplx && (a_i || x_i || h_i || y_i)) return CPLXAMD_EINVAL;
  if ((cplx && !y_i) || (x_i && !x_r) || (h_i && !h_r)) return CPLXAMD_EINVAL;
  if ((d->flags & ~(CPLXAMD_SCAN_REVERSE | CPLXAMD_SCAN_CONJ | CPLXAMD_SCAN_LAG)) != 0) return CPLXAMD_EINVAL;
  if ((d->flags & CPLXAMD_SCAN_LAG) && h_r) return CPLXAMD_EINVAL;
  ScanRuns s;
  if (const int e = scan_decode(*d, s)) return e;
  ScanPlan p;
  if (const int e = scan_plan_for(*d, s, dtype, cplx, p)) return e;
  if (p.ws > 0 && (!ws || ws_bytes < p.ws)) return CPLXAMD_EWS;
  if (p.grid == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_F64)
    return scan_t<double, double>(a_r, a_i, x_r, x_i, h_r, h_i, y_r, y_i, *d, s, p, cplx != 0, ws, st);
  if (dtype == CPLXAMD_BF16)
    return scan_t<bf16_t, float>(a_r, a_i, x_r, x_i, h_r, h_i, y_r, y_i, *d, s, p, cplx != 0, ws, st);
  return scan_t<float, float>(a_r, a_i, x_r, x_i, h_r, h_i, y_r, y_i, *d, s, p, cplx != 0, ws, st);
}

}  // extern "C"
