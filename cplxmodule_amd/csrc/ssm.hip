// The diagonal state-space scan with N states per row, along the last dim, as ONE kernel that keeps the states on chip
// (cplx.ssm_scan: cplxmodule_amd/ssm.py).  In processing order p (step p is sample p, or n - 1 - p in
// reverse):
//   h[s, p] = A[s, p] h[s, p - 1] + b[s, p] X[p],   y[p] = sum_s c[s, p] h[s, p],   h[s, -1] = h0[s] (or zero)
// A is a itself (one value per state, or one per step) or exp(dt[p] a[s]) formed in registers with cplx.exp's device
// function; X is x, or dt x.  Four flags: `reverse`; `conj` conjugates a, b and c; `lag` takes the coefficient (and its
// dt) of step p - 1, and what enters step 0 is not scaled; `dt_out` moves the factor dt from x on load to y on store.
// With b and c swapped and all four flipped the kernel is its own adjoint in x (cplxamd.h states the identity).
//
// Work split: scan.hip's row plan.  A workgroup of four waves walks one row's tiles of 256 L steps (L = 16); a thread
// owns a chunk of L steps, whose x (times dt), dt and 2 L accumulators of y stay in VGPRs for the whole tile.  The states
// go by in groups of G (ssm_group): per state, (1) the chunk from zero state for its map (P, s); (2) per GROUP, the maps
// composed in order -- a log-depth __shfl_up scan over the lanes, the four waves' totals through a double-buffered LDS
// exchange, one barrier; (3) the chunk again from its true entering state, y[q] += c[s, q] h.  y is stored once per tile,
// 16 bytes per access.  The carried states of all N states go from tile to tile through LDS (N values, double-buffered by
// the tile's parity, moved on by thread 0), not through registers.  b and c are read per state in phase 1 (b) and
// again in phase 3 (b, c): shared by the rows of a batch entry they come from cache.  A coefficient that varies along
// time (and exp(dt a)) is formed once per state and tile and held from phase 1 to phase 3.
// No atomics, no spin loops, no workspace; rows are not cut into segments: a few long rows run on a few workgroups.
#include "ssm_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI>
int ssm_t(const SsmIo<TI>& g, unsigned grid, bool cplx, int mode, hipStream_t st) {
#define CPLXAMD_SSM_CASE(CX, AM)                                      \
  if (cplx == CX && mode == AM) {                                     \
    ssm_chunks<TI, CX, AM><<<grid, kScanThreads, 0, st>>>(g);         \
    CPLXAMD_CHECK_LAUNCH();                                           \
    return 0;                                                         \
  }
  CPLXAMD_SSM_CASE(true, kSsmConst)
  CPLXAMD_SSM_CASE(true, kSsmVary)
  CPLXAMD_SSM_CASE(true, kSsmDt)
  CPLXAMD_SSM_CASE(false, kSsmConst)
  CPLXAMD_SSM_CASE(false, kSsmVary)
  CPLXAMD_SSM_CASE(false, kSsmDt)
#undef CPLXAMD_SSM_CASE
  return CPLXAMD_EINVAL;
}

template <typename TI>
SsmIo<TI> ssm_io(const void* const (&in)[11], void* const (&out)[4], const cplxamd_ssm_desc& d, const int64_t (&size)[3],
                 const int64_t (&rs)[kSsmPlanes][3]) {
  SsmIo<TI> g{};
  const TI** src[9] = {&g.ar, &g.ai, &g.br, &g.bi, &g.cr, &g.ci, &g.xr, &g.xi, &g.dt};
  for (int k = 0; k < 9; ++k) *src[k] = (const TI*)in[k];
  g.hr = (const float*)in[9], g.hi = (const float*)in[10];
  g.yr = (TI*)out[0], g.yi = (TI*)out[1], g.fr = (float*)out[2], g.fi = (float*)out[3];
  g.n = d.n, g.states = (int)d.states;
  g.a_es = d.a_es, g.b_es = d.b_es, g.c_es = d.c_es;
  g.a_ns = d.a_ns, g.b_ns = d.b_ns, g.c_ns = d.c_ns, g.h_ns = d.h_ns, g.f_ns = d.f_ns;
  g.s1 = size[1], g.s2 = size[2];
  for (int k = 0; k < kSsmPlanes; ++k)
    for (int s = 0; s < 3; ++s) g.rs[k][s] = rs[k][s];
  g.rev = (d.flags & CPLXAMD_SSM_REVERSE) != 0, g.conj = (d.flags & CPLXAMD_SSM_CONJ) != 0;
  g.lag = (d.flags & CPLXAMD_SSM_LAG) != 0, g.dt_out = (d.flags & CPLXAMD_SSM_DT_OUT) != 0;
  return g;
}

}  // namespace

extern "C" {

int cplxamd_ssm_plan(int64_t n, int64_t states, int64_t rows, int dtype, int cplx, int time_varying, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  SsmPlan p;
  if (const int e = ssm_plan_for(n, states, rows, dtype, cplx, time_varying, p)) return e;
  out[CPLXAMD_SSM_CHUNK] = p.chunk;
  out[CPLXAMD_SSM_TILE] = p.tile;
  out[CPLXAMD_SSM_TILES] = p.tiles;
  out[CPLXAMD_SSM_GROUP] = p.group;
  out[CPLXAMD_SSM_LDS_BYTES] = p.lds;
  out[CPLXAMD_SSM_THREADS] = p.threads;
  out[CPLXAMD_SSM_GRID] = p.grid;
  out[CPLXAMD_SSM_WINDOW] = p.window;
  return 0;
}

int cplxamd_ssm_scan(const void* a_r, const void* a_i, const void* b_r, const void* b_i, const void* c_r, const void* c_i,
                     const void* x_r, const void* x_i, const void* dt, const void* h_r, const void* h_i, void* y_r,
                     void* y_i, void* f_r, void* f_i, const cplxamd_ssm_desc* d, int cplx, int dtype, void* stream) {
  if (!a_r || !b_r || !c_r || !x_r || !y_r || !d || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  if (!cplx && (a_i || b_i || c_i || x_i || h_i || y_i || f_i)) return CPLXAMD_EINVAL;
  if ((cplx && !y_i) || (h_i && !h_r) || (cplx && (f_r != nullptr) != (f_i != nullptr))) return CPLXAMD_EINVAL;
  const int all = CPLXAMD_SSM_REVERSE | CPLXAMD_SSM_CONJ | CPLXAMD_SSM_LAG | CPLXAMD_SSM_DT_OUT;
  if ((d->flags & ~all) != 0 || (d->a_es | d->b_es | d->c_es) < 0 || (d->a_es | d->b_es | d->c_es) > 1) return CPLXAMD_EINVAL;
  if (d->a_ns < 0 || d->b_ns < 0 || d->c_ns < 0 || d->h_ns < 0 || d->f_ns < 0) return CPLXAMD_EINVAL;
  if (dt && d->a_es != 0) return CPLXAMD_EINVAL;            // exp(dt a) takes the poles: one value per state
  int64_t size[3], rows, rs[kSsmPlanes][3];
  using D = cplxamd_ssm_desc;
  const RunStride<D> f[] = {{&D::a_stride, rs[kSsmA]}, {&D::b_stride, rs[kSsmB]}, {&D::c_stride, rs[kSsmC]},
                            {&D::x_stride, rs[kSsmX]}, {&D::dt_stride, rs[kSsmD]}, {&D::h_stride, rs[kSsmH]},
                            {&D::y_stride, rs[kSsmY]}, {&D::f_stride, rs[kSsmF]}};
  if (const int e = decode_runs(*d, f, size, rows)) return e;
  const int mode = dt ? kSsmDt : (d->a_es == 0 ? kSsmConst : kSsmVary);
  SsmPlan p;
  if (const int e = ssm_plan_for(d->n, d->states, rows, dtype, cplx, mode != kSsmConst, p)) return e;
  if (p.grid == 0) return 0;
  const void* const in[11] = {a_r, a_i, b_r, b_i, c_r, c_i, x_r, x_i, dt, h_r, h_i};
  void* const out[4] = {y_r, y_i, f_r, f_i};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_BF16) return ssm_t<bf16_t>(ssm_io<bf16_t>(in, out, *d, size, rs), (unsigned)p.grid, cplx != 0, mode, st);
  return ssm_t<float>(ssm_io<float>(in, out, *d, size, rs), (unsigned)p.grid, cplx != 0, mode, st);
}

}  // extern "C"
