// The gradients of a, b, c, dt and x of the diagonal state-space scan (csrc/ssm.hip) as ONE kernel that recomputes h and
// lambda in registers (the backward of cplx.ssm_scan when a parameter gradient is asked for: cplxmodule_amd/ssm.py;
// DESIGN section 29.8).  In processing order p (step p is sample p, or n - 1 - p in reverse), with X = x or dt x:
//   h[s, p]      = A[s, p] h[s, p - 1] + b[s, p] X[p]                             h[s, -1] = h0[s] (or zero)
//   lambda[s, p] = conj(c[s, p]) g[p] + conj(A[s, p + 1]) lambda[s, p + 1]        gf[s] enters step n - 1 unscaled
//   dc = g conj(h),  db = lambda conj(X),  dA = lambda conj(h[p - 1]),  dX[p] = sum_s conj(b[s, p]) lambda[s, p]
//   da = dA, or with dt: da[s] = sum_p dA conj(dt A),  ddt[p] = Re sum_s dA conj(a A) + Re(conj(x[p]) dX[p]);  dx = dX or dt dX
// the formulas of ssm.parameter_gradients.  The kernel carries mu[s, p] = conj(A[s, p]) lambda[s, p], what enters step
// p - 1, so that a chunk needs no coefficient of its neighbour.
//
// Work split: ssm.hip's.  A workgroup of four waves owns a row; a thread owns a chunk of L = 16 steps of every tile of
// 256 L steps, whose X, g, dt and the accumulators of dX and ddt stay in VGPRs for the whole tile.  The states go by in
// groups of G (ssm_pgrad_group): (1) per state, both chunk maps from zero state -- h's ascending, mu's descending; the
// coefficient chunk is formed once and held; (2) per GROUP, h's maps scanned up the lanes and mu's down, the waves' totals
// of both through a double-buffered LDS exchange, ONE barrier; (3) per state, the chunk of h rerun from its true entering
// state and kept, then mu's chunk rerun descending, forming dc, db, dA and the contributions to dX and ddt as it goes.
// A gradient that varies along time is stored by the thread that formed it, its own chunk, into a dense float32
// [rows, states, n] plane: no reduction.  A gradient of an operand with one value per state is summed over the chunk, over
// the wave by shuffles in a fixed order, and lane 0's sums go through a second double-buffered LDS exchange that the NEXT
// group's barrier publishes (one extra barrier per row, not per group); thread s adds the four waves' sums of state s to
// its own accumulators and stores them once per row as [rows, states].  The tiles are walked LAST TO FIRST: mu's carried
// states live in LDS as the forward's do.  The states of h that enter the tiles are needed in the other order: with more
// than one tile a prologue in the same launch runs phases 1 and 2 for h alone, first tile to last but one, and leaves
// them in a float32 workspace [rows, tiles, states] that the workgroup reads back behind a barrier -- its own row only.
// No atomics, no spin loops, no communication between workgroups: reruns give the same bits.
#include "ssm_grad_impl.h"

using namespace cplxamd;
using namespace cplxamd::sp;

namespace {

template <typename TI>
int pgrad_t(const SsmGradIo<TI>& g, unsigned grid, bool cplx, int mode, hipStream_t st) {
#define CPLXAMD_PGRAD_CASE(CX, AM)                                    \
  if (cplx == CX && mode == AM) {                                     \
    ssm_pgrad<TI, CX, AM><<<grid, kScanThreads, 0, st>>>(g);          \
    CPLXAMD_CHECK_LAUNCH();                                           \
    return 0;                                                         \
  }
  CPLXAMD_PGRAD_CASE(true, kSsmConst)
  CPLXAMD_PGRAD_CASE(true, kSsmVary)
  CPLXAMD_PGRAD_CASE(true, kSsmDt)
  CPLXAMD_PGRAD_CASE(false, kSsmConst)
  CPLXAMD_PGRAD_CASE(false, kSsmVary)
  CPLXAMD_PGRAD_CASE(false, kSsmDt)
#undef CPLXAMD_PGRAD_CASE
  return CPLXAMD_EINVAL;
}

template <typename TI>
SsmGradIo<TI> pgrad_io(const void* const* in, void* const* out, const cplxamd_ssm_pgrad_desc& d, int64_t tiles,
                       const int64_t (&size)[3], const int64_t (&rs)[kPgPlanes][3]) {
  SsmGradIo<TI> g{};
  const TI** src[9] = {&g.ar, &g.ai, &g.br, &g.bi, &g.cr, &g.ci, &g.xr, &g.xi, &g.dt};
  for (int k = 0; k < 9; ++k) *src[k] = (const TI*)in[k];
  g.hr = (const float*)in[9], g.hi = (const float*)in[10];
  g.gr = (const TI*)in[11], g.gi = (const TI*)in[12];
  g.fr = (const float*)in[13], g.fi = (const float*)in[14];
  g.dxr = (TI*)out[0], g.dxi = (TI*)out[1];
  float** dst[10] = {&g.dar, &g.dai, &g.dbr, &g.dbi, &g.dcr, &g.dci, &g.ddt, &g.lr, &g.li, &g.ws};
  for (int k = 0; k < 10; ++k) *dst[k] = (float*)out[2 + k];
  g.n = d.n, g.tiles = tiles, g.states = (int)d.states, g.need = d.need;
  g.b_es = (int)d.b_es, g.c_es = (int)d.c_es;
  g.a_ns = d.a_ns, g.b_ns = d.b_ns, g.c_ns = d.c_ns, g.h_ns = d.h_ns, g.f_ns = d.f_ns;
  g.s1 = size[1], g.s2 = size[2];
  for (int k = 0; k < kPgPlanes; ++k)
    for (int s = 0; s < 3; ++s) g.rs[k][s] = rs[k][s];
  g.rev = (d.flags & CPLXAMD_SSM_REVERSE) != 0;
  return g;
}

}  // namespace

extern "C" {

int cplxamd_ssm_pgrad_plan(int64_t n, int64_t states, int64_t rows, int dtype, int cplx, int time_varying, int64_t* out) {
  if (!out) return CPLXAMD_EINVAL;
  SsmGradPlan p;
  if (const int e = ssm_pgrad_plan_for(n, states, rows, dtype, cplx, time_varying, p)) return e;
  out[CPLXAMD_SSM_PGRAD_CHUNK] = p.chunk;
  out[CPLXAMD_SSM_PGRAD_TILE] = p.tile;
  out[CPLXAMD_SSM_PGRAD_TILES] = p.tiles;
  out[CPLXAMD_SSM_PGRAD_GROUP] = p.group;
  out[CPLXAMD_SSM_PGRAD_LDS_BYTES] = p.lds;
  out[CPLXAMD_SSM_PGRAD_WS_BYTES] = p.ws;
  out[CPLXAMD_SSM_PGRAD_THREADS] = p.threads;
  out[CPLXAMD_SSM_PGRAD_GRID] = p.grid;
  return 0;
}

int cplxamd_ssm_pgrad(const void* const* in, void* const* out, const cplxamd_ssm_pgrad_desc* d, int cplx, int dtype,
                      void* stream) {
  if (!in || !out || !d || (cplx != 0 && cplx != 1)) return CPLXAMD_EINVAL;
  enum { A_R, A_I, B_R, B_I, C_R, C_I, X_R, X_I, DT, H_R, H_I, G_R, G_I, F_R, F_I };
  enum { DX_R, DX_I, DA_R, DA_I, DB_R, DB_I, DC_R, DC_I, DDT, L_R, L_I, WS };
  if (!in[A_R] || !in[B_R] || !in[C_R] || !in[X_R] || !in[G_R]) return CPLXAMD_EINVAL;
  for (const int k : {A_I, B_I, C_I, X_I, H_I, G_I, F_I})
    if (!cplx && in[k]) return CPLXAMD_EINVAL;
  for (const int k : {DX_I, DA_I, DB_I, DC_I, L_I})
    if (!cplx && out[k]) return CPLXAMD_EINVAL;
  if ((in[H_I] && !in[H_R]) || (in[F_I] && !in[F_R]) || (cplx && (out[L_R] != nullptr) != (out[L_I] != nullptr))) return CPLXAMD_EINVAL;
  const int all = CPLXAMD_SSM_NEED_A | CPLXAMD_SSM_NEED_B | CPLXAMD_SSM_NEED_C | CPLXAMD_SSM_NEED_DT | CPLXAMD_SSM_NEED_X;
  if ((d->flags & ~CPLXAMD_SSM_REVERSE) != 0 || (d->need & ~all) != 0) return CPLXAMD_EINVAL;
  if ((d->a_es | d->b_es | d->c_es) < 0 || (d->a_es | d->b_es | d->c_es) > 1) return CPLXAMD_EINVAL;
  if (d->a_ns < 0 || d->b_ns < 0 || d->c_ns < 0 || d->h_ns < 0 || d->f_ns < 0) return CPLXAMD_EINVAL;
  if (in[DT] && d->a_es != 0) return CPLXAMD_EINVAL;        // exp(dt a) takes the poles: one value per state
  if ((d->need & CPLXAMD_SSM_NEED_DT) && !in[DT]) return CPLXAMD_EINVAL;
  // every gradient that is asked for has its planes
  const int bit[4] = {CPLXAMD_SSM_NEED_X, CPLXAMD_SSM_NEED_A, CPLXAMD_SSM_NEED_B, CPLXAMD_SSM_NEED_C};
  for (int k = 0; k < 4; ++k)
    if ((d->need & bit[k]) && (!out[2 * k] || (cplx && !out[2 * k + 1]))) return CPLXAMD_EINVAL;
  if ((d->need & CPLXAMD_SSM_NEED_DT) && !out[DDT]) return CPLXAMD_EINVAL;
  int64_t size[3], rows, rs[kPgPlanes][3];
  using D = cplxamd_ssm_pgrad_desc;
  const RunStride<D> f[] = {{&D::a_stride, rs[kPgA]}, {&D::b_stride, rs[kPgB]}, {&D::c_stride, rs[kPgC]},
                            {&D::x_stride, rs[kPgX]}, {&D::dt_stride, rs[kPgD]}, {&D::h_stride, rs[kPgH]},
                            {&D::g_stride, rs[kPgG]}, {&D::f_stride, rs[kPgF]}};
  if (const int e = decode_runs(*d, f, size, rows)) return e;
  const int mode = in[DT] ? kSsmDt : (d->a_es == 0 ? kSsmConst : kSsmVary);
  SsmGradPlan p;
  if (const int e = ssm_pgrad_plan_for(d->n, d->states, rows, dtype, cplx, mode != kSsmConst, p)) return e;
  if (p.grid == 0) return 0;
  if (p.ws > 0 && !out[WS]) return CPLXAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CPLXAMD_BF16)
    return pgrad_t<bf16_t>(pgrad_io<bf16_t>(in, out, *d, p.tiles, size, rs), (unsigned)p.grid, cplx != 0, mode, st);
  return pgrad_t<float>(pgrad_io<float>(in, out, *d, p.tiles, size, rs), (unsigned)p.grid, cplx != 0, mode, st);
}

}  // extern "C"
