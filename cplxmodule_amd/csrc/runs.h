// The batch runs of the signal kernels (fft, rfft, fftconv, upfirdn, iir, filtfilt): the one decoder of a descriptor's
// runs, the choice of runs by a key stride, and the three-run form that travels as a kernel argument.  The host side
// that fuses dims into runs and fills the descriptors is cplxmodule_amd/_runs.py.
#pragma once
#include "common.h"

namespace cplxamd {
namespace sp {

// one stride array of a descriptor and where its three right-aligned values go
template <typename D>
struct RunStride {
  int64_t (D::*from)[3];
  int64_t* to;
};
// The runs of descriptor d, right-aligned (run 2 innermost): sizes into size (unused: 1), every stride array of f into
// its destination (unused: 0), the product of the sizes into rows.  A run count outside 0 .. 3 and a negative size
// are CPLXAMD_EINVAL, and so is a negative stride unless `any_stride`; a product beyond 64 bits is CPLXAMD_ESHAPE.
template <typename D, int N>
inline int decode_runs(const D& d, const RunStride<D> (&f)[N], int64_t (&size)[3], int64_t& rows, bool any_stride = false) {
  if (d.runs < 0 || d.runs > 3) return CPLXAMD_EINVAL;
  rows = 1;
  for (int s = 0; s < 3; ++s) {
    size[s] = 1;
    for (const RunStride<D>& x : f) x.to[s] = 0;
  }
  for (int q = 0; q < d.runs; ++q) {
    const int s = 3 - d.runs + q;
    if (d.size[q] < 0) return CPLXAMD_EINVAL;
    size[s] = d.size[q];
    for (const RunStride<D>& x : f) {
      if (!any_stride && (d.*x.from)[q] < 0) return CPLXAMD_EINVAL;
      x.to[s] = (d.*x.from)[q];
    }
    if (__builtin_mul_overflow(rows, d.size[q], &rows)) return CPLXAMD_ESHAPE;
  }
  return 0;
}

// ---- the batch: three runs, right-aligned (unused ones have size 1 and stride 0) -----------------------------------------
struct ConvRuns {
  int64_t rows, size[3], as[3], bs[3], ys[3];
};
// the runs (of more than one row) whose `key` stride is non-zero (`want`) or zero, right-aligned into sel (-1: none);
// returns the product of their sizes
inline int64_t select_runs(const ConvRuns& r, const int64_t* key, bool want, int (&sel)[3]) {
  int n = 0, tmp[3];
  int64_t count = 1;
  for (int s = 0; s < 3; ++s)
    if (r.size[s] != 1 && (key[s] != 0) == want) {
      tmp[n++] = s;
      count *= r.size[s];
    }
  for (int s = 0; s < 3; ++s) sel[s] = s >= 3 - n ? tmp[s - (3 - n)] : -1;
  return count;
}
// three runs of a kernel argument: sizes of runs 1 and 2, two strides per run
struct Sub {
  int64_t s1, s2, p[3], q[3];
};
inline Sub sub_runs(const ConvRuns& r, const int (&sel)[3], const int64_t* p, const int64_t* q) {
  Sub o{1, 1, {0, 0, 0}, {0, 0, 0}};
  for (int s = 0; s < 3; ++s)
    if (sel[s] >= 0) {
      o.p[s] = p[sel[s]];
      o.q[s] = q[sel[s]];
      if (s == 1) o.s1 = r.size[sel[s]];
      if (s == 2) o.s2 = r.size[sel[s]];
    }
  return o;
}
__device__ __forceinline__ void sub_offsets(const Sub& b, int64_t v, int64_t& po, int64_t& qo) {
  const int64_t i2 = v % b.s2, w = v / b.s2, i1 = w % b.s1, i0 = w / b.s1;
  po = i0 * b.p[0] + i1 * b.p[1] + i2 * b.p[2];
  qo = i0 * b.q[0] + i1 * b.q[1] + i2 * b.q[2];
}

}  // namespace sp
}  // namespace cplxamd
