// The complex exponential of cplx.exp's kernel (csrc/cplxfn.hip, which states its numerics) as a device function of its
// own file: csrc/ssm.hip forms exp(dt a) per step with the same code.  Include inside namespace cplxamd.
#pragma once

struct CF { float re, im; };

__device__ __forceinline__ CF f_exp(float x, float y) {
  float s, c;
  sincosf(y, &s, &c);
  if (x > 88.0f) {    // e^x overflows at 88.72, e^x cos y need not
    const float h = expf(0.5f * x);
    return {(h * c) * h, (h * s) * h};
  }
  const float e = expf(x);
  return {e * c, e * s};
}
