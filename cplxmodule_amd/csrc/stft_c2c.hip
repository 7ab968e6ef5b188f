// The full-spectrum analysis of stft.hip -- a Cplx signal, or a real one with a null imaginary plane, framed, padded and
// windowed in the loader of the complex kernels (fft_impl.h) --, in a translation unit of its own.
#include "stft_impl.h"

namespace cplxamd {
namespace sp {

int stft_full_analysis(const void* xr, const void* xi, void* yr, void* yi, const cplxamd_stft_desc& d, int dtype,
                       const FftPlan& p, char* ws, hipStream_t st) {
  if (dtype == CPLXAMD_F64) return stft_full_analysis_t<double, double>(xr, xi, yr, yi, d, p, ws, st);
  if (dtype == CPLXAMD_BF16) return stft_full_analysis_t<bf16_t, float>(xr, xi, yr, yi, d, p, ws, st);
  return stft_full_analysis_t<float, float>(xr, xi, yr, yi, d, p, ws, st);
}

}  // namespace sp
}  // namespace cplxamd
