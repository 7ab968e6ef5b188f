// The full-spectrum transform of synthesis of stft.hip -- full spectra of frames -> windowed complex frames in the two
// planes of the workspace (the window in the store of the complex kernels, fft_impl.h) --, in a translation unit of its
// own.  bf16 spectra give float32 frames: the overlap-add pass rounds once.
#include "stft_impl.h"

namespace cplxamd {
namespace sp {

int stft_full_frames(const void* xr, const void* xi, void* Fr, void* Fi, const cplxamd_stft_desc& d, int64_t r0, int64_t nr,
                     int in_dtype, const FftPlan& p, char* ws, hipStream_t st, bool build) {
  if (in_dtype == CPLXAMD_F64)
    return stft_full_frames_t<double, double>(xr, xi, (double*)Fr, (double*)Fi, d, r0, nr, p, ws, st, build);
  if (in_dtype == CPLXAMD_BF16)
    return stft_full_frames_t<bf16_t, float>(xr, xi, (float*)Fr, (float*)Fi, d, r0, nr, p, ws, st, build);
  return stft_full_frames_t<float, float>(xr, xi, (float*)Fr, (float*)Fi, d, r0, nr, p, ws, st, build);
}

}  // namespace sp
}  // namespace cplxamd
