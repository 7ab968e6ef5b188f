// The transform of synthesis of stft.hip -- half spectra of frames -> windowed real frames in the workspace --, in a
// translation unit of its own (the two directions compile side by side).  bf16 spectra give float32 frames: the
// overlap-add pass rounds once.
#include "stft_impl.h"

namespace cplxamd {
namespace sp {

int stft_frames(const void* xr, const void* xi, void* F, const cplxamd_stft_desc& d, int64_t r0, int64_t nr, int in_dtype,
                const RfftPlan& p, char* ws, hipStream_t st, bool build) {
  if (in_dtype == CPLXAMD_F64) return stft_frames_t<double, double>(xr, xi, (double*)F, d, r0, nr, p, ws, st, build);
  if (in_dtype == CPLXAMD_BF16) return stft_frames_t<bf16_t, float>(xr, xi, (float*)F, d, r0, nr, p, ws, st, build);
  return stft_frames_t<float, float>(xr, xi, (float*)F, d, r0, nr, p, ws, st, build);
}

}  // namespace sp
}  // namespace cplxamd
