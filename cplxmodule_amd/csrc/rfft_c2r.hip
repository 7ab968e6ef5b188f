// The half spectrum -> real direction of rfft.hip, in a translation unit of its own (the two directions compile side by
// side).
#include "rfft_impl.h"

namespace cplxamd {
namespace sp {
template int rfft_any<true>(const void*, const void*, void*, void*, const cplxamd_fft_desc&, int, int, const Batch&, const RfftPlan&,
                            char*, hipStream_t);
}  // namespace sp
}  // namespace cplxamd
