// Host-side launch plan shared by conv_cl_wgrad.hip and its real-valued twin conv_cl_wgrad_real.hip.
#pragma once
#include "launch.h"

namespace cplxamd {

// Splits of the pixel loop (returned) and stages per split.  shared: the chip is shared with RCCL collectives
// (CPLXAMD_LAUNCH_SHARED): twice as many, half as long splits, so that the workgroups that find their CU taken do not make
// the launch take two rounds (the workspace is always sized for this plan)
inline int clw_plan(int64_t nstages, int tiles, int& per_split, bool shared) {
  const int ncu = device_cus();
  int64_t s = ncu / tiles;                            // one workgroup per CU (120 KiB of LDS each), one round
  if (s < 1) s = 1;
  if (shared) s *= 2;
  const int64_t maxs = (nstages + 15) / 16;           // >= 16 stages per split
  if (s > maxs) s = maxs;
  per_split = (int)((nstages + s - 1) / s);
  return (int)((nstages + per_split - 1) / per_split);
}

}  // namespace cplxamd
