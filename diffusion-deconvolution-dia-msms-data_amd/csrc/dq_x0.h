// The x0 estimate of one element from x_t and the (guided, rescaled) network output v under each objective, in the update's own arithmetic
// (k_update.hip): what the per-window statistics (k_winstat.hip) and the per-window form of the Solver update both call, so the quantile
// is taken over the very bits the update then clamps.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/dq_hip.h"  // DQ_PRED_*

namespace dq {

template <int PRED>
__device__ __forceinline__ float net_x0(float sa, float sb, float x, float v) {
  if (PRED == DQ_PRED_V) return sa * x - sb * v;
  if (PRED == DQ_PRED_X0) return v;
  return (x - sb * v) / sa;
}

}  // namespace dq
