// Classifier-free guidance inside the update kernels: the guided network output of one element,
//   g = u + w * (c - u)
// from the conditional output c and the unconditional output u, in fp32: one subtraction, then ONE fused multiply-add (fmaf is asked for
// by name; the library is built with -ffp-contract=off, so the compiler contracts nothing on its own and nothing else in the update
// changes).  c == u gives g == u exactly for every finite w (w * 0 + u), w == 0 gives u, w == 1 gives c up to the rounding of (c - u) + u.
// The update kernel (k_step_update, k_update.hip) runs its arithmetic on g in place of the network output, for both
// objectives: guidance commutes with the affine map between eps and x0.
#pragma once
#include <hip/hip_runtime.h>

namespace dq {

__device__ __forceinline__ float guide(float c, float u, float w) { return fmaf(w, c - u, u); }

}  // namespace dq
