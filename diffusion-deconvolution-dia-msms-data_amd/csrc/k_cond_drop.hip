// Conditioning dropout for classifier-free guidance: while training, the MS1 condition of a window is replaced as a
// whole by the constant `null_value` with probability p, so that the network also learns the unconditional output the guided sampler
// combines with the conditional one.
//   k_cond_drop  out (B, per) = window b of `in`, or null_value in every element iff r2 < thresh                    8 B / element
// r2 is the THIRD output word of philox4x32_10 (dq_philox.h) on counter (0, draw, id lo, id hi) under key (seed lo, seed hi), id = ids ?
// ids[b] : b.  The normals of philox_normal use words 0 and 1 only, so the decision never correlates with a noise draw under the same seed,
// whatever the element and draw index.  thresh = (uint32) floor(p * 2^32) is formed on the host in double (0 <= p < 1; p == 0: thresh 0,
// nothing is ever dropped).  A kept window is a bit copy.  The seed is read from DEVICE memory like k_randn's; a window decides alone, from
// its id, wherever it sits in a batch.
// 16-byte accesses when both pointers are 16-byte aligned (a lane's four elements may straddle windows when per % 4 != 0: each element
// finds its own, one Philox evaluation per window a lane touches), one element per lane for the tail and for every other alignment.
// Element-wise and out of place: `out` may alias `in` (a lane reads its elements before it writes them; no __restrict__ on the two).
// Grid-stride, no LDS, no atomics, like the stream kernels next door.
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include <algorithm>
#include <cmath>

namespace dq {

__device__ __forceinline__ bool cond_dropped(uint64_t seed, int64_t id, uint32_t draw, uint32_t thresh) {
  uint32_t c0 = 0u, c1 = draw, c2 = (uint32_t)((uint64_t)id & 0xffffffffu), c3 = (uint32_t)((uint64_t)id >> 32);
  philox4x32_10(c0, c1, c2, c3, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  return c2 < thresh;
}

__global__ void __launch_bounds__(256) k_cond_drop(const float* in, float* out, const int64_t* __restrict__ ids,
                                                   const uint64_t* __restrict__ seed_p, uint32_t draw, uint32_t thresh, float null_value,
                                                   int64_t n, int64_t per) {
  const uint64_t seed = seed_p[0];
  const int64_t n4 = ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(in)[i];
    float vv[4] = {v.x, v.y, v.z, v.w};
    int64_t b = (4 * i) / per, e = 4 * i - b * per;
    bool drop = cond_dropped(seed, ids ? ids[b] : b, draw, thresh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e >= per) { e -= per; ++b; drop = cond_dropped(seed, ids ? ids[b] : b, draw, thresh); }  // (per >= 1: one window further at most)
      if (drop) vv[j] = null_value;
      ++e;
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(vv[0], vv[1], vv[2], vv[3]);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    const int64_t b = i / per;
    const float v = in[i];
    out[i] = cond_dropped(seed, ids ? ids[b] : b, draw, thresh) ? null_value : v;
  }
}

int launch_cond_drop(const float* in, float* out, const int64_t* ids, const uint64_t* seed_dev, int draw, double p, float null_value, int B,
                     int64_t per, hipStream_t s) {
  DQ_REQUIRE(in && out && seed_dev, "cond_drop: null argument");
  DQ_REQUIRE(p >= 0.0 && p < 1.0, "cond_drop: the drop probability must satisfy 0 <= p < 1");  // (false for NaN)
  DQ_REQUIRE(draw >= 0, "cond_drop: the draw index must be >= 0");
  DQ_REQUIRE(B >= 0 && per >= 0, "cond_drop: negative size");
  DQ_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "cond_drop: tensors must be 4-byte aligned");
  const int64_t n = (int64_t)B * per;
  if (n == 0) return 0;
  const uint32_t thresh = (uint32_t)std::floor(p * 4294967296.0);  // (p < 1 in double: below 2^32)
  const int grid = (int)std::min<int64_t>(((n + 3) / 4 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_cond_drop, dim3(grid), dim3(256), 0, s, in, out, ids, seed_dev, (uint32_t)draw, thresh, null_value, n, per);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
