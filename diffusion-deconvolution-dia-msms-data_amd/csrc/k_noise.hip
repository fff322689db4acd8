// Stochastic half of the sampler: standard-normal noise from a counter-based generator evaluated inside the kernels
// (dq_philox.h), keyed by (seed, window id, element inside the window, draw index).  Seed and window ids are read from DEVICE memory, so a
// captured step is replayed unchanged under a new seed or for other windows.
//   k_randn          (B, per_window) normals of one draw index (x_T: draw 0)                                  4 B / element
// 16 B per lane, grid-stride, no LDS, like the stream kernels next door.  The stochastic update that draws from the same generator: the Sto
// family of k_update.hip.
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include <algorithm>

namespace dq {

// out[b * per + e] = z(seed, ids ? ids[b] : b, e, draw).  16-byte stores when `out` is 16-byte aligned (a lane's four elements may straddle
// two windows when per % 4 != 0: each element finds its own), scalar stores for the tail and for every other alignment.
__global__ void __launch_bounds__(256) k_randn(float* __restrict__ out, const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p,
                                               uint32_t draw, int64_t n, int64_t per) {
  const uint64_t seed = seed_p[0];
  const int64_t n4 = (((uintptr_t)out & 15) == 0) ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n4; i += stride) {
    int64_t b = (4 * i) / per, e = 4 * i - b * per;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      while (e >= per) { e -= per; ++b; }
      v[j] = philox_normal(seed, ids ? ids[b] : b, (uint32_t)e, draw);
      ++e;
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    const int64_t b = i / per;
    out[i] = philox_normal(seed, ids ? ids[b] : b, (uint32_t)(i - b * per), draw);
  }
}

int launch_randn(float* out, const int64_t* ids, const uint64_t* seed_dev, int draw, int B, int64_t per_window, hipStream_t s) {
  DQ_REQUIRE(out && seed_dev, "randn: null output or seed");
  DQ_REQUIRE(B >= 0 && per_window >= 0 && per_window <= (int64_t)0xffffffff, "randn: need B >= 0 and 0 <= per_window < 2^32");
  DQ_REQUIRE(draw >= 0, "randn: the draw index must be >= 0");
  DQ_REQUIRE(((uintptr_t)out & 3) == 0, "randn: the output must be 4-byte aligned");
  const int64_t n = (int64_t)B * per_window;
  if (n == 0) return 0;
  const int grid = (int)std::min<int64_t>(((n + 3) / 4 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_randn, dim3(grid), dim3(256), 0, s, out, ids, seed_dev, (uint32_t)draw, n, per_window);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
