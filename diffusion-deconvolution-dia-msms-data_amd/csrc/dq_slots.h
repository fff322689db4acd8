// The ordered slot sum of the parameter gradients: ONE definition.  A producer kernel leaves its partial sums in a
// "slot" of its own with plain stores; a reduce kernel adds the slots of an element up in the order fixed here.  No float atomics, so every
// gradient is repeatable to the bit -- and the ORDER is a contract (the data-parallel test, the repeatability tests and the parity dumps
// under profiles/ compare bits), not a detail of one kernel.
//
// A reduce workgroup owns EL consecutive elements x G slot groups (EL * G = 256 threads: el = thread % EL, g = thread / EL):
//   slot_sum<G, DEEP>   group g's share of one element: two accumulators from 0; slots g, g + 2G, g + 4G, ... go into s0 in ascending
//                       order, slots g + G, g + 3G, ... into s1 in ascending order, a trailing unpaired slot into s0; the share is s0 + s1.
//                       DEEP only puts eight loads in flight and adds them in exactly the order of the two-at-a-time loop: the same sums
//                       bit for bit, a quarter of the memory round trips.
//   slot_meet<EL, G>    the G shares of an element meet in LDS: group 0 returns ((0 + red[0][el]) + red[1][el]) + ... in group order.
// The producers' side:
//   slot_wave_sums<C>   four per-channel accumulator sets, each summed over the wave (wave_sum), into red[wv][q * C + c]; barrier
//   over_waves4         (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]): the four waves of a 256-thread workgroup, in this order
#pragma once
#include "dq_common.h"

namespace dq {

// slot b of element e: part[b * stride + e]
template <int G, bool DEEP>
__device__ __forceinline__ float slot_sum(const float* part, int e, int stride, int cnt, int g) {
  float s0 = 0.f, s1 = 0.f;
  int b = g;
  if (DEEP) {
    for (; b + 7 * G < cnt; b += 8 * G) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(b + G * u) * stride + e];
#pragma unroll
      for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
    }
  }
  for (; b + G < cnt; b += 2 * G) {
    s0 += part[(int64_t)b * stride + e];
    s1 += part[(int64_t)(b + G) * stride + e];
  }
  if (b < cnt) s0 += part[(int64_t)b * stride + e];
  return s0 + s1;
}

// every thread of the workgroup calls it (a barrier inside); v = 0 for an element out of range.  The total is group 0's; the rest get 0.
template <int EL, int G>
__device__ __forceinline__ float slot_meet(float (&red)[G][EL + 1], float v, int g, int el) {
  red[g][el] = v;
  __syncthreads();
  float s = 0.f;
  if (g == 0) {
#pragma unroll
    for (int k = 0; k < G; ++k) s += red[k][el];
  }
  return s;
}

// red: float[waves][values]; waves w0 .. w0 + 3
template <typename RED>
__device__ __forceinline__ float over_waves4(const RED& red, int i, int w0 = 0) {
  return (red[w0][i] + red[w0 + 1][i]) + (red[w0 + 2][i] + red[w0 + 3][i]);
}
template <int C, typename RED>
__device__ __forceinline__ void slot_wave_sums(RED& red, const float (&a0)[C], const float (&a1)[C], const float (&a2)[C], const float (&a3)[C],
                                               int lane, int wv) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float s0 = wave_sum(a0[c]), s1 = wave_sum(a1[c]), s2 = wave_sum(a2[c]), s3 = wave_sum(a3[c]);
    if (lane == 0) { red[wv][c] = s0; red[wv][C + c] = s1; red[wv][2 * C + c] = s2; red[wv][3 * C + c] = s3; }
  }
  __syncthreads();
}

}  // namespace dq
