// Counter-based noise for the stochastic sampler: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as
// 1, 2, 3", SC'11; the Random123 constants) and one standard normal per counter by Box-Muller.  Plain C++: no inline assembly, no LDS, no
// cooperation between lanes -- a lane computes the normal of its own element from (seed, window id, element, draw index) alone, so a window
// draws the same noise wherever it sits in a batch and a captured step never changes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dq {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;  // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;  // Weyl increments of the key

// the ten rounds on counter (c0, c1, c2, c3) under key (k0, k1); the counter words are replaced by the output words
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
}

// z ~ N(0, 1) of element `e` of window `w` at draw index `d` under `seed`: counter (e, d, w lo, w hi), key (seed lo, seed hi); output words
// r0, r1 -> u1 = ((r0 >> 9) + 0.5) 2^-23 in (0, 1) and u2 = (r1 >> 8) 2^-24 in [0, 1), both exact in fp32; r2, r3 unused
__device__ __forceinline__ float philox_normal(uint64_t seed, int64_t w, uint32_t e, uint32_t d) {
  uint32_t c0 = e, c1 = d, c2 = (uint32_t)((uint64_t)w & 0xffffffffu), c3 = (uint32_t)((uint64_t)w >> 32);
  philox4x32_10(c0, c1, c2, c3, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  const float u1 = ((float)(c0 >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23
  const float u2 = (float)(c1 >> 8) * 5.9604644775390625e-08f;           // 2^-24
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

}  // namespace dq
