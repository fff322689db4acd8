// Wave-level primitives of the gfx950 kernels: ONE definition and one name each.  A kernel file includes this
// header and adds no copy or alias of its own; tests/test_wave_header.py keeps the MFMA builtins and the 4-float vector type here.
//   f32x4 / f32x16, mfma4 / mfma16 / mfma32    the three fp32 matrix instructions
//   swap_half, wave_fence                       lane ^ 32 ; ordering point of a wave-private LDS exchange
//   row_sum16, half_sum, gsum4, gmax4           reductions over a 16-lane row, a 32-lane half, the four 16-lane groups
//   LOG2E, ATT_SCALE                            log2(e), 32^-0.5
// (wave_sum / wave_max over all 64 lanes: dq_common.h, on row_sum16.  Tile-level helpers on top of these: dq_mfma.h.)
#pragma once
#include <hip/hip_runtime.h>

namespace dq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float LOG2E = 1.4426950408889634f;       // folded into the q / k projection operands: the softmaxes use exp2
constexpr float ATT_SCALE = 0.17677669529663687f;  // 32^-0.5 = dim_head^-0.5 (reference unet1d.py:481)

// v_mfma_f32_4x4x1_16b_f32: 16 independent 4x4 outer products.  Block = lane >> 2; a lane supplies A_blk[i = lane & 3] and
// B_blk[j = lane & 3]; register i of lane (blk, j) receives A_blk[i] * B_blk[j] (mapping measured: tools/probe/mfma4x4.hip).
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }
// v_mfma_f32_16x16x4_f32: A: lane l supplies A[l % 16][l / 16], B: B[l / 16][l % 16]; register r of lane (g, j) receives D[4 g + r][j]
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// v_mfma_f32_32x32x2_f32 (exact fp32): A: lane l supplies A[l & 31][l >> 5], B: B[l >> 5][l & 31]; the C/D row map: rmap, dq_mfma.h
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// value of lane ^ 32 (ds_bpermute).  gfx950's v_permlane32_swap_b32 (tools/probe/permlane32.hip) was tried here: with the
// two register copies and the select it needs it is four VALU instructions, and the VALU-bound forward kernel got 4 % slower
// (the LDS pipe that serves ds_bpermute is otherwise idle there); the latency-bound backward did not change.
__device__ __forceinline__ float swap_half(float v) { return __shfl_xor(v, 32, 64); }

// Ordering point of a wave-private LDS exchange: what this wave wrote is visible to its own lanes, and the compiler moves no LDS
// access across it.  No other wave is waited for.
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// sum over the 16 lanes of a row (every lane receives it): four DPP adds, no LDS
__device__ __forceinline__ float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));  // row_mirror
  return v;
}
// sum over the 32 lanes that share (lane >> 5): the row sums, then the two rows of a half meet through v_readlane (no LDS round trips)
__device__ __forceinline__ float half_sum(float v) {
  const int x = __float_as_int(row_sum16(v));
  const float lo = __int_as_float(__builtin_amdgcn_readlane(x, 0)) + __int_as_float(__builtin_amdgcn_readlane(x, 16));
  const float hi = __int_as_float(__builtin_amdgcn_readlane(x, 32)) + __int_as_float(__builtin_amdgcn_readlane(x, 48));
  return (threadIdx.x & 32) ? hi : lo;
}
// sum / maximum over the four lane groups (lanes j, j + 16, j + 32, j + 48; every lane receives it), all VALU: v_permlane16_swap
// (rows 0 <-> 1, 2 <-> 3), then v_permlane32_swap (halves) (tools/probe/blocks_sum.hip pins the semantics)
__device__ __forceinline__ float gsum4(float t) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_int(t), __float_as_int(t), false, false);
  t = __int_as_float(a[0]) + __int_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_int(t), __float_as_int(t), false, false);
  return __int_as_float(b[0]) + __int_as_float(b[1]);
}
__device__ __forceinline__ float gmax4(float t) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_int(t), __float_as_int(t), false, false);
  t = fmaxf(__int_as_float(a[0]), __int_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_int(t), __float_as_int(t), false, false);
  return fmaxf(__int_as_float(b[0]), __int_as_float(b[1]));
}

}  // namespace dq
