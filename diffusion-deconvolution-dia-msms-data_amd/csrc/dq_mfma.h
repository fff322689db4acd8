// 32x32 tile helpers shared by the LinearAttention and bottleneck-attention kernels, on the wave primitives of dq_wave.h (mfma32 =
// v_mfma_f32_32x32x2_f32, exact fp32; and the split-bf16 form on v_mfma_f32_32x32x16_bf16 at the end of the file).
//   A operand: lane l supplies A[i = l & 31][k = l >> 5] ; B operand: lane l supplies B[k = l >> 5][j = l & 31]
//   C/D: register r of lane l holds D[row = rmap(r, l >> 5)][col = l & 31]
// An accumulator X (rows in registers, column on the lane) feeds, register by register, a product that sums over X's
// ROW index:  sum_r mfma(X.r, Y.r) = X^T Y  with rows = X's columns, cols = Y's columns.
#pragma once
#include <hip/hip_runtime.h>
#include "dq_wave.h"

namespace dq {

__device__ __forceinline__ constexpr int rmap(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// Which channel x-register j of a lane of half `half` holds in the LinearAttention kernels, and how many such registers a lane
// has.  C = 8 / 16: the accumulator row map (8 / 16 channel slots, all used).  C = 4: c = 2 * half + j over TWO registers, C = 12:
// c = 6 * half + j over SIX -- with the row map the lanes of half 1 would hold channels 4..7 (C = 4) resp. four of the sixteen slots
// would be empty (C = 12), i.e. part of every K = 2 slice of a 32x32x2 product would be zero padding: four MFMAs per K = 4
// projection instead of two, eight per K = 12 projection instead of six.
__host__ __device__ __forceinline__ constexpr int la_nj(int C) { return C == 4 ? 2 : (C == 12 ? 6 : (C <= 8 ? 4 : 8)); }
__device__ __forceinline__ constexpr int la_chan(int C, int j, int half) {
  return C == 4 ? 2 * half + j : (C == 12 ? 6 * half + j : rmap(j, half));
}
// k_la_small: the channel that half `half` supplies in K-step i of a projection (C / 2 steps).  C = 8 / 16: the accumulator row map, so
// that a projection operand register IS the residual / output register of the same index; C = 12: i + 6 half (six full steps instead of
// eight with a third of the slots empty; the residual is then read a second time in the row-map layout).
__host__ __device__ __forceinline__ constexpr int sm_chan(int C, int i, int half) { return C == 12 ? i + 6 * half : (i & 3) + 8 * (i >> 2) + 4 * half; }
// The LinearAttention backward kernels' operand helpers (k_la_bwd.h, k_la_long.hip).
// This lane's operand slice of a per-position / per-d channel vector: v[c = la_chan(C, j, half)] (zero beyond C)
template <int C>
__device__ __forceinline__ float own_of(const float (&v)[C], int j, int half) {
  const int c0 = la_chan(C, j, 0), c1 = la_chan(C, j, 1);
  const float lo = c0 < C ? v[c0 < C ? c0 : 0] : 0.f, hi = c1 < C ? v[c1 < C ? c1 : 0] : 0.f;
  return half ? hi : lo;
}
// sum_r mfma4(A = src[(4*g + (lane&3)) * pitch + off + rmap(r, half)], B = t[r]) on two interleaved accumulator chains (a
// dependent 4x4x1 MFMA issues every ~14.5 cycles, independent ones every ~8.5)
__device__ __forceinline__ f32x4 chain4(const float* src, int pitch, int off, int g, const f32x16& t, int lane, int half) {
  const float* ar = src + (g * 4 + (lane & 3)) * pitch + off + 4 * half;
  f32x4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const float4 a4 = *reinterpret_cast<const float4*>(ar + 8 * q4);
    t0 = mfma4(a4.x, t[q4 * 4 + 0], t0); t1 = mfma4(a4.y, t[q4 * 4 + 1], t1);
    t0 = mfma4(a4.z, t[q4 * 4 + 2], t0); t1 = mfma4(a4.w, t[q4 * 4 + 3], t1);
  }
  return t0 + t1;
}

// X^T Y over all 16 registers
__device__ __forceinline__ f32x16 xty(const f32x16& x, const f32x16& y, f32x16 acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc = mfma32(x[r], y[r], acc);
  return acc;
}

// ---- 32x32 transposes of an accumulator tile through a wave-private LDS tile: two layouts, the row pitch in the name.
// Pitch 33, [32][33] (conflict-free both ways), in two halves: the tile is put down where its registers end their life and taken up,
// transposed, where the transposed form is first needed
__device__ __forceinline__ void transpose_put33(const f32x16& a, float* tile, int col, int half) {
  wave_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[rmap(r, half) * 33 + col] = a[r];
}
__device__ __forceinline__ f32x16 transpose_get33(const float* tile, int col, int half) {
  wave_fence();
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = tile[col * 33 + rmap(r, half)];
  return o;
}
__device__ __forceinline__ f32x16 transpose_tile33(f32x16 a, float* tile, int col, int half) {
  transpose_put33(a, tile, col, half);
  return transpose_get33(tile, col, half);
}
// Pitch 36, [32][TRP36]: written as 16 dwords per lane (a row's 32 lanes are consecutive: conflict-free), read back as FOUR 16-byte
// reads -- registers 4 q .. 4 q + 3 are rows 8 q + 4 half .. + 3 of the transposed tile, consecutive in memory; the row pitch of 36
// floats keeps them 16-byte aligned and spreads a 16-lane phase over all 64 banks (36 col mod 64 takes every multiple of 4 once).
// With pitch 33 the reads are eight ds_read2_b32 per transpose.
constexpr int TRP36 = 36;
__device__ __forceinline__ f32x16 transpose_tile36(f32x16 a, float* tile, int col, int half) {
  wave_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[rmap(r, half) * TRP36 + col] = a[r];
  wave_fence();
  f32x16 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(tile + col * TRP36 + 8 * q + 4 * half);
    o[4 * q + 0] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
  }
  return o;
}

// keep element (row in registers, column on the lane) only where row / N == col / N  (pairs inside one m/z row)
template <int N>
__device__ __forceinline__ f32x16 mask_same_row(f32x16 a, int col, int half) {
  const int cr = col / N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rr = half ? rmap(r, 1) / N : rmap(r, 0) / N;
    a[r] = rr == cr ? a[r] : 0.f;
  }
  return a;
}

// ---- split-bf16: an fp32 value is EXACTLY the sum of three bf16 values (H = bf16(v), M = bf16(v - H), L = v - H - M: 8 + 8 + 8
// significant bits), so a product x y is the sum of nine part products, each exact in fp32.  The six at or above 2^-16 of the largest -- HH,
// HM, MH, MM, HL, LH -- are kept; the three dropped ones (ML, LM, LL) are < 2^-23 of |x||y| together in the worst case: a few fp32
// roundings.  v_mfma_f32_32x32x16_bf16 (32 cycles for K = 16) accumulates in fp32.
//   A operand: element j (0..7) of lane l is A[i = l & 31][k = 8 (l >> 5) + j] ; B operand: B[k = 8 (l >> 5) + j][n = l & 31] ; C/D as above
//   (tools/probe/mfma32x32x16_bf16.hip pins the map and the chaining below with exact integer data).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { union { u32x4 u; bf16x8 b; } c; c.u = v; return c.b; }
__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0); }

// A 32 x 32 tile (rows in the 16 registers of a lane, column on the lane) as the operand of a product that sums over its ROW index: registers
// 8 s .. 8 s + 7 are the lane's eight K elements of K-step s (s = 0, 1), i.e. K slot (s, half, j) is row rmap(8 s + j, half) -- the same
// permutation of the 32 rows for every tile in this layout, so two such tiles multiply slot by slot.  Three planes of 2 x 4 dwords.
struct Split16 { u32x4 h[2], m[2], l[2]; };
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// The parts are ROUNDED to nearest (v_cvt_pk_bf16_f32, two values per instruction): |M| <= 2^-9 and |L| <= 2^-17 of the value's binade with
// either sign, so the dropped terms are a quarter of what truncated parts would leave and do not lean one way.  Every subtraction is exact.
__device__ __forceinline__ Split16 split_tile(const f32x16& x) {
  Split16 t;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int p = 0; p < 4; ++p) {  // 9 vector instructions per two values: 3 conversions, 4 unpacks, 2 v_pk_add_f32
      const f32x2 v = {x[8 * s + 2 * p], x[8 * s + 2 * p + 1]};
      const bf16x2 h = __builtin_convertvector(v, bf16x2);
      const f32x2 r = v - __builtin_convertvector(h, f32x2);
      const bf16x2 m = __builtin_convertvector(r, bf16x2);
      const bf16x2 l = __builtin_convertvector(r - __builtin_convertvector(m, f32x2), bf16x2);  // exact: <= 8 significant bits are left
      t.h[s][p] = __builtin_bit_cast(unsigned, h);  // low half = the first value
      t.m[s][p] = __builtin_bit_cast(unsigned, m);
      t.l[s][p] = __builtin_bit_cast(unsigned, l);
    }
  return t;
}
// X^T Y of two split tiles, six terms x two K-steps, the small terms first: twelve dependent 32-cycle MFMAs (sixteen of 64 cycles in xty).
// MIRROR swaps the roles of x and y in the order of the terms, so that xty6<true>(y, x) adds the same part products in the same order as
// xty6(x, y) and is its transpose BIT FOR BIT: the backward kernels recompute the forward's scores, and P = exp(S - lse) is only as good as
// the two evaluations of S agree (one ulp of a score of 2^20 is a factor of e^(1/8) in P).
template <bool MIRROR = false>
__device__ __forceinline__ f32x16 xty6(const Split16& x, const Split16& y, f32x16 acc) {
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = MIRROR ? mfma_bf16(x.h[s], y.l[s], acc) : mfma_bf16(x.l[s], y.h[s], acc);
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = MIRROR ? mfma_bf16(x.l[s], y.h[s], acc) : mfma_bf16(x.h[s], y.l[s], acc);
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = mfma_bf16(x.m[s], y.m[s], acc);
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = MIRROR ? mfma_bf16(x.h[s], y.m[s], acc) : mfma_bf16(x.m[s], y.h[s], acc);
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = MIRROR ? mfma_bf16(x.m[s], y.h[s], acc) : mfma_bf16(x.h[s], y.m[s], acc);
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = mfma_bf16(x.h[s], y.h[s], acc);
  return acc;
}

}  // namespace dq
