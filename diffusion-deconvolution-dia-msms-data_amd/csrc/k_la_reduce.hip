// The slot reduction of the LinearAttention backward.  Every backward form -- the register-resident kernels (k_la_bwd.h, k_la_bwd1.h), the
// row form (k_la_rows_bwd.hip), the fused tiny levels (k_tiny.hip) and the sweep kernel of long rows (k_la_long.hip) -- leaves its parameter
// gradients in partial slots (plain stores); the kernels here sum the slots in a fixed order: no atomics, bitwise repeatable.
//   k_linattn_dw_reduce         slots of the sweep kernel (512 C floats: dWqkv | dWo)
//   k_linattn_dw_reduce_multi   slots in the la_slot(C) layout (dq_kernels.h), several layers in one launch
//   k_linattn_dwvo              dWv = Wo^T dW2, dWo = dW2 Wv^T from the summed dW2, once per layer
#include "dq_common.h"
#include "dq_kernels.h"

namespace dq {

// grad[e] += sum over the wave slots in a fixed order (deterministic).  A block owns 16 consecutive elements x 16 slot
// groups: thread (e, g) sums slots g, g+16, g+32, ... (64-byte segments per group: every fetched sector is fully used, unlike
// a lane-per-slot gather), the 16 group sums meet in LDS.
// Slot layout: dWqkv (384C) | dWo (128C) [| d g_out (C) | d b_out (C) | d g_pre (C) when nelem == 515C]
__global__ void __launch_bounds__(256) k_linattn_dw_reduce(const float* __restrict__ part, int nslots, int C, int nelem,
                                                           float* __restrict__ dw_qkv, float* __restrict__ dw_out,
                                                           float* __restrict__ dg_out, float* __restrict__ db_out,
                                                           float* __restrict__ dg_pre) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  float s0 = 0.f, s1 = 0.f;
  if (e < nelem) {
    int b = g;
    // (eight loads in flight, added in the order of the two-at-a-time loop: same sums bit for bit, a quarter of the memory round trips)
    for (; b + 112 < nslots; b += 128) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(b + 16 * u) * nelem + e];
#pragma unroll
      for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
    }
    for (; b + 16 < nslots; b += 32) {
      s0 += part[(int64_t)b * nelem + e];
      s1 += part[(int64_t)(b + 16) * nelem + e];
    }
    if (b < nslots) s0 += part[(int64_t)b * nelem + e];
  }
  red[g][el] = s0 + s1;
  __syncthreads();
  if (g == 0 && e < nelem) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][el];
    if (e < 384 * C) dw_qkv[e] += s;
    else if (e < 512 * C) dw_out[e - 384 * C] += s;
    else if (e < 513 * C) dg_out[e - 512 * C] += s;
    else if (e < 514 * C) db_out[e - 513 * C] += s;
    else dg_pre[e - 514 * C] += s;
  }
}
// The slot reduction of the register-resident backward (slot layout la_slot(C)), for several LinearAttention layers at once: block ->
// (item, 16-element group) through a prefix table.  dWq | dWk and the gains go to the gradient buffers (+=); the summed dW2 of the four
// heads goes to the item's w2sum scratch, from which k_linattn_dwvo forms dWv and dWo.
struct LaReduceMulti { LaReduceItem it[LA_REDUCE_MAX]; int first_block[LA_REDUCE_MAX + 1]; int count; };
__global__ void __launch_bounds__(256) k_linattn_dw_reduce_multi(LaReduceMulti m) {
  int i = 0;
  while (i + 1 < m.count && (int)blockIdx.x >= m.first_block[i + 1]) ++i;
  const LaReduceItem& it = m.it[i];
  const int C = it.C, nelem = la_slot(C), nslots = it.nslots;
  const float* __restrict__ part = it.part;
  // 32 consecutive elements x 8 slot groups per block: a half-wave reads one whole 128-byte line of a slot.  (With 16 elements x 16 groups
  // every access was half a line -- the launch reads ~45 MB of slots per train step and ran at the rate of twice that, 28 us.)
  __shared__ float red[8][33];
  const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int e = ((int)blockIdx.x - m.first_block[i]) * 32 + el;
  float s0 = 0.f, s1 = 0.f;
  if (e < nelem) {
    int b = g;
    for (; b + 56 < nslots; b += 64) {  // eight loads in flight, added in a fixed order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(b + 8 * u) * nelem + e];
#pragma unroll
      for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
    }
    for (; b + 8 < nslots; b += 16) {
      s0 += part[(int64_t)b * nelem + e];
      s1 += part[(int64_t)(b + 8) * nelem + e];
    }
    if (b < nslots) s0 += part[(int64_t)b * nelem + e];
  }
  red[g][el] = s0 + s1;
  __syncthreads();
  if (g == 0 && e < nelem) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[k][el];
    const int w2b = 256 * C, gb = w2b + 4 * C * C;
    if (e < w2b) it.dw_qkv[e] += s;                 // rows 0..255 of to_qkv: q | k
    else if (e < gb) it.w2sum[e - w2b] = s;         // dW2[head][c'][c]
    else if (e < gb + C) it.dg_out[e - gb] += s;
    else if (e < gb + 2 * C) it.db_out[e - gb - C] += s;
    else it.dg_pre[e - gb - 2 * C] += s;
  }
}
// dWv[e][c] += sum_c' Wo[c'][e] dW2[h(e)][c'][c] ; dWo[c'][e] += sum_c dW2[h(e)][c'][c] Wv[e][c]   (e = head * 32 + d: the 128 value /
// output channels; W2_h = Wo_h Wv_h).  One block per (layer, head); the head's dW2 and weight slices in LDS (as
// one block per layer with every operand read from memory in a runtime-length loop this was 42 us at the end of the backward).
__global__ void __launch_bounds__(256) k_linattn_dwvo(LaReduceMulti m) {
  const LaReduceItem& it = m.it[blockIdx.x];
  const int C = it.C, hd = blockIdx.y;
  __shared__ float w2[16 * 16], wo[16 * 32], wv[32 * 16];  // dW2_h [c'][c] ; Wo[c'][e = hd*32 + d] as [c'][d] ; Wv[e][c] as [d][c]
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) w2[i] = it.w2sum[hd * C * C + i];
  for (int i = threadIdx.x; i < 32 * C; i += blockDim.x) {
    wo[i] = it.w_out[(i >> 5) * 128 + hd * 32 + (i & 31)];
    wv[i] = it.w_qkv[(256 + hd * 32) * C + i];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 32 * C; idx += blockDim.x) {
    const int d = idx / C, c = idx - d * C, e = hd * 32 + d;
    float sv = 0.f, so = 0.f;
    for (int k = 0; k < C; ++k) {
      sv = fmaf(wo[k * 32 + d], w2[k * C + c], sv);   // k = c'
      so = fmaf(w2[c * C + k], wv[d * C + k], so);    // row c' = c of dW2, k = c
    }
    it.dw_qkv[(256 + e) * C + c] += sv;
    it.dw_out[c * 128 + e] += so;
  }
}

// one slot per wave of a resident round + the summed dW2
int64_t la_part_reserve(int C) { return ((int64_t)(C <= 8 ? 2048 : 1024) * la_slot(C) + 4 * C * C + 63) / 64 * 64; }
int launch_linattn_dw_reduce_multi(const LaReduceItem* items, int count, hipStream_t s) {
  if (count == 0) return 0;
  DQ_REQUIRE(count <= LA_REDUCE_MAX, "linattn dw reduce: too many deferred layers");
  LaReduceMulti m;
  m.count = count;
  int blocks = 0;
  for (int i = 0; i < count; ++i) {
    m.it[i] = items[i];
    m.first_block[i] = blocks;
    blocks += cdiv(la_slot(items[i].C), 32);
  }
  m.first_block[count] = blocks;
  hipLaunchKernelGGL(k_linattn_dw_reduce_multi, dim3(blocks), dim3(256), 0, s, m);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_linattn_dwvo, dim3(count, 4), dim3(256), 0, s, m);
  DQ_LAUNCH_CHECK();
  return 0;
}
// the slots of the sweep kernel (rows longer than 64 positions: 512 C floats per wave, dWqkv | dWo)
int launch_linattn_dw_reduce(const float* part, int nslots, int C, float* dw_qkv, float* dw_out, hipStream_t s) {
  hipLaunchKernelGGL(k_linattn_dw_reduce, dim3(cdiv(512 * C, 16)), dim3(256), 0, s, part, nslots, C, 512 * C, dw_qkv, dw_out,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
