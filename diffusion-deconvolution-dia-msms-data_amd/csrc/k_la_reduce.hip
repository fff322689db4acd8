// The slot reduction of the LinearAttention backward.  Every backward form -- the register-resident kernels (k_la_bwd.h, k_la_bwd1.h), the
// row form (k_la_rows_bwd.hip), the fused tiny levels (k_tiny.hip) and the sweep kernel of long rows (k_la_long.hip) -- leaves its parameter
// gradients in partial slots (plain stores); the kernels here sum the slots in a fixed order: no atomics, bitwise repeatable.
//   k_linattn_dw_reduce         slots of the sweep kernel (512 C floats: dWqkv | dWo)
//   k_linattn_dw_reduce_multi   slots in the la_slot(C) layout (dq_kernels.h), several layers in one launch
//   k_linattn_dwvo              dWv = Wo^T dW2, dWo = dW2 Wv^T from the summed dW2, once per layer
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_slots.h"

namespace dq {

// grad[e] += the ordered sum of the wave slots (dq_slots.h).  A block owns 16 consecutive elements x 16 slot groups: thread (e, g) takes
// slots g, g+16, g+32, ... (64-byte segments per group: every fetched sector is fully used, unlike a lane-per-slot gather).
// Slot layout: dWqkv (384C) | dWo (128C)
__global__ void __launch_bounds__(256) k_linattn_dw_reduce(const float* __restrict__ part, int nslots, int C, float* __restrict__ dw_qkv,
                                                           float* __restrict__ dw_out) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el, nelem = 512 * C;
  const float s = slot_meet<16, 16>(red, e < nelem ? slot_sum<16, true>(part, e, nelem, nslots, g) : 0.f, g, el);
  if (g == 0 && e < nelem) {
    if (e < 384 * C) dw_qkv[e] += s;
    else dw_out[e - 384 * C] += s;
  }
}
// The slot reduction of the register-resident backward (slot layout la_slot(C)), for several LinearAttention layers at once: block ->
// (item, 32-element group) through a prefix table.  dWq | dWk and the gains go to the gradient buffers (+=); the summed dW2 of the four
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
  const float s = slot_meet<32, 8>(red, e < nelem ? slot_sum<8, true>(part, e, nelem, nslots, g) : 0.f, g, el);
  if (g == 0 && e < nelem) {
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
  hipLaunchKernelGGL(k_linattn_dw_reduce, dim3(cdiv(512 * C, 16)), dim3(256), 0, s, part, nslots, C, dw_qkv, dw_out);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
