// First conv of the MS1 feature path (attn_cond_proj.1.0, k7 'same' + GELU, unet1d.py:976, 1122-1130) for attn_cond_channels = M1 > 1.
// The conditioning arrives as (B, RT, M1) with the m/z channel contiguous -- the layout the data side produces -- and both kernels read it as it
// is: lane = m/z channel (strided by 64), so a row's M1 floats are one coalesced read and no (B, M1, RT) copy is ever made.
//
//   forward   u[b][c][rt] = bias[c] + sum_tap sum_m W0[c][m][tap] * n(ms1[b][rt + tap - 3][m]),  n(v) = v * cm + ca
//             rows outside 0..RT-1 contribute nothing (the reference zero-pads the NORMALISED tensor: no `ca` from the padding)
//   wgrad     dW0[c][m][tap] = sum_{b, rt} du[b][c][rt] * n(ms1[b][rt + tap - 3][m]),  dbias[c] = sum du
//
// M1 = 1 never comes here (k_ms1_norm + k_conv_fwd<8, 7> as before).  No float atomics: the forward's cross-lane sum is a fixed tree,
// the weight gradient leaves one slot per workgroup for k_wgrad_reduce's ordered sum.
#include "dq_common.h"
#include "dq_kernels.h"

#include <algorithm>

namespace dq {
namespace {

constexpr int CO = 8;  // attn_cond_init_dim = 2 * dim

// One wave = MS1_FWD_TP consecutive RT positions of one sample; the MS1_FWD_TP + 6 rows they see are read once.  Per lane and 64-channel
// chunk: the 56 weights of its channel in registers, then row by row (ascending) a product into each of the <= 7 positions the row
// reaches.  The order of a position's sum is (chunk, row) on the lane and a fixed tree across lanes: it depends on M1 only, not on B, RT or
// the grid, so a window's features do not depend on the batch it is in.
__global__ void __launch_bounds__(256) k_ms1_feat_fwd(Ms1FeatFwd a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, M1 = a.M1, RT = a.RT;
  const int rt0 = (blockIdx.x * MS1_FWD_WAVES + wave) * MS1_FWD_TP;
  if (rt0 >= RT) return;  // (wave-uniform; the kernel has no barrier)
  const float* __restrict__ src = a.ms1 + (int64_t)b * RT * M1;
  float* __restrict__ nrm = a.ms1n_out ? a.ms1n_out + (int64_t)b * RT * M1 : nullptr;
  float acc[MS1_FWD_TP][CO];
#pragma unroll
  for (int p = 0; p < MS1_FWD_TP; ++p)
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[p][c] = 0.f;
  for (int m0 = 0; m0 < M1; m0 += 64) {
    const int m = m0 + lane;
    const bool ok = m < M1;
    float w[CO][7];
#pragma unroll
    for (int c = 0; c < CO; ++c)
#pragma unroll
      for (int tap = 0; tap < 7; ++tap) w[c][tap] = ok ? a.w[((int64_t)c * M1 + m) * 7 + tap] : 0.f;
#pragma unroll
    for (int j = 0; j < MS1_FWD_TP + 6; ++j) {
      const int r = rt0 - 3 + j;
      float v = 0.f;
      if (ok && r >= 0 && r < RT) {
        v = fmaf(src[(int64_t)r * M1 + m], a.cm, a.ca);  // (k_ms1_norm's arithmetic)
        if (nrm && j >= 3 && j < 3 + MS1_FWD_TP) nrm[(int64_t)r * M1 + m] = v;  // (the rows this wave owns: what the weight gradient reads)
      }
#pragma unroll
      for (int tap = 0; tap < 7; ++tap) {
        const int p = j - tap;  // row r is tap `tap` of position rt0 + p
        if (p >= 0 && p < MS1_FWD_TP) {
#pragma unroll
          for (int c = 0; c < CO; ++c) acc[p][c] += w[c][tap] * v;
        }
      }
    }
  }
  // Cross-lane sum as a reduce-scatter: at distance h a lane hands the half of its values its partner keeps to that partner and adds what it
  // receives to the half it keeps -- 63 exchanges for the 64 sums (a full reduction of each would be 64 x 6), and lane p * 8 + c ends up with
  // output (position p, channel c).  A fixed tree of six additions per output.
  float* flat = &acc[0][0];
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const bool up = (lane & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float send = up ? flat[i] : flat[i + h], keep = up ? flat[i + h] : flat[i];
      flat[i] = keep + __shfl_xor(send, h, 64);
    }
  }
  const float mine = flat[0];
  const int p = lane >> 3, c = lane & 7, rt = rt0 + p;
  if (rt < RT) {
    const float u = mine + a.bias[c];
    const int64_t o = ((int64_t)b * CO + c) * RT + rt;
    if (a.u_out) a.u_out[o] = u;
    a.a_out[o] = gelu_f(u);
  }
}
static_assert(MS1_FWD_TP * CO == 64, "one output per lane");

// A workgroup walks units (sample, MS1_WG_T consecutive positions), wave w of it the 64-channel chunks w, w + waves, ...: lane = m/z channel,
// 56 accumulators.  d u of the unit sits in LDS with zeros around it, so every row adds its 7 x 8 products without a bounds test; rows
// outside 0..RT-1 are not read.  Each workgroup leaves [dW0 (8, M1, 7) | dbias (8)] in its own slot.
__global__ void __launch_bounds__(256) k_ms1_feat_wgrad(Ms1FeatWgrad a, int ntiles, int units, int nchunks) {
  __shared__ __attribute__((aligned(16))) float dus[MS1_WG_T + 12][CO];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int M1 = a.M1, RT = a.RT;
  float* __restrict__ part = a.part + (int64_t)blockIdx.x * (56 * (int64_t)M1 + CO);
  float bsum = 0.f;
  for (int c0 = 0; c0 < nchunks; c0 += nw) {  // (workgroup-uniform trip counts: the barriers below are reached by every wave)
    const int m = (c0 + wave) * 64 + lane;
    const bool ok = m < M1;
    float acc[CO][7];
#pragma unroll
    for (int c = 0; c < CO; ++c)
#pragma unroll
      for (int tap = 0; tap < 7; ++tap) acc[c][tap] = 0.f;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
      const int b = u / ntiles, rt0 = (u % ntiles) * MS1_WG_T;
      __syncthreads();
      for (int i = threadIdx.x; i < (MS1_WG_T + 12) * CO; i += blockDim.x) {
        const int j = i >> 3, c = i & 7, rt = rt0 - 6 + j;
        dus[j][c] = (j >= 6 && j < 6 + MS1_WG_T && rt < RT) ? a.du[((int64_t)b * CO + c) * RT + rt] : 0.f;
      }
      __syncthreads();
      if (c0 == 0 && threadIdx.x < CO)
        for (int j = 6; j < 6 + MS1_WG_T; ++j) bsum += dus[j][threadIdx.x];
      const float* __restrict__ src = a.ms1n + (int64_t)b * RT * M1;
      const int r_lo = max(rt0 - 3, 0), r_hi = min(rt0 + MS1_WG_T + 3, RT);
      for (int r = r_lo; r < r_hi; ++r) {
        const float v = ok ? src[(int64_t)r * M1 + m] : 0.f;
        const int j0 = r - rt0 + 9;  // position rt = r - tap + 3 sits at dus[rt - rt0 + 6]
#pragma unroll
        for (int tap = 0; tap < 7; ++tap) {
          const float4 d0 = *reinterpret_cast<const float4*>(&dus[j0 - tap][0]);
          const float4 d1 = *reinterpret_cast<const float4*>(&dus[j0 - tap][4]);
          acc[0][tap] += d0.x * v; acc[1][tap] += d0.y * v; acc[2][tap] += d0.z * v; acc[3][tap] += d0.w * v;
          acc[4][tap] += d1.x * v; acc[5][tap] += d1.y * v; acc[6][tap] += d1.z * v; acc[7][tap] += d1.w * v;
        }
      }
    }
    if (ok) {
#pragma unroll
      for (int c = 0; c < CO; ++c)
#pragma unroll
        for (int tap = 0; tap < 7; ++tap) part[((int64_t)c * M1 + m) * 7 + tap] = acc[c][tap];
    }
  }
  if (threadIdx.x < CO) part[56 * (int64_t)M1 + threadIdx.x] = bsum;
}

}  // namespace

int launch_ms1_feat_fwd(const Ms1FeatFwd& a, hipStream_t s) {
  DQ_REQUIRE(a.ms1 && a.w && a.bias && a.a_out, "ms1_feat_fwd: missing operand");
  DQ_REQUIRE(a.B > 0 && a.RT > 0 && a.M1 >= 1 && a.M1 <= MS1_MAX_CHANNELS, "ms1_feat_fwd: need B, RT > 0 and 1 <= M1 <= 4096");
  DQ_REQUIRE(a.B <= 65535, "ms1_feat_fwd: B above 65535");
  dim3 grid(cdiv(a.RT, MS1_FWD_WAVES * MS1_FWD_TP), a.B), block(64 * MS1_FWD_WAVES);
  hipLaunchKernelGGL(k_ms1_feat_fwd, grid, block, 0, s, a);
  DQ_LAUNCH_CHECK();
  return 0;
}

int ms1_feat_wgrad_parts(int B, int RT, int M1) {
  const int64_t units = (int64_t)B * cdiv(RT, MS1_WG_T), slot = 56 * (int64_t)M1 + CO;
  // one unit per workgroup up to MS1_WG_MAX_PARTS, and no more slots than ~16 MB of scratch holds (wide M1: a workgroup walks several units)
  return (int)std::max<int64_t>(1, std::min<int64_t>({units, MS1_WG_MAX_PARTS, std::max<int64_t>(8, (int64_t(1) << 22) / slot)}));
}
int64_t ms1_feat_wgrad_part_floats(int B, int RT, int M1) { return (int64_t)ms1_feat_wgrad_parts(B, RT, M1) * (56 * (int64_t)M1 + CO); }

int launch_ms1_feat_wgrad(const Ms1FeatWgrad& a, hipStream_t s) {
  DQ_REQUIRE(a.ms1n && a.du && a.dw && a.dbias && a.part, "ms1_feat_wgrad: missing operand");
  DQ_REQUIRE(a.B > 0 && a.RT > 0 && a.M1 >= 1 && a.M1 <= MS1_MAX_CHANNELS, "ms1_feat_wgrad: need B, RT > 0 and 1 <= M1 <= 4096");
  DQ_REQUIRE(a.part_floats >= ms1_feat_wgrad_part_floats(a.B, a.RT, a.M1), "ms1_feat_wgrad: scratch too small");
  const int ntiles = cdiv(a.RT, MS1_WG_T), units = a.B * ntiles, nchunks = cdiv(a.M1, 64);
  const int parts = ms1_feat_wgrad_parts(a.B, a.RT, a.M1);
  hipLaunchKernelGGL(k_ms1_feat_wgrad, dim3(parts), dim3(64 * std::min(4, nchunks)), 0, s, a, ntiles, units, nchunks);
  DQ_LAUNCH_CHECK();
  return launch_wgrad_reduce(a.part, parts, 56 * a.M1, CO, a.dw, a.dbias, s);
}

}  // namespace dq
