// Streaming kernels of the transformer's held-out evaluation (dq_tfm_eval_step): R repeats of a batch of B windows
// stacked into N = R * B samples, sample n = r * B + b (repeat-major).  The clean window x0 is shared by the repeats and never replicated;
// the noise of (r, b) is either read from a (R, B, per) tensor or drawn in the kernel from the counter-based generator of k_noise.hip at
// draw index first_draw + r, and then never written to memory.
//   k_q_sample_repeats            k_q_sample (k_stream.hip) over the stack                 12 B / element (noise read), 8 B (noise drawn)
//   k_mse_per_window_repeats      k_mse_per_window (k_stream.hip) over the stack           8 B / element (target read), 4 B (target drawn)
//   k_mse_per_window_repeats_finish  one loss per repeat                                   8 B / slice
//   k_tfm_kv_broadcast            rows [0, S2) of samples 0 .. B-1 of a (N, Sk, 2H) buffer to samples B .. N-1      8 B / element copied
// The head and the copy: 16 B per lane, grid-stride, no LDS.  per % 4 == 0 throughout (dq_tfm_create: input_dim % 4 == 0).
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include <algorithm>

namespace dq {

// x_t[n] = sa * norm(x0[n % B]) + sb * z[n] with sa, sb from alpha_bars[t[n]]: k_q_sample's expressions in k_q_sample's order.  The sample of
// float4 i is i / per4, the element 4 * (i % per4) + j (the indexing of k_update.hip's Sto family).
__global__ void __launch_bounds__(256) k_q_sample_repeats(const float* __restrict__ alpha_bars, const float* __restrict__ x0,
                                                          const int64_t* __restrict__ t, const float* __restrict__ noise,
                                                          const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p, uint32_t first_draw,
                                                          float* __restrict__ x_t, int B, int64_t total, int64_t per4, int normalize) {
  const uint64_t seed = noise ? 0 : seed_p[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / per4, e4 = i - n * per4;
    const int64_t r = n / B, b = n - r * B;
    const float ab = alpha_bars[t[n]];
    const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
    float4 x = reinterpret_cast<const float4*>(x0)[b * per4 + e4];
    float4 nz;
    if (noise) nz = reinterpret_cast<const float4*>(noise)[i];
    else {
      const int64_t w = ids ? ids[b] : b;
      const uint32_t e0 = (uint32_t)e4 * 4u, d = first_draw + (uint32_t)r;
      nz.x = philox_normal(seed, w, e0, d); nz.y = philox_normal(seed, w, e0 + 1u, d);
      nz.z = philox_normal(seed, w, e0 + 2u, d); nz.w = philox_normal(seed, w, e0 + 3u, d);
    }
    if (normalize) { x.x = x.x * 2.f - 1.f; x.y = x.y * 2.f - 1.f; x.z = x.z * 2.f - 1.f; x.w = x.w * 2.f - 1.f; }
    float4 o;
    o.x = sa * x.x + sb * nz.x; o.y = sa * x.y + sb * nz.y; o.z = sa * x.z + sb * nz.z; o.w = sa * x.w + sb * nz.w;
    reinterpret_cast<float4*>(x_t)[i] = o;
  }
}

int launch_q_sample_repeats(const float* alpha_bars, const float* x0, const int64_t* t, const float* noise, const int64_t* ids,
                            const uint64_t* seed_dev, int first_draw, float* x_t, int B, int R, int64_t per, int normalize, hipStream_t s) {
  DQ_REQUIRE(alpha_bars && x0 && t && x_t, "q_sample_repeats: null argument");
  DQ_REQUIRE(noise || seed_dev, "q_sample_repeats: a null noise needs the seed (device memory)");
  DQ_REQUIRE(B > 0 && R > 0 && per > 0 && per % 4 == 0 && per <= (int64_t)0xffffffff,
             "q_sample_repeats: need B, repeats > 0 and a per-window element count that is a positive multiple of 4 below 2^32");
  DQ_REQUIRE(first_draw >= 0, "q_sample_repeats: the draw index must be >= 0");
  DQ_REQUIRE((((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)x_t) & 15) == 0, "q_sample_repeats: tensors must be 16-byte aligned");
  const int64_t per4 = per / 4, total = (int64_t)R * B * per4;
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
  hipLaunchKernelGGL(k_q_sample_repeats, dim3(grid), dim3(256), 0, s, alpha_bars, x0, t, noise, ids, seed_dev, (uint32_t)first_draw, x_t, B, total,
                     per4, normalize);
  DQ_LAUNCH_CHECK();
  return 0;
}

// k_mse_per_window over the N stacked windows: the target row of window n is n % Bt (Bt = B: the shared x0; Bt = N: one row per window), or,
// with target == nullptr, the noise of (n / B, n % B) drawn here.  The slice partition, the fp64 sums and their order are k_mse_per_window's.
__global__ void __launch_bounds__(256) k_mse_per_window_repeats(const float* __restrict__ out, const float* __restrict__ target, int Bt, float tm,
                                                                float ta, const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p,
                                                                uint32_t first_draw, int B, double* __restrict__ slices, int64_t per,
                                                                int nslices) {
  const int64_t n = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * MSE_PW_SLICE, i1 = min(per, i0 + MSE_PW_SLICE);
  const float* __restrict__ o = out + n * per;
  double acc = 0.0;
  if (target) {
    const float* __restrict__ z = target + (n % Bt) * per;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float zt = z[i] * tm + ta;
      const double d = (double)o[i] - (double)zt;
      acc += d * d;
    }
  } else {
    const int64_t r = n / B, b = n - r * B;
    const uint64_t seed = seed_p[0];
    const int64_t w = ids ? ids[b] : b;
    const uint32_t dr = first_draw + (uint32_t)r;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const float zt = philox_normal(seed, w, (uint32_t)i, dr) * tm + ta;
      const double d = (double)o[i] - (double)zt;
      acc += d * d;
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slices[n * nslices + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// k_mse_per_window_finish once per repeat (block r): per_window[r * B + b] and loss[r] = (float)(sum_b lw[t[r, b]] * mse[r, b] / B), the sums in
// fp64 in index order, each result rounded to fp32 once.  lw == nullptr: weight 1.
__global__ void __launch_bounds__(256) k_mse_per_window_repeats_finish(const double* __restrict__ slices, const float* __restrict__ lw,
                                                                       const int64_t* __restrict__ t, float* __restrict__ per_window,
                                                                       float* __restrict__ loss, int B, int64_t per, int nslices) {
  __shared__ double stage[256];
  const int64_t n0 = (int64_t)blockIdx.x * B;
  double total = 0.0;
  for (int base = 0; base < B; base += 256) {
    const int b = base + threadIdx.x;
    if (b < B) {
      double sum = 0.0;
      for (int g = 0; g < nslices; ++g) sum += slices[(n0 + b) * nslices + g];
      const double mse = sum / (double)per;
      per_window[n0 + b] = (float)mse;
      stage[threadIdx.x] = lw ? (double)lw[t[n0 + b]] * mse : mse;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(256, B - base);
      for (int j = 0; j < m; ++j) total += stage[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[blockIdx.x] = (float)(total / (double)B);
}

int launch_mse_per_window_repeats(const float* out, const float* target, int Bt, float tm, float ta, const int64_t* ids, const uint64_t* seed_dev,
                                  int first_draw, const float* lw, const int64_t* t, float* per_window, float* loss_out, void* scratch,
                                  int64_t scratch_bytes, int B, int R, int64_t per, hipStream_t s) {
  DQ_REQUIRE(out && per_window && loss_out && scratch, "mse_per_window_repeats: null argument");
  DQ_REQUIRE(B > 0 && R > 0 && (int64_t)R * B <= 65535 && per > 0 && per <= (int64_t)0xffffffff,
             "mse_per_window_repeats: need B, repeats > 0, repeats * B <= 65535 and 0 < per < 2^32");
  const int N = R * B;
  DQ_REQUIRE(target || seed_dev, "mse_per_window_repeats: a null target needs the seed (device memory)");
  DQ_REQUIRE(!target || Bt == B || Bt == N, "mse_per_window_repeats: the target has B or repeats * B windows");
  DQ_REQUIRE(first_draw >= 0, "mse_per_window_repeats: the draw index must be >= 0");
  DQ_REQUIRE(!lw || t, "mse_per_window_repeats: the weighted form needs t");
  DQ_REQUIRE(scratch_bytes >= mse_per_window_scratch_bytes(N, per), "mse_per_window_repeats: scratch too small (dq_mse_per_window_scratch_bytes(repeats * B, per))");
  DQ_REQUIRE(((uintptr_t)scratch & 7) == 0, "mse_per_window_repeats: scratch must be 8-byte aligned");
  const int64_t nslices = (per + MSE_PW_SLICE - 1) / MSE_PW_SLICE;
  hipLaunchKernelGGL(k_mse_per_window_repeats, dim3((unsigned)nslices, N), dim3(256), 0, s, out, target, Bt, tm, ta, ids, seed_dev,
                     (uint32_t)first_draw, B, (double*)scratch, per, (int)nslices);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mse_per_window_repeats_finish, dim3(R), dim3(256), 0, s, (const double*)scratch, lw, t, per_window, loss_out, B, per,
                     (int)nslices);
  DQ_LAUNCH_CHECK();
  return 0;
}

// kv (N, Sk, 2H): rows [0, S2) of sample n >= B <- the same rows of sample n % B.  row4 = S2 * 2H / 4 float4 copied per sample, sample4 =
// Sk * 2H / 4 float4 between two samples.  Source (samples < B) and destination (samples >= B) never overlap.
__global__ void __launch_bounds__(256) k_tfm_kv_broadcast(float4* kv, int B, int64_t total, int64_t row4, int64_t sample4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / row4, e = i - m * row4, n = m + B;
    kv[n * sample4 + e] = kv[(n % B) * sample4 + e];
  }
}

int launch_tfm_kv_broadcast(float* kv, int B, int R, int S2, int Sk, int H, hipStream_t s) {
  DQ_REQUIRE(kv, "tfm_kv_broadcast: null buffer");
  DQ_REQUIRE(B > 0 && R > 0 && S2 > 0 && Sk >= S2 && H > 0 && H % 2 == 0, "tfm_kv_broadcast: need B, repeats, S2 > 0, Sk >= S2 and an even H");
  DQ_REQUIRE(((uintptr_t)kv & 15) == 0, "tfm_kv_broadcast: the buffer must be 16-byte aligned");
  if (R == 1) return 0;  // (nothing to replicate: no launch)
  const int64_t row4 = (int64_t)S2 * 2 * H / 4, sample4 = (int64_t)Sk * 2 * H / 4, total = (int64_t)(R - 1) * B * row4;
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
  hipLaunchKernelGGL(k_tfm_kv_broadcast, dim3(grid), dim3(256), 0, s, reinterpret_cast<float4*>(kv), B, total, row4, sample4);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
