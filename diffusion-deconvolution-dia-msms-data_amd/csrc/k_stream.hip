// Streaming (HBM-bound) kernels of the DDIM process: q_sample (K0), the sample epilogue, MSE loss + its gradient (K10), the held-out
// per-window MSE and the MS1 term of train_step.  (The sampler updates, K9: k_update.hip; clip + AdamW, K11: k_adamw.hip.)
// Reference arithmetic: dquartic/model/model.py:239-242 (q_sample), :319-322 (sample epilogue), :361 (mse_loss), :364-402 (the MS1 term).
// The element-wise kernels: 16 B per lane, grid-stride, no LDS.  Algorithmic bytes per element are stated per kernel.
#include "dq_common.h"
#include "dq_kernels.h"
#include <algorithm>
#include <cmath>

namespace dq {

// ---- K0: x_t = sqrt(ab[t_b]) * (2*x0-1) + sqrt(1-ab[t_b]) * noise : 12 B / element (2 reads + 1 write)
__global__ void __launch_bounds__(256) k_q_sample(const float* __restrict__ alpha_bars, const float* __restrict__ x0,
                                                  const int64_t* __restrict__ t, const float* __restrict__ noise,
                                                  float* __restrict__ x_t, int B, int64_t per4, int normalize) {
  const int64_t total = (int64_t)B * per4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / per4);
    const float ab = alpha_bars[t[b]];
    const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
    float4 x = reinterpret_cast<const float4*>(x0)[i];
    const float4 nz = reinterpret_cast<const float4*>(noise)[i];
    if (normalize) { x.x = x.x * 2.f - 1.f; x.y = x.y * 2.f - 1.f; x.z = x.z * 2.f - 1.f; x.w = x.w * 2.f - 1.f; }
    float4 o;
    o.x = sa * x.x + sb * nz.x; o.y = sa * x.y + sb * nz.y; o.z = sa * x.z + sb * nz.z; o.w = sa * x.w + sb * nz.w;
    reinterpret_cast<float4*>(x_t)[i] = o;
  }
}

// the same per element for a window whose RT*MZ is no multiple of 4 (MZ = 2 with an odd RT): a float4 would straddle two windows
__global__ void __launch_bounds__(256) k_q_sample_1(const float* __restrict__ alpha_bars, const float* __restrict__ x0,
                                                    const int64_t* __restrict__ t, const float* __restrict__ noise,
                                                    float* __restrict__ x_t, int B, int64_t per, int normalize) {
  const int64_t total = (int64_t)B * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const float ab = alpha_bars[t[i / per]];
    const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
    float x = x0[i];
    if (normalize) x = x * 2.f - 1.f;
    x_t[i] = sa * x + sb * noise[i];
  }
}

int launch_q_sample(const float* alpha_bars, const float* x0, const int64_t* t, const float* noise, float* x_t, int B,
                    int64_t per_sample, int normalize, hipStream_t s) {
  DQ_REQUIRE(B >= 0 && per_sample >= 0, "q_sample: negative size");
  if (per_sample % 4 != 0) {
    const int grid = (int)std::min<int64_t>(cdiv(B * per_sample, 256), 2048);
    if (grid == 0) return 0;
    hipLaunchKernelGGL(k_q_sample_1, dim3(grid), dim3(256), 0, s, alpha_bars, x0, t, noise, x_t, B, per_sample, normalize);
    DQ_LAUNCH_CHECK();
    return 0;
  }
  const int64_t per4 = per_sample / 4, total = B * per4;
  if (total == 0) return 0;
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
  hipLaunchKernelGGL(k_q_sample, dim3(grid), dim3(256), 0, s, alpha_bars, x0, t, noise, x_t, B, per4, normalize);
  DQ_LAUNCH_CHECK();
  return 0;
}

// ---- sample() epilogue (model.py:319-322): x = (x+1)/2 ; pred = ((2c-1)+1)/2 - x : 16 B / element
__global__ void __launch_bounds__(256) k_sample_finish(const float* __restrict__ x, const float* __restrict__ ms2_cond,
                                                       float* __restrict__ out_x, float* __restrict__ out_noise, int64_t n4,
                                                       int normalize) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float4 c = reinterpret_cast<const float4*>(ms2_cond)[i];
    float4 o, p;
    if (!normalize) {  // identity normalisation: x stays, pred_noise = ms2_cond - x
      p.x = c.x - v.x; p.y = c.y - v.y; p.z = c.z - v.z; p.w = c.w - v.w;
      reinterpret_cast<float4*>(out_x)[i] = v;
      reinterpret_cast<float4*>(out_noise)[i] = p;
      continue;
    }
    o.x = (v.x + 1.f) * 0.5f; o.y = (v.y + 1.f) * 0.5f; o.z = (v.z + 1.f) * 0.5f; o.w = (v.w + 1.f) * 0.5f;
    p.x = ((c.x * 2.f - 1.f) + 1.f) * 0.5f - o.x; p.y = ((c.y * 2.f - 1.f) + 1.f) * 0.5f - o.y;
    p.z = ((c.z * 2.f - 1.f) + 1.f) * 0.5f - o.z; p.w = ((c.w * 2.f - 1.f) + 1.f) * 0.5f - o.w;
    reinterpret_cast<float4*>(out_x)[i] = o;
    reinterpret_cast<float4*>(out_noise)[i] = p;
  }
}

__global__ void __launch_bounds__(256) k_sample_finish_1(const float* __restrict__ x, const float* __restrict__ ms2_cond,
                                                         float* __restrict__ out_x, float* __restrict__ out_noise, int64_t n,
                                                         int normalize) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i], c = ms2_cond[i];
    const float o = normalize ? (v + 1.f) * 0.5f : v;
    out_x[i] = o;
    out_noise[i] = normalize ? ((c * 2.f - 1.f) + 1.f) * 0.5f - o : c - v;
  }
}

int launch_sample_finish(const float* x, const float* ms2_cond, float* out_x, float* out_noise, int64_t n, int normalize,
                         hipStream_t s) {
  DQ_REQUIRE(n >= 0, "sample_finish: negative element count");
  if (n == 0) return 0;
  if (n % 4 != 0) {  // (an element count that is no multiple of 4: one element per lane and step)
    hipLaunchKernelGGL(k_sample_finish_1, dim3((int)std::min<int64_t>(cdiv(n, 256), 2048)), dim3(256), 0, s, x, ms2_cond, out_x, out_noise, n,
                       normalize);
    DQ_LAUNCH_CHECK();
    return 0;
  }
  const int grid = (int)std::min<int64_t>(cdiv(n / 4, 256), 2048);
  hipLaunchKernelGGL(k_sample_finish, dim3(grid), dim3(256), 0, s, x, ms2_cond, out_x, out_noise, n / 4, normalize);
  DQ_LAUNCH_CHECK();
  return 0;
}

// ---- K10: loss = mean((eps-noise)^2) ; grad = 2*(eps-noise)*gscale : 12 B / element
// partial sums go to ``partials`` (one per block, fixed order => deterministic); k_loss_final sums them.
// Weighted form (pred_type "x0", model.py:372-376, 404): target' = target*tm + ta (the normalised x0), every sample's
// squared error and gradient are multiplied by lw[t[b]] (the SNR table); lw == nullptr => weight 1.
__global__ void __launch_bounds__(256) k_mse_fwd_bwd(const float* __restrict__ eps, const float* __restrict__ noise,
                                                     float* __restrict__ grad, float* __restrict__ partials, int64_t n4,
                                                     float gscale, const float* __restrict__ lw, const int64_t* __restrict__ t,
                                                     int64_t per4, float tm, float ta) {
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 e = reinterpret_cast<const float4*>(eps)[i];
    float4 z = reinterpret_cast<const float4*>(noise)[i];
    float w = 1.f;
    if (lw) {
      w = lw[t[i / per4]];
      z.x = z.x * tm + ta; z.y = z.y * tm + ta; z.z = z.z * tm + ta; z.w = z.w * tm + ta;
    }
    float4 d;
    d.x = e.x - z.x; d.y = e.y - z.y; d.z = e.z - z.z; d.w = e.w - z.w;
    acc += w * (d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w);
    if (grad) {
      const float gs = gscale * w;
      float4 g;
      g.x = d.x * gs; g.y = d.y * gs; g.z = d.z * gs; g.w = d.w * gs;
      reinterpret_cast<float4*>(grad)[i] = g;
    }
  }
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// n or the per-sample count no multiple of 4: one element per lane and step, the same partial sums per block
__global__ void __launch_bounds__(256) k_mse_fwd_bwd_1(const float* __restrict__ eps, const float* __restrict__ noise,
                                                       float* __restrict__ grad, float* __restrict__ partials, int64_t n,
                                                       float gscale, const float* __restrict__ lw, const int64_t* __restrict__ t,
                                                       int64_t per, float tm, float ta) {
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float z = noise[i], w = 1.f;
    if (lw) { w = lw[t[i / per]]; z = z * tm + ta; }
    const float d = eps[i] - z;
    acc += w * (d * d);
    if (grad) grad[i] = d * (gscale * w);
  }
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(64) k_sum_partials(const float* __restrict__ partials, int n, float scale, float* __restrict__ out) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) acc += partials[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[0] = acc * scale;
}

__global__ void __launch_bounds__(256) k_axpy(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

__global__ void __launch_bounds__(256) k_copy(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_zero(float4* __restrict__ dst, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) dst[i] = float4{0.f, 0.f, 0.f, 0.f};
}
// dst[0..n) = 0 as a kernel (n a multiple of 4, dst 16-byte aligned): no memset node in the middle of the step
int launch_zero(float* dst, int64_t n, hipStream_t s) {
  if (n == 0) return 0;
  DQ_REQUIRE(n % 4 == 0 && ((uintptr_t)dst & 15) == 0, "zero: needs a 16-byte aligned buffer of a multiple of 4 floats");
  hipLaunchKernelGGL(k_zero, dim3((int)std::min<int64_t>(cdiv(n / 4, 256), 8192)), dim3(256), 0, s, reinterpret_cast<float4*>(dst), n / 4);
  DQ_LAUNCH_CHECK();
  return 0;
}

// plain kernel copy: a hipMemcpyAsync in the middle of the step costs far more than its 3 us blit (queue barriers around it)
int launch_copy(float* dst, const float* src, int64_t n, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_copy, dim3((int)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, s, dst, src, n);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_axpy(float* dst, const float* src, int64_t n, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_axpy, dim3((int)std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, s, dst, src, n);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_sum_partials(const float* partials, int count, float scale, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(64), 0, s, partials, count, scale, out);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_mse_fwd_bwd(const float* eps, const float* noise, float* loss_out, float* grad_out, float* partials, int64_t n,
                       hipStream_t s, const float* lw, const int64_t* t, int64_t per_sample, float tm, float ta, int* defer_sum) {
  DQ_REQUIRE(n > 0, "mse: element count must be positive");
  DQ_REQUIRE(!lw || (t && per_sample > 0 && n % per_sample == 0),
             "mse: the weighted form needs t and a per-sample element count that divides n");
  const bool vec = n % 4 == 0 && (!lw || per_sample % 4 == 0);
  const int grid = (int)std::min<int64_t>(cdiv(vec ? n / 4 : n, 256), MSE_MAX_BLOCKS);
  if (vec)
    hipLaunchKernelGGL(k_mse_fwd_bwd, dim3(grid), dim3(256), 0, s, eps, noise, grad_out, partials, n / 4, 2.0f / (float)n, lw, t,
                       lw ? per_sample / 4 : (int64_t)1, tm, ta);
  else
    hipLaunchKernelGGL(k_mse_fwd_bwd_1, dim3(grid), dim3(256), 0, s, eps, noise, grad_out, partials, n, 2.0f / (float)n, lw, t,
                       lw ? per_sample : (int64_t)1, tm, ta);
  DQ_LAUNCH_CHECK();
  if (defer_sum) { *defer_sum = grid; return 0; }  // the caller sums the partials later (launch_sum_partials(partials, grid, 1 / n, loss_out))
  return launch_sum_partials(partials, grid, 1.0f / (float)n, loss_out, s);
}

// ---- K10 under the v objective (pred_type "v_prediction"): the target z = sa_b * noise - sb_b * (x0 * tm + ta) with
// sa_b = sqrt(ab[t_b]), sb_b = sqrt(1 - ab[t_b]) (k_q_sample's two square roots) is formed per element and never written : 16 B / element.
// lw (nullable: 1) weights sample b by lw[t_b] as in the weighted form above.  V = 4: 16 B per lane (per % 4 == 0, so no lane's four
// elements straddle two samples); V = 1: any count.  nv, perv: the element count and the per-sample count in units of V.
template <int V>
__global__ void __launch_bounds__(256) k_mse_v_fwd_bwd(const float* __restrict__ pred, const float* __restrict__ x0, const float* __restrict__ noise,
                                                       const float* __restrict__ alpha_bars, float* __restrict__ grad, float* __restrict__ partials,
                                                       int64_t nv, float gscale, const float* __restrict__ lw, const int64_t* __restrict__ t,
                                                       int64_t perv, float tm, float ta) {
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tb = t[i / perv];
    const float ab = alpha_bars[tb];
    const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
    const float w = lw ? lw[tb] : 1.f;
    float e[V], x[V], z[V], g[V];
    if constexpr (V == 4) {
      const float4 e4 = reinterpret_cast<const float4*>(pred)[i], x4 = reinterpret_cast<const float4*>(x0)[i], z4 = reinterpret_cast<const float4*>(noise)[i];
      e[0] = e4.x; e[1] = e4.y; e[2] = e4.z; e[3] = e4.w;
      x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w;
      z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
    } else {
      e[0] = pred[i]; x[0] = x0[i]; z[0] = noise[i];
    }
    const float gs = gscale * w;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float d = e[j] - (sa * z[j] - sb * (x[j] * tm + ta));
      sq += d * d;
      g[j] = d * gs;
    }
    acc += w * sq;
    if (grad) {
      if constexpr (V == 4) reinterpret_cast<float4*>(grad)[i] = make_float4(g[0], g[1], g[2], g[3]);
      else grad[i] = g[0];
    }
  }
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

int launch_mse_v_fwd_bwd(const float* pred, const float* x0, const float* noise, const float* alpha_bars, float tm, float ta, const float* lw,
                         const int64_t* t, float* loss_out, float* grad_out, float* partials, int B, int64_t per, hipStream_t s, int* defer_sum) {
  DQ_REQUIRE(pred && x0 && noise && alpha_bars && t && partials && (loss_out || defer_sum), "mse_v: null argument");
  DQ_REQUIRE(B > 0 && per > 0, "mse_v: B and per must be positive");
  const int64_t n = (int64_t)B * per;
  const uintptr_t bits = (uintptr_t)pred | (uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)grad_out;
  const bool vec = per % 4 == 0 && (bits & 15) == 0;
  const int grid = (int)std::min<int64_t>(cdiv(vec ? n / 4 : n, 256), MSE_MAX_BLOCKS);
  if (vec)
    hipLaunchKernelGGL(k_mse_v_fwd_bwd<4>, dim3(grid), dim3(256), 0, s, pred, x0, noise, alpha_bars, grad_out, partials, n / 4, 2.0f / (float)n, lw,
                       t, per / 4, tm, ta);
  else
    hipLaunchKernelGGL(k_mse_v_fwd_bwd<1>, dim3(grid), dim3(256), 0, s, pred, x0, noise, alpha_bars, grad_out, partials, n, 2.0f / (float)n, lw, t,
                       per, tm, ta);
  DQ_LAUNCH_CHECK();
  if (defer_sum) { *defer_sum = grid; return 0; }  // (as launch_mse_fwd_bwd)
  return launch_sum_partials(partials, grid, 1.0f / (float)n, loss_out, s);
}

// ---- held-out loss (dq_mse_per_window, dq_eval_step): per-window MSE and its weighted mean, forward only : 8 B / element
// target' = target * tm + ta in fp32 (one multiply, one add: what k_mse_fwd_bwd forms), d = (double)out - (double)target', d * d summed in
// fp64.  One block per (slice of MSE_PW_SLICE elements, window): the partition of a window depends on `per` alone, never on B, and the
// slices are added in index order -- no atomics, so a window's value does not depend on the batch around it.  scratch: one double per slice.
__global__ void __launch_bounds__(256) k_mse_per_window(const float* __restrict__ out, const float* __restrict__ target, float tm, float ta,
                                                        double* __restrict__ slices, int64_t per, int nslices) {
  const int64_t b = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * MSE_PW_SLICE, i1 = min(per, i0 + MSE_PW_SLICE);
  const float* __restrict__ o = out + b * per;
  const float* __restrict__ z = target + b * per;
  double acc = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float zt = z[i] * tm + ta;
    const double d = (double)o[i] - (double)zt;
    acc += d * d;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slices[b * nslices + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// per_window[b] = (float)(sum of the window's slices / per); loss = (float)(sum_b lw[t_b] * (sum_b / per) / B), both sums in fp64 in index
// order (256 windows at a time are staged in LDS, thread 0 adds them up), each result rounded to fp32 once.  lw == nullptr: weight 1.
__global__ void __launch_bounds__(256) k_mse_per_window_finish(const double* __restrict__ slices, const float* __restrict__ lw,
                                                               const int64_t* __restrict__ t, float* __restrict__ per_window,
                                                               float* __restrict__ loss, int B, int64_t per, int nslices) {
  __shared__ double stage[256];
  double total = 0.0;
  for (int base = 0; base < B; base += 256) {
    const int b = base + threadIdx.x;
    if (b < B) {
      double sum = 0.0;
      for (int g = 0; g < nslices; ++g) sum += slices[(int64_t)b * nslices + g];
      const double mse = sum / (double)per;
      per_window[b] = (float)mse;
      stage[threadIdx.x] = lw ? (double)lw[t[b]] * mse : mse;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(256, B - base);
      for (int j = 0; j < m; ++j) total += stage[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(total / (double)B);
}

int64_t mse_per_window_scratch_bytes(int B, int64_t per) {
  if (B < 1 || per < 1) return -1;
  return (int64_t)sizeof(double) * B * ((per + MSE_PW_SLICE - 1) / MSE_PW_SLICE);
}

int launch_mse_per_window(const float* out, const float* target, float tm, float ta, const float* lw, const int64_t* t, float* per_window,
                          float* loss_out, void* scratch, int64_t scratch_bytes, int B, int64_t per, hipStream_t s) {
  DQ_REQUIRE(out && target && per_window && loss_out && scratch, "mse_per_window: null argument");
  DQ_REQUIRE(B > 0 && B <= 65535 && per > 0, "mse_per_window: need 0 < B <= 65535 and per > 0");
  DQ_REQUIRE(!lw || t, "mse_per_window: the weighted form needs t");
  DQ_REQUIRE(scratch_bytes >= mse_per_window_scratch_bytes(B, per), "mse_per_window: scratch too small (dq_mse_per_window_scratch_bytes)");
  DQ_REQUIRE(((uintptr_t)scratch & 7) == 0, "mse_per_window: scratch must be 8-byte aligned");
  const int64_t nslices = (per + MSE_PW_SLICE - 1) / MSE_PW_SLICE;
  DQ_REQUIRE(nslices <= INT32_MAX, "mse_per_window: window too large");
  hipLaunchKernelGGL(k_mse_per_window, dim3((unsigned)nslices, B), dim3(256), 0, s, out, target, tm, ta, (double*)scratch, per, (int)nslices);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mse_per_window_finish, dim3(1), dim3(256), 0, s, (const double*)scratch, lw, t, per_window, loss_out, B, per,
                     (int)nslices);
  DQ_LAUNCH_CHECK();
  return 0;
}

// the same under the v objective: the target sa_b * noise - sb_b * (x0 * tm + ta) in fp32 (k_mse_v_fwd_bwd's arithmetic), formed per
// element : 12 B / element.  Slices, order and the finishing kernel are k_mse_per_window's.
__global__ void __launch_bounds__(256) k_mse_per_window_v(const float* __restrict__ out, const float* __restrict__ x0, const float* __restrict__ noise,
                                                          const float* __restrict__ alpha_bars, const int64_t* __restrict__ t, float tm, float ta,
                                                          double* __restrict__ slices, int64_t per, int nslices) {
  const int64_t b = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * MSE_PW_SLICE, i1 = min(per, i0 + MSE_PW_SLICE);
  const float ab = alpha_bars[t[b]];
  const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
  const float* __restrict__ o = out + b * per;
  const float* __restrict__ x = x0 + b * per;
  const float* __restrict__ z = noise + b * per;
  double acc = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float zt = sa * z[i] - sb * (x[i] * tm + ta);
    const double d = (double)o[i] - (double)zt;
    acc += d * d;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slices[b * nslices + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

int launch_mse_per_window_v(const float* out, const float* x0, const float* noise, const float* alpha_bars, float tm, float ta, const float* lw,
                            const int64_t* t, float* per_window, float* loss_out, void* scratch, int64_t scratch_bytes, int B, int64_t per,
                            hipStream_t s) {
  DQ_REQUIRE(out && x0 && noise && alpha_bars && t && per_window && loss_out && scratch, "mse_per_window_v: null argument");
  DQ_REQUIRE(B > 0 && B <= 65535 && per > 0, "mse_per_window_v: need 0 < B <= 65535 and per > 0");
  DQ_REQUIRE(scratch_bytes >= mse_per_window_scratch_bytes(B, per), "mse_per_window_v: scratch too small (dq_mse_per_window_scratch_bytes)");
  DQ_REQUIRE(((uintptr_t)scratch & 7) == 0, "mse_per_window_v: scratch must be 8-byte aligned");
  const int64_t nslices = (per + MSE_PW_SLICE - 1) / MSE_PW_SLICE;
  DQ_REQUIRE(nslices <= INT32_MAX, "mse_per_window_v: window too large");
  hipLaunchKernelGGL(k_mse_per_window_v, dim3((unsigned)nslices, B), dim3(256), 0, s, out, x0, noise, alpha_bars, t, tm, ta, (double*)scratch, per,
                     (int)nslices);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mse_per_window_finish, dim3(1), dim3(256), 0, s, (const double*)scratch, lw, t, per_window, loss_out, B, per,
                     (int)nslices);
  DQ_LAUNCH_CHECK();
  return 0;
}

// ---- the MS1 term of train_step (reference model.py:364-371, 379-386, 398-402; semantics chosen in DESIGN.md section 12 because
// the reference's branch raises): per sample b, with D = x_t - eps_pred ('eps') or x0_pred ('x0'),
//   additional_b = sum over f in {sum, mean, max over m/z} of mean_rt (s_f[rt] / max_rt s_f - ms1n[rt] / max_rt ms1n)^2
//   loss_b = (1 - w) * MSE_b + w * additional_b ; loss = mean_b loss_weight[t_b] * loss_b
// (1) k_ms1_rows: one wave per (b, rt) row -> sum, max and arg-max over m/z;
// (2) k_ms1_sample: one block per sample -> the three normalisers, additional_b and d additional_b / d s_f[rt];
// (3) k_ms1_apply: grad = (1 - w) * grad_MSE + sign * w * loss_weight_b / B * (d/d s_sum + d/d s_mean / MZ + [mz == argmax] d/d s_max)
//     and the loss scalar.  Fixed-order reductions throughout.
__global__ void __launch_bounds__(256) k_ms1_rows(const float* __restrict__ out, const float* __restrict__ x_t, int64_t rows, int MZ,
                                                  float* __restrict__ rsum, float* __restrict__ rmax, int* __restrict__ ramax) {
  const int64_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float sm = 0.f, mx = -INFINITY;
  int am = 0;
  for (int mz = lane; mz < MZ; mz += 64) {
    const float o = out[row * MZ + mz];
    const float d = x_t ? x_t[row * MZ + mz] - o : o;
    sm += d;
    if (d > mx) { mx = d; am = mz; }
  }
  sm = wave_sum(sm);
  // arg-max over the lanes: larger value wins, the smaller index on ties (torch.max returns the first maximum)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float omx = __shfl_xor(mx, o, 64);
    const int oam = __shfl_xor(am, o, 64);
    if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
  }
  if (lane == 0) { rsum[row] = sm; rmax[row] = mx; ramax[row] = am; }
}

__device__ __forceinline__ void block_argmax(float& v, int& idx, float* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = idx; }
  __syncthreads();
  v = sv[0]; idx = si[0];
  for (int k = 1; k < 4; ++k)
    if (sv[k] > v || (sv[k] == v && si[k] < idx)) { v = sv[k]; idx = si[k]; }
}
__device__ __forceinline__ float block_sum4(float v, float* sv) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sv[0] + sv[1]) + (sv[2] + sv[3]);
}

__global__ void __launch_bounds__(256) k_ms1_sample(const float* __restrict__ rsum, const float* __restrict__ rmax,
                                                    const float* __restrict__ ms1, float cm, float ca, int RT, int MZ,
                                                    const float* __restrict__ lw, const int64_t* __restrict__ t,
                                                    float* __restrict__ dsum, float* __restrict__ dmax, float* __restrict__ addl) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int b = blockIdx.x;
  const float* s_sum = rsum + (int64_t)b * RT;
  const float* s_max = rmax + (int64_t)b * RT;
  const float* m1 = ms1 + (int64_t)b * RT;
  const float invMZ = 1.0f / (float)MZ;
  // the four row maxima (and where they sit): sum, mean (= sum / MZ: same place), max, and the MS1 chromatogram
  float a0 = -INFINITY, a2 = -INFINITY, a3 = -INFINITY;
  int i0 = 0, i2 = 0, i3 = 0;
  for (int rt = threadIdx.x; rt < RT; rt += 256) {
    const float v0 = s_sum[rt], v2 = s_max[rt], v3 = fmaf(m1[rt], cm, ca);
    if (v0 > a0) { a0 = v0; i0 = rt; }
    if (v2 > a2) { a2 = v2; i2 = rt; }
    if (v3 > a3) { a3 = v3; i3 = rt; }
  }
  block_argmax(a0, i0, sv, si);
  block_argmax(a2, i2, sv, si);
  block_argmax(a3, i3, sv, si);
  const float m_sum = a0, m_mean = a0 * invMZ, m_max = a2, m_ms1 = a3;
  // A_f = mean_rt (u_f - v)^2 ; c_f = sum_rt g_f s_f / m_f^2 with g_f = 2 (u_f - v) / RT
  float A0 = 0.f, A1 = 0.f, A2 = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
  const float gs = 2.0f / (float)RT;
  for (int rt = threadIdx.x; rt < RT; rt += 256) {
    const float v = fmaf(m1[rt], cm, ca) / m_ms1;
    const float s0 = s_sum[rt], s1 = s0 * invMZ, s2 = s_max[rt];
    const float e0 = s0 / m_sum - v, e1 = s1 / m_mean - v, e2 = s2 / m_max - v;
    A0 = fmaf(e0, e0, A0); A1 = fmaf(e1, e1, A1); A2 = fmaf(e2, e2, A2);
    c0 = fmaf(gs * e0, s0, c0); c1 = fmaf(gs * e1, s1, c1); c2 = fmaf(gs * e2, s2, c2);
  }
  A0 = block_sum4(A0, sv); A1 = block_sum4(A1, sv); A2 = block_sum4(A2, sv);
  c0 = block_sum4(c0, sv) / (m_sum * m_sum); c1 = block_sum4(c1, sv) / (m_mean * m_mean); c2 = block_sum4(c2, sv) / (m_max * m_max);
  for (int rt = threadIdx.x; rt < RT; rt += 256) {
    const float v = fmaf(m1[rt], cm, ca) / m_ms1;
    const float s0 = s_sum[rt], s1 = s0 * invMZ, s2 = s_max[rt];
    const float d0 = gs * (s0 / m_sum - v) / m_sum - (rt == i0 ? c0 : 0.f);
    const float d1 = gs * (s1 / m_mean - v) / m_mean - (rt == i0 ? c1 : 0.f);
    const float d2 = gs * (s2 / m_max - v) / m_max - (rt == i2 ? c2 : 0.f);
    dsum[(int64_t)b * RT + rt] = fmaf(d1, invMZ, d0);
    dmax[(int64_t)b * RT + rt] = d2;
  }
  if (threadIdx.x == 0) addl[b] = (lw ? lw[t[b]] : 1.0f) * (((A0 + A1) + A2) / (float)RT);
}

__global__ void __launch_bounds__(256) k_ms1_apply(float* __restrict__ grad, const float* __restrict__ dsum, const float* __restrict__ dmax,
                                                   const int* __restrict__ ramax, const float* __restrict__ lw,
                                                   const int64_t* __restrict__ t, const float* __restrict__ addl, float w, float sign,
                                                   int B, int RT, int MZ, float* __restrict__ loss) {
  const int64_t n = (int64_t)B * RT * MZ;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / MZ;
    const int mz = (int)(i - row * MZ);
    const int b = (int)(row / RT);
    const float k = sign * w * (lw ? lw[t[b]] : 1.0f) / (float)B;
    const float extra = dsum[row] + (mz == ramax[row] ? dmax[row] : 0.f);
    if (grad) grad[i] = fmaf(1.0f - w, grad[i], k * extra);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += addl[b];
    loss[0] = (1.0f - w) * loss[0] + w * acc / (float)B;
  }
}

// scratch: 5 * B * RT + B floats.  loss_out / grad hold the MSE part on entry (launch_mse_fwd_bwd) and the combined loss on exit.
int launch_ms1_loss(const float* out, const float* x_t, const float* ms1, float cm, float ca, const float* lw, const int64_t* t, float w,
                    int B, int RT, int MZ, float* grad, float* loss_out, float* scratch, hipStream_t s) {
  DQ_REQUIRE(out && ms1 && loss_out && scratch && B > 0 && RT > 0 && MZ > 0, "ms1 loss: missing operand");
  DQ_REQUIRE(!lw || t, "ms1 loss: per-timestep weights need t");
  const int64_t rows = (int64_t)B * RT;
  float* rsum = scratch; float* rmax = rsum + rows; int* ramax = reinterpret_cast<int*>(rmax + rows);
  float* dsum = rmax + 2 * rows; float* dmax = dsum + rows; float* addl = dmax + rows;
  hipLaunchKernelGGL(k_ms1_rows, dim3(cdiv(rows, 4)), dim3(256), 0, s, out, x_t, rows, MZ, rsum, rmax, ramax);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ms1_sample, dim3(B), dim3(256), 0, s, rsum, rmax, ms1, cm, ca, RT, MZ, lw, t, dsum, dmax, addl);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ms1_apply, dim3((int)std::min<int64_t>(cdiv(rows * MZ, 256), 4096)), dim3(256), 0, s, grad, dsum, dmax, ramax, lw, t,
                     addl, w, x_t ? -1.0f : 1.0f, B, RT, MZ, loss_out);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
