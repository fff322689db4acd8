// K11: global L2 norm (two-stage, deterministic) + clip + AdamW on the flat parameter buffer, optionally with an exponential moving
// average of the parameters kept in the same pass (DESIGN.md sections 21, 33).  Reference arithmetic:
// dquartic/model/model_interface.py:1121-1122 (clip_grad_norm_(10.0) + AdamW with torch defaults).
//   k_sumsq              partial sums of (g * gscale)^2, one per block in a fixed order                          4 B / param
//   k_adamw_hyper        (device-scalar step only) bumps the step counter and forms the step's scalars behind the partial sums
//   k_adamw_clip<EMA>    clip coefficient from the partials, then the update: reads p g m v, writes p m v       28 B / param
//                        <true>: and e <- e + w (p_new - e) from the p just formed: one more read and write     36 B / param
//                        (a lerp over the flat buffer afterwards reads p again: 40 B and a launch)
// One launcher, launch_adamw, for the four entry points: scalars from the host or from device memory, with or without the average.
#include "dq_common.h"
#include "dq_kernels.h"
#include <algorithm>
#include <cmath>

namespace dq {

__global__ void __launch_bounds__(256) k_sumsq(const float* __restrict__ g, int64_t n, float gscale, float* __restrict__ partials) {
  // 16-byte loads, four independent accumulators, two loads in flight: the 764 MB gradient of the transformer (191 M parameters)
  // is a bandwidth job; the scalar one-accumulator loop ran it at 2.3 TB/s
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const int64_t n4 = (((uintptr_t)g & 15) == 0) ? n / 4 : 0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const float4 u = g4[i], w = g4[i + stride];
    a0 = fmaf(u.x * gscale, u.x * gscale, a0); a1 = fmaf(u.y * gscale, u.y * gscale, a1);
    a2 = fmaf(u.z * gscale, u.z * gscale, a2); a3 = fmaf(u.w * gscale, u.w * gscale, a3);
    a0 = fmaf(w.x * gscale, w.x * gscale, a0); a1 = fmaf(w.y * gscale, w.y * gscale, a1);
    a2 = fmaf(w.z * gscale, w.z * gscale, a2); a3 = fmaf(w.w * gscale, w.w * gscale, a3);
  }
  for (; i < n4; i += stride) {
    const float4 u = g4[i];
    a0 = fmaf(u.x * gscale, u.x * gscale, a0); a1 = fmaf(u.y * gscale, u.y * gscale, a1);
    a2 = fmaf(u.z * gscale, u.z * gscale, a2); a3 = fmaf(u.w * gscale, u.w * gscale, a3);
  }
  for (int64_t j = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += stride) {
    const float v = g[j] * gscale;
    a0 = fmaf(v, v, a0);
  }
  float acc = (a0 + a1) + (a2 + a3);
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// The step's scalars: decay, step_size, bc2_sqrt formed in double like torch's Python-side arithmetic, then applied in fp32; ema_w = (float)(1 - beta_t)
struct AdamwScalars { float decay, step_size, bc2_sqrt, ema_w; };

// One element.  -ffp-contract=off: no contraction either way, so p, m, v are the same bits with and without the average, which is one
// fp32 subtraction and one fmaf behind them.
template <bool EMA>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float& e, float coef, const AdamwScalars& h, float one_m_b1,
                                           float b2, float one_m_b2, float eps) {
  const float gi = g * coef;
  float pi = p * h.decay;
  const float mo = m;
  const float mi = mo + one_m_b1 * (gi - mo);          // torch: exp_avg.lerp_(grad, 1 - beta1)
  const float vi = fmaf(one_m_b2 * gi, gi, b2 * v);    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(vi) / h.bc2_sqrt + eps;
  pi -= h.step_size * (mi / denom);
  p = pi; m = mi; v = vi;
  if constexpr (EMA) e = fmaf(h.ema_w, pi - e, e);
}

// hyp null: the step's scalars are the launch argument `h` (host variant); else hyp[0..3] = decay, step_size, bc2_sqrt, ema_w (device
// variant: nothing about the call changes from one step to the next, so a captured graph of it can be replayed).
// 16-byte accesses when every buffer of the instantiation is 16-byte aligned (the way k_sumsq picks its path: the 191 M-parameter
// transformer's step is a bandwidth job), scalar accesses for the tail and for every other alignment.  e is not touched without EMA.
template <bool EMA>
__global__ void __launch_bounds__(256) k_adamw_clip(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ e, int64_t n,
                                                    const float* __restrict__ partials, int n_partials, float gscale, float max_norm,
                                                    const float* __restrict__ hyp, AdamwScalars h, float one_m_b1, float b2, float one_m_b2,
                                                    float eps, float* __restrict__ gnorm_out) {
  // every block re-derives the same clip coefficient from the same partials in the same order
  __shared__ float s_coef;
  if (threadIdx.x < 64) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_partials; i += 64) acc += partials[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
      const float nrm = sqrtf(acc);
      const float c = max_norm / (nrm + 1e-6f);  // torch clip_grad_norm_: coef clamped to 1
      s_coef = (max_norm > 0.f) ? fminf(c, 1.0f) : 1.0f;
      if (blockIdx.x == 0 && gnorm_out) gnorm_out[0] = nrm;
    }
  }
  __syncthreads();
  const float coef = s_coef * gscale;
  if (hyp) { h.decay = hyp[0]; h.step_size = hyp[1]; h.bc2_sqrt = hyp[2]; if constexpr (EMA) h.ema_w = hyp[3]; }
  const bool aligned = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (EMA ? (uintptr_t)e : 0)) & 15) == 0);
  const int64_t n4 = aligned ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m); float4* v4 = reinterpret_cast<float4*>(v); float4* e4 = reinterpret_cast<float4*>(e);
  for (int64_t i = first; i < n4; i += stride) {
    float4 pp = p4[i], mm = m4[i], vv = v4[i], ee = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EMA) ee = e4[i];
    const float4 gg = g4[i];
    adamw_elem<EMA>(pp.x, gg.x, mm.x, vv.x, ee.x, coef, h, one_m_b1, b2, one_m_b2, eps);
    adamw_elem<EMA>(pp.y, gg.y, mm.y, vv.y, ee.y, coef, h, one_m_b1, b2, one_m_b2, eps);
    adamw_elem<EMA>(pp.z, gg.z, mm.z, vv.z, ee.z, coef, h, one_m_b1, b2, one_m_b2, eps);
    adamw_elem<EMA>(pp.w, gg.w, mm.w, vv.w, ee.w, coef, h, one_m_b1, b2, one_m_b2, eps);
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
    if constexpr (EMA) e4[i] = ee;
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i], ei = 0.f;
    if constexpr (EMA) ei = e[i];
    adamw_elem<EMA>(pi, g[i], mi, vi, ei, coef, h, one_m_b1, b2, one_m_b2, eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) e[i] = ei;
  }
}

// beta_t = min(beta, (1 + t) / (10 + t)) with warm-up, beta without; w_t = (float)(1 - beta_t), in double on the host and in k_adamw_hyper
__host__ __device__ inline float ema_weight(double beta, int warmup, int t) {
  const double bt = warmup ? fmin(beta, (1.0 + (double)t) / (10.0 + (double)t)) : beta;
  return (float)(1.0 - bt);
}
__host__ __device__ inline AdamwScalars adamw_scalars(double lr, double b1, double b2, double wd, int t) {
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  return AdamwScalars{(float)(1.0 - lr * wd), (float)(lr / bc1), (float)sqrt(bc2), 0.f};
}

// The device-scalar step's scalars, hyp (8 floats behind the partial sums): formed from the device step counter exactly as launch_adamw
// forms them on the host; the counter is incremented first (step t = 1 for the first call).  hyp[3], the EMA weight, only with `ema`.
__global__ void k_adamw_hyper(int* __restrict__ step, const float* __restrict__ lr_dev, double b1, double b2, double wd, int ema, double ema_beta,
                              int ema_warmup, float* __restrict__ hyp) {
  const int t = step[0] + 1;
  step[0] = t;
  const double lr = (double)lr_dev[0] + (double)lr_dev[1];  // (hi, lo) float pair: ~48 bits of the host's double lr
  const AdamwScalars h = adamw_scalars(lr, b1, b2, wd, t);
  hyp[0] = h.decay;
  hyp[1] = h.step_size;
  hyp[2] = h.bc2_sqrt;
  if (ema) hyp[3] = ema_weight(ema_beta, ema_warmup, t);
}

int launch_adamw(const AdamwStep& a, hipStream_t s) {
  const bool dev = a.step_dev || a.lr_dev;
  if (dev) DQ_REQUIRE(a.n > 0 && a.lr_dev && a.step_dev, "adamw: need n > 0, the device learning rate and the device step counter");
  else DQ_REQUIRE(a.n > 0 && a.step >= 1, "adamw: need n > 0 and step >= 1");
  DQ_REQUIRE(!a.ema || (a.ema_decay >= 0.f && a.ema_decay < 1.f), "adamw + ema: ema_decay must satisfy 0 <= ema_decay < 1");  // (false for NaN)
  // (one grid for all four entries; the device-scalar step keeps 8 floats of the MSE_MAX_BLOCKS-float scratch for its scalars: the norm's
  // partial sums are then taken in the same order by all, for any n)
  const int grid = (int)std::min<int64_t>(cdiv(a.n, 256), MSE_MAX_BLOCKS - 8);
  float* hyp = dev ? a.partials + (MSE_MAX_BLOCKS - 8) : nullptr;
  AdamwScalars h{0.f, 0.f, 0.f, 0.f};
  if (dev) {
    hipLaunchKernelGGL(k_adamw_hyper, dim3(1), dim3(1), 0, s, a.step_dev, a.lr_dev, a.b1, a.b2, a.wd, a.ema ? 1 : 0, (double)a.ema_decay,
                       a.ema_warmup, hyp);
    DQ_LAUNCH_CHECK();
  } else {
    h = adamw_scalars(a.lr, a.b1, a.b2, a.wd, a.step);
    if (a.ema) h.ema_w = ema_weight((double)a.ema_decay, a.ema_warmup, a.step);
  }
  hipLaunchKernelGGL(k_sumsq, dim3(grid), dim3(256), 0, s, a.g, a.n, a.gscale, a.partials);
  DQ_LAUNCH_CHECK();
  const auto kernel = a.ema ? k_adamw_clip<true> : k_adamw_clip<false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.ema, a.n, a.partials, grid, a.gscale, a.max_norm,
                     (const float*)hyp, h, (float)(1.0 - a.b1), (float)a.b2, (float)(1.0 - a.b2), (float)a.eps, a.gnorm_out);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
