// Streaming (HBM-bound) kernels of the DDIM process: q_sample (K0), the sample epilogue, MSE loss + its gradient (K10), the held-out
// per-window MSE and the MS1 term of train_step.  (The sampler updates, K9: k_update.hip; clip + AdamW, K11: k_adamw.hip.)
// Reference arithmetic: dquartic/model/model.py:239-242 (q_sample), :319-322 (sample epilogue), :361 (mse_loss), :364-402 (the MS1 term).
// The element-wise kernels: V = 4 (16 B per lane) or V = 1 elements per lane and trip, grid-stride, no LDS.  One template per job (DESIGN.md
// section 36): k_q_sample<V, STACKED>, k_sample_finish<V>, k_mse_fwd_bwd<Target, V>, k_mse_per_window<Target>, k_mse_per_window_finish; the
// fp32 and the fp64 block tails are block_partial_sum and block_slice_sum.  Algorithmic bytes per element are stated per kernel.
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include "../../include/dq_hip.h"  // DQ_PRED_*
#include <algorithm>
#include <cmath>

namespace dq {

// V consecutive floats of p, counted in units of V (V = 4: one 16-byte access)
template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, int64_t i, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else v[0] = p[i];
}
template <int V>
__device__ __forceinline__ void store_v(float* __restrict__ p, int64_t i, const float (&v)[V]) {
  if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
  else p[i] = v[0];
}

// sa = sqrt(ab), sb = sqrt(1 - ab) of a sample's alpha-bar: q_sample's two coefficients, and the v target's
struct SqrtAb { float sa, sb; };
__device__ __forceinline__ SqrtAb sqrt_ab(float ab) { return {sqrtf(ab), sqrtf(1.0f - ab)}; }

// one float per block: the block's sum of acc (wave sums, then red[0] + red[1] + red[2] + red[3] left to right) -> dst[blockIdx.x]
__device__ __forceinline__ void block_partial_sum(float acc, float* __restrict__ dst) {
  __shared__ float red[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) dst[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// the fp64 counterpart (butterfly per wave, then (red[0] + red[1]) + (red[2] + red[3])) -> *dst
__device__ __forceinline__ void block_slice_sum(double acc, double* __restrict__ dst) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- K0: x_t = sqrt(ab[t_n]) * (2*x0-1) + sqrt(1-ab[t_n]) * noise : 12 B / element (2 reads + 1 write); 8 B with the noise drawn
// total, perv: the element count and the per-sample count in units of V (V = 1: a window whose RT*MZ is no multiple of 4 -- MZ = 2 with an
// odd RT -- where a float4 would straddle two windows).  STACKED (dq_tfm_eval_step): R repeats of B windows, sample
// n = r * B + b reads x0 row b (the clean window is shared by the repeats, never replicated) and its noise at n -- or, noise == nullptr,
// draws it from the counter-based generator of k_noise.hip at element 4 * e4 + j, draw index first_draw + r, and never writes it.
template <int V, bool STACKED>
__global__ void __launch_bounds__(256) k_q_sample(const float* __restrict__ alpha_bars, const float* __restrict__ x0,
                                                  const int64_t* __restrict__ t, const float* __restrict__ noise,
                                                  const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p, uint32_t first_draw,
                                                  float* __restrict__ x_t, int B, int64_t total, int64_t perv, int normalize) {
  uint64_t seed = 0;
  if constexpr (STACKED) seed = noise ? 0 : seed_p[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / perv;
    const SqrtAb c = sqrt_ab(alpha_bars[t[n]]);
    float x[V], nz[V], o[V];
    if constexpr (STACKED) {
      const int64_t e = i - n * perv, r = n / B, b = n - r * B;
      load_v<V>(x0, b * perv + e, x);
      if (noise) load_v<V>(noise, i, nz);
      else {
        const int64_t w = ids ? ids[b] : b;
        const uint32_t e0 = (uint32_t)e * (uint32_t)V, d = first_draw + (uint32_t)r;
#pragma unroll
        for (int j = 0; j < V; ++j) nz[j] = philox_normal(seed, w, e0 + (uint32_t)j, d);
      }
    } else {
      load_v<V>(x0, i, x);
      load_v<V>(noise, i, nz);
    }
    if (normalize) {
#pragma unroll
      for (int j = 0; j < V; ++j) x[j] = x[j] * 2.f - 1.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = c.sa * x[j] + c.sb * nz[j];
    store_v<V>(x_t, i, o);
  }
}

int launch_q_sample(const float* alpha_bars, const float* x0, const int64_t* t, const float* noise, float* x_t, int B, int64_t per,
                    int normalize, hipStream_t s, const NoiseStack* st) {
  if (st) {  // the stacked form refuses what the plain one serves one element at a time, and misaligned tensors
    DQ_REQUIRE(alpha_bars && x0 && t && x_t, "q_sample: null argument");
    DQ_REQUIRE(noise || st->seed, "q_sample: a null noise needs the seed (device memory)");
    DQ_REQUIRE(B > 0 && st->R > 0 && per > 0 && per % 4 == 0 && per <= (int64_t)0xffffffff,
               "q_sample: the stacked form needs B, repeats > 0 and a per-window element count that is a positive multiple of 4 below 2^32");
    DQ_REQUIRE(st->first_draw >= 0, "q_sample: the draw index must be >= 0");
    DQ_REQUIRE((((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)x_t) & 15) == 0, "q_sample: the stacked form's tensors must be 16-byte aligned");
  } else
    DQ_REQUIRE(B >= 0 && per >= 0, "q_sample: negative size");
  // 16 bytes per lane iff per % 4 == 0.  Alignment is not consulted: the plain form has always taken the caller's word for it
  const int V = per % 4 == 0 ? 4 : 1;
  const int64_t perv = per / V, total = (int64_t)(st ? st->R : 1) * B * perv;
  if (total == 0) return 0;
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 2048);
  auto k = st ? k_q_sample<4, true> : V == 4 ? k_q_sample<4, false> : k_q_sample<1, false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, alpha_bars, x0, t, noise, st ? st->ids : nullptr, st ? st->seed : nullptr,
                     (uint32_t)(st ? st->first_draw : 0), x_t, B, total, perv, normalize);
  DQ_LAUNCH_CHECK();
  return 0;
}

// ---- sample() epilogue (model.py:319-322): x = (x+1)/2 ; pred = ((2c-1)+1)/2 - x : 16 B / element
// (identity normalisation: x stays, pred_noise = ms2_cond - x)
template <int V>
__global__ void __launch_bounds__(256) k_sample_finish(const float* __restrict__ x, const float* __restrict__ ms2_cond,
                                                       float* __restrict__ out_x, float* __restrict__ out_noise, int64_t nv,
                                                       int normalize) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float v[V], c[V], o[V], p[V];
    load_v<V>(x, i, v);
    load_v<V>(ms2_cond, i, c);
    if (normalize) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o[j] = (v[j] + 1.f) * 0.5f;
        p[j] = ((c[j] * 2.f - 1.f) + 1.f) * 0.5f - o[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        o[j] = v[j];
        p[j] = c[j] - v[j];
      }
    }
    store_v<V>(out_x, i, o);
    store_v<V>(out_noise, i, p);
  }
}

int launch_sample_finish(const float* x, const float* ms2_cond, float* out_x, float* out_noise, int64_t n, int normalize,
                         hipStream_t s) {
  DQ_REQUIRE(n >= 0, "sample_finish: negative element count");
  if (n == 0) return 0;
  const int V = n % 4 == 0 ? 4 : 1;  // (the count alone; the sampler's buffers are 16-byte aligned)
  const int grid = (int)std::min<int64_t>(cdiv(n / V, 256), 2048);
  hipLaunchKernelGGL(V == 4 ? k_sample_finish<4> : k_sample_finish<1>, dim3(grid), dim3(256), 0, s, x, ms2_cond, out_x, out_noise, n / V,
                     normalize);
  DQ_LAUNCH_CHECK();
  return 0;
}

// ---- K10: loss = mean(w_b (pred - target)^2) ; grad = 2 * (pred - target) * w_b / n : 12 B / element (v: 16 B)
// partial sums go to ``partials`` (one per block, fixed order => deterministic); k_sum_partials sums them.  A Target is the device side of
// LossTarget for this kernel: sample(i, perv) is the per-sample part of the lane's V elements (element i in units of V, perv per sample in
// the same units), elems() their targets.
//   MseRead  the tensor itself, weight 1 (lw == nullptr: the noise of the eps objective), or z * tm + ta weighted by lw[t_b] (pred_type "x0",
//            model.py:372-376, 404).  The map belongs to the weighted form ONLY: z * 1 + 0 is not z (it turns a -0 into +0, and with it the
//            sign of a zero gradient), and the unweighted form never divides by perv
//   MseV     sa_b * noise - sb_b * (x0 * tm + ta) (pred_type "v_prediction"; k_level.hip's comments know this
//            arithmetic under the kernel's former name, k_mse_v_fwd_bwd), formed per element and never written,
//            weighted by lw[t_b] (lw == nullptr: 1)
struct MseRead {
  const float* z; const float* lw; const int64_t* t; float tm, ta;
  struct Sample { float w; };
  __device__ __forceinline__ Sample sample(int64_t i, int64_t perv) const { return {lw ? lw[t[i / perv]] : 1.f}; }
  template <int V>
  __device__ __forceinline__ void elems(const Sample&, int64_t i, float (&zt)[V]) const {
    load_v<V>(z, i, zt);
    if (lw) {
#pragma unroll
      for (int j = 0; j < V; ++j) zt[j] = zt[j] * tm + ta;
    }
  }
};
struct MseV {
  const float* noise; const float* x0; const float* alpha_bars; const float* lw; const int64_t* t; float tm, ta;
  struct Sample { float w; SqrtAb c; };
  __device__ __forceinline__ Sample sample(int64_t i, int64_t perv) const {
    const int64_t tb = t[i / perv];
    const SqrtAb c = sqrt_ab(alpha_bars[tb]);  // (asked for before the weight: the two loads then fly together)
    return {lw ? lw[tb] : 1.f, c};
  }
  template <int V>
  __device__ __forceinline__ void elems(const Sample& sm, int64_t i, float (&zt)[V]) const {
    float x[V], z[V];
    load_v<V>(x0, i, x);
    load_v<V>(noise, i, z);
#pragma unroll
    for (int j = 0; j < V; ++j) zt[j] = sm.c.sa * z[j] - sm.c.sb * (x[j] * tm + ta);
  }
};

template <class Target, int V>
__global__ void __launch_bounds__(256) k_mse_fwd_bwd(const float* __restrict__ pred, const Target tg, float* __restrict__ grad,
                                                     float* __restrict__ partials, int64_t nv, int64_t perv, float gscale) {
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const typename Target::Sample sm = tg.sample(i, perv);
    float e[V], zt[V], g[V];
    load_v<V>(pred, i, e);
    tg.template elems<V>(sm, i, zt);
    const float gs = gscale * sm.w;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float d = e[j] - zt[j];
      sq += d * d;
      g[j] = d * gs;
    }
    acc += sm.w * sq;
    if (grad) store_v<V>(grad, i, g);
  }
  block_partial_sum(acc, partials);
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

LossTarget loss_target(int pred_type, const float* x0, const float* noise, const float* alpha_bars, float cm, float ca, const float* lw,
                       const int64_t* t) {
  LossTarget tg;
  tg.t = t;
  if (pred_type == DQ_PRED_EPS) {  // model.py:361: the noise, weight 1; where the caller keeps none, it is drawn again
    tg.z = noise;
    if (!noise) tg.kind = TargetKind::DRAWN;
    return tg;
  }
  tg.tm = cm; tg.ta = ca; tg.lw = lw;
  if (pred_type == DQ_PRED_X0) { tg.z = x0; tg.shared = true; }  // model.py:372-376, 404: the normalised x0, weighted by lw[t_b]
  else {  // sa_b noise - sb_b (normalised x0), weighted by lw[t_b] (null: 1)
    tg.kind = TargetKind::V; tg.z = noise; tg.x0 = x0; tg.alpha_bars = alpha_bars;
  }
  return tg;
}

int launch_mse_fwd_bwd(const float* pred, const LossTarget& tg, float* loss_out, float* grad_out, float* partials, int B, int64_t per,
                       hipStream_t s, int* defer_sum) {
  const bool v = tg.kind == TargetKind::V;
  DQ_REQUIRE(tg.kind != TargetKind::DRAWN && !tg.stacked, "mse: a drawn or stacked target belongs to the per-window form");
  DQ_REQUIRE(pred && tg.z && partials && (loss_out || defer_sum) && (!v || (tg.x0 && tg.alpha_bars && tg.t)), "mse: null argument");
  DQ_REQUIRE(B > 0 && per > 0, "mse: B and the per-sample element count must be positive");
  DQ_REQUIRE(!tg.lw || tg.t, "mse: the weighted form needs t");
  const int64_t n = (int64_t)B * per;
  // Who takes 16 bytes per lane -- V decides the block partition, hence the bits of the sum, so each form keeps the predicate it was built
  // with.  Read target: the counts alone (n, and per where a lane must not straddle two samples' weights); alignment is not consulted.
  // v target: per, and the alignment of every tensor it touches.
  const uintptr_t bits = (uintptr_t)pred | (uintptr_t)tg.x0 | (uintptr_t)tg.z | (uintptr_t)grad_out;
  const bool vec = v ? per % 4 == 0 && (bits & 15) == 0 : n % 4 == 0 && (!tg.lw || per % 4 == 0);
  const int V = vec ? 4 : 1;
  const int grid = (int)std::min<int64_t>(cdiv(n / V, 256), MSE_MAX_BLOCKS);
  const float gscale = 2.0f / (float)n;
  const int64_t perv = per / V;  // (an unweighted read target never looks at it: there per need not divide by V)
  if (v) {
    auto k = vec ? k_mse_fwd_bwd<MseV, 4> : k_mse_fwd_bwd<MseV, 1>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, pred, MseV{tg.z, tg.x0, tg.alpha_bars, tg.lw, tg.t, tg.tm, tg.ta}, grad_out, partials,
                       n / V, perv, gscale);
  } else {
    auto k = vec ? k_mse_fwd_bwd<MseRead, 4> : k_mse_fwd_bwd<MseRead, 1>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, pred, MseRead{tg.z, tg.lw, tg.t, tg.tm, tg.ta}, grad_out, partials, n / V, perv,
                       gscale);
  }
  DQ_LAUNCH_CHECK();
  if (defer_sum) { *defer_sum = grid; return 0; }  // the caller sums the partials later (launch_sum_partials(partials, grid, 1 / n, loss_out))
  return launch_sum_partials(partials, grid, 1.0f / (float)n, loss_out, s);
}

// ---- held-out loss (dq_mse_per_window*, dq_eval_step, dq_tfm_eval_step): per-window MSE and its weighted mean, forward only : 8 B / element
// (v: 12 B, drawn: 4 B).  The target in fp32 (the expressions of k_mse_fwd_bwd's targets, except that the read target is ALWAYS mapped:
// only d * d is used here), d = (double)out - (double)target, d * d summed in fp64.  One block per (slice of MSE_PW_SLICE elements, window):
// the partition of a window depends on `per` alone, never on B, and the slices are added in index order -- no atomics, so a window's value
// does not depend on the batch around it.  scratch: one double per slice.  A Target here: window(n, per) is the per-window part, at() the
// target of element i of that window.
//   PwRead   z[row] * tm + ta, row = n (one row per window) or, SHARED, n % Bt (Bt = B under R repeats: the row shared by the repeats; an
//            instantiation of its own, so that the plain form pays for no remainder)
//   PwV      sa_n * noise - sb_n * (x0 * tm + ta)
//   PwDrawn  the noise of (r, b) = (n / B, n % B) drawn here at element (uint32_t)i, draw index first_draw + r, mapped like PwRead
template <bool SHARED>
struct PwRead {
  const float* z; uint32_t Bt; float tm, ta;
  struct Window { const float* z; };
  __device__ __forceinline__ Window window(int64_t n, int64_t per) const {
    return {z + (SHARED ? (int64_t)((uint32_t)n % Bt) : n) * per};  // (n and Bt are below 2^16: a 32-bit remainder, once per block)
  }
  __device__ __forceinline__ float at(const Window& w, int64_t i) const { return w.z[i] * tm + ta; }
};
struct PwV {
  const float* noise; const float* x0; const float* alpha_bars; const int64_t* t; float tm, ta;
  struct Window { const float* z; const float* x; SqrtAb c; };
  __device__ __forceinline__ Window window(int64_t n, int64_t per) const { return {noise + n * per, x0 + n * per, sqrt_ab(alpha_bars[t[n]])}; }
  __device__ __forceinline__ float at(const Window& w, int64_t i) const { return w.c.sa * w.z[i] - w.c.sb * (w.x[i] * tm + ta); }
};
struct PwDrawn {
  const int64_t* ids; const uint64_t* seed_p; uint32_t first_draw; int B; float tm, ta;
  struct Window { uint64_t seed; int64_t id; uint32_t draw; };
  __device__ __forceinline__ Window window(int64_t n, int64_t) const {
    const int64_t r = n / B, b = n - r * B;
    return {seed_p[0], ids ? ids[b] : b, first_draw + (uint32_t)r};
  }
  __device__ __forceinline__ float at(const Window& w, int64_t i) const { return philox_normal(w.seed, w.id, (uint32_t)i, w.draw) * tm + ta; }
};

template <class Target>
__global__ void __launch_bounds__(256) k_mse_per_window(const float* __restrict__ out, const Target tg, double* __restrict__ slices, int64_t per,
                                                        int nslices) {
  const int64_t n = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * MSE_PW_SLICE, i1 = min(per, i0 + MSE_PW_SLICE);
  const float* __restrict__ o = out + n * per;
  const typename Target::Window w = tg.window(n, per);
  double acc = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float zt = tg.at(w, i);
    const double d = (double)o[i] - (double)zt;
    acc += d * d;
  }
  block_slice_sum(acc, slices + n * nslices + blockIdx.x);
}

// block r: per_window[r * B + b] = (float)(sum of the window's slices / per) and loss[r] = (float)(sum_b lw[t[r, b]] * (sum_b / per) / B),
// both sums in fp64 in index order (256 windows at a time are staged in LDS, thread 0 adds them up), each result rounded to fp32 once.
// lw == nullptr: weight 1.  Grid R: one block per repeat (1 without a stack).
__global__ void __launch_bounds__(256) k_mse_per_window_finish(const double* __restrict__ slices, const float* __restrict__ lw,
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

int64_t mse_per_window_scratch_bytes(int B, int64_t per) {
  if (B < 1 || per < 1) return -1;
  return (int64_t)sizeof(double) * B * ((per + MSE_PW_SLICE - 1) / MSE_PW_SLICE);
}

int launch_mse_per_window(const float* out, const LossTarget& tg, float* per_window, float* loss_out, void* scratch, int64_t scratch_bytes,
                          int B, int R, int64_t per, hipStream_t s) {
  const bool v = tg.kind == TargetKind::V, drawn = tg.kind == TargetKind::DRAWN;
  DQ_REQUIRE(out && per_window && loss_out && scratch && (drawn || tg.z) && (!v || (tg.x0 && tg.alpha_bars && tg.t)),
             "mse_per_window: null argument");
  DQ_REQUIRE(B > 0 && R > 0 && (int64_t)R * B <= 65535 && per > 0 && (!tg.stacked || per <= (int64_t)0xffffffff),
             "mse_per_window: need B, repeats > 0, repeats * B <= 65535 and per > 0 (a stacked target: per < 2^32)");
  DQ_REQUIRE(tg.stacked ? !v : !drawn && R == 1, "mse_per_window: repeats and a drawn target need a stacked target, the v target a plain one");
  const int N = R * B;
  DQ_REQUIRE(!drawn || tg.seed, "mse_per_window: a null target needs the seed (device memory)");
  DQ_REQUIRE(!tg.stacked || drawn || tg.Bt == B || tg.Bt == N, "mse_per_window: the target has B or repeats * B windows");
  DQ_REQUIRE(tg.first_draw >= 0, "mse_per_window: the draw index must be >= 0");
  DQ_REQUIRE(!tg.lw || tg.t, "mse_per_window: the weighted form needs t");
  DQ_REQUIRE(scratch_bytes >= mse_per_window_scratch_bytes(N, per), "mse_per_window: scratch too small (dq_mse_per_window_scratch_bytes(repeats * B, per))");
  DQ_REQUIRE(((uintptr_t)scratch & 7) == 0, "mse_per_window: scratch must be 8-byte aligned");
  const int64_t nslices = (per + MSE_PW_SLICE - 1) / MSE_PW_SLICE;
  DQ_REQUIRE(nslices <= INT32_MAX, "mse_per_window: window too large");
  const dim3 grid((unsigned)nslices, N);
  double* slices = (double*)scratch;
  if (v)
    hipLaunchKernelGGL(k_mse_per_window<PwV>, grid, dim3(256), 0, s, out, PwV{tg.z, tg.x0, tg.alpha_bars, tg.t, tg.tm, tg.ta}, slices, per,
                       (int)nslices);
  else if (drawn)
    hipLaunchKernelGGL(k_mse_per_window<PwDrawn>, grid, dim3(256), 0, s, out,
                       PwDrawn{tg.ids, tg.seed, (uint32_t)tg.first_draw, B, tg.tm, tg.ta}, slices, per, (int)nslices);
  else if (tg.stacked && tg.Bt != N)
    hipLaunchKernelGGL(k_mse_per_window<PwRead<true>>, grid, dim3(256), 0, s, out, PwRead<true>{tg.z, (uint32_t)tg.Bt, tg.tm, tg.ta}, slices, per,
                       (int)nslices);
  else
    hipLaunchKernelGGL(k_mse_per_window<PwRead<false>>, grid, dim3(256), 0, s, out, PwRead<false>{tg.z, (uint32_t)N, tg.tm, tg.ta}, slices, per,
                       (int)nslices);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mse_per_window_finish, dim3(R), dim3(256), 0, s, (const double*)slices, tg.lw, tg.t, per_window, loss_out, B, per,
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
