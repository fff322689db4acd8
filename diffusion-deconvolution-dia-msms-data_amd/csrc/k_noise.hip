// Stochastic half of the sampler: standard-normal noise from a counter-based generator evaluated inside the kernels
// (dq_philox.h), keyed by (seed, window id, element inside the window, draw index).  Seed and window ids are read from DEVICE memory, so a
// captured step is replayed unchanged under a new seed or for other windows.
//   k_randn          (B, per_window) normals of one draw index (x_T: draw 0)                                  4 B / element
//   k_ddim_step_sto  k_ddim_step (k_stream.hip) plus sigma * z: x_prev = sap*x0 + c*eps + sigma*z (t > 0)      12 B / element
//   k_ddim_step_sto_g, _g_1  the same update on the guided network output, x_prev mirrored   20 B / element
// 16 B per lane, grid-stride, no LDS, like the stream kernels next door.
#include "dq_common.h"
#include "dq_guide.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include <algorithm>

namespace dq {

// out[b * per + e] = z(seed, ids ? ids[b] : b, e, draw).  16-byte stores when `out` is 16-byte aligned (a lane's four elements may straddle
// two windows when per % 4 != 0: each element finds its own), scalar stores for the tail and for every other alignment.
__global__ void __launch_bounds__(256) k_randn(float* __restrict__ out, const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p,
                                               uint32_t draw, int64_t n, int64_t per) {
  const uint64_t seed = seed_p[0];
  const int64_t n4 = (((uintptr_t)out & 15) == 0) ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = first; i < n4; i += stride) {
    int64_t b = (4 * i) / per, e = 4 * i - b * per;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      while (e >= per) { e -= per; ++b; }
      v[j] = philox_normal(seed, ids ? ids[b] : b, (uint32_t)e, draw);
      ++e;
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    const int64_t b = i / per;
    out[i] = philox_normal(seed, ids ? ids[b] : b, (uint32_t)(i - b * per), draw);
  }
}

int launch_randn(float* out, const int64_t* ids, const uint64_t* seed_dev, int draw, int B, int64_t per_window, hipStream_t s) {
  DQ_REQUIRE(out && seed_dev, "randn: null output or seed");
  DQ_REQUIRE(B >= 0 && per_window >= 0 && per_window <= (int64_t)0xffffffff, "randn: need B >= 0 and 0 <= per_window < 2^32");
  DQ_REQUIRE(draw >= 0, "randn: the draw index must be >= 0");
  DQ_REQUIRE(((uintptr_t)out & 3) == 0, "randn: the output must be 4-byte aligned");
  const int64_t n = (int64_t)B * per_window;
  if (n == 0) return 0;
  const int grid = (int)std::min<int64_t>(((n + 3) / 4 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_randn, dim3(grid), dim3(256), 0, s, out, ids, seed_dev, (uint32_t)draw, n, per_window);
  DQ_LAUNCH_CHECK();
  return 0;
}

// k_ddim_step's arithmetic for x0 and eps (both objectives), then x_prev = (sap*x0 + c*eps) + sigma*z on a step with t > 0, x0 on the t == 0
// step (sap < 0: no noise drawn, k_ddim_step's result bit for bit).  coef: rows [sa, sb, sap, c]; sigma: one float per row.  step_ptr set
// (graph replay): row and draw index 1 + step come from the device step counter; null: row 0 and the `draw` argument.  The window of
// float4 i is i / per4 (per_window % 4 == 0), the element 4 * (i % per4) + j.
struct StoRow { float sa, sb, sap, c, sigma; bool last; };

// the step's row; with step_ptr (graph replay) the row AND the draw index 1 + step come from the device step counter
__device__ __forceinline__ StoRow sto_row(const float* coef, const float* sigma_tab, const int* step_ptr, uint32_t& draw) {
  if (step_ptr) { const int st = step_ptr[0]; coef += 4 * st; sigma_tab += st; draw = 1u + (uint32_t)st; }
  return StoRow{coef[0], coef[1], coef[2], coef[3], sigma_tab[0], coef[2] < 0.f};
}

// One element: x_prev from x, the network output v (or, guided, g in its place: dq_guide.h) and the noise of element e of window w; the
// step's eps by reference
template <bool PRED_X0>
__device__ __forceinline__ float sto_elem(const StoRow& r, float x, float v, uint64_t seed, int64_t w, uint32_t e, uint32_t draw, float& ep) {
  float x0;
  if (PRED_X0) { x0 = v; ep = (x - r.sa * x0) / r.sb; }
  else         { ep = v; x0 = (x - r.sb * ep) / r.sa; }
  float z = 0.f;
  if (!r.last) z = philox_normal(seed, w, e, draw);  // (uniform: the t == 0 step draws nothing)
  return r.last ? x0 : (r.sap * x0 + r.c * ep) + r.sigma * z;
}

template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_ddim_step_sto(const float* __restrict__ x_t, const float* __restrict__ eps, float* __restrict__ x_prev,
                                                       float* __restrict__ eps_out, const float* __restrict__ coef,
                                                       const float* __restrict__ sigma_tab, const int64_t* __restrict__ ids,
                                                       const uint64_t* __restrict__ seed_p, uint32_t draw, int64_t n4, int64_t per4,
                                                       const int* __restrict__ step_ptr) {
  const StoRow r = sto_row(coef, sigma_tab, step_ptr, draw);
  const uint64_t seed = seed_p[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(x_t)[i];
    const float4 e = reinterpret_cast<const float4*>(eps)[i];
    const float xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
    const int64_t b = i / per4;
    const uint32_t e0 = (uint32_t)(i - b * per4) * 4u;
    const int64_t w = ids ? ids[b] : b;
    float ov[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = sto_elem<PRED_X0>(r, xv[j], ev[j], seed, w, e0 + (uint32_t)j, draw, dv[j]);
    reinterpret_cast<float4*>(x_prev)[i] = make_float4(ov[0], ov[1], ov[2], ov[3]);
    if (PRED_X0 && eps_out) reinterpret_cast<float4*>(eps_out)[i] = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
}

// The guided update (dq_guide.h): sto_elem on g = u + w (c - u) in place of the network output.  The noise of window b
// is drawn ONCE, keyed by the window's id as above, and the result goes through both stores: x_prev and, when given, x_mirror (the
// unconditional half's copy of x for the next forward) -- the two halves never see different noise.  eps_out (nullable) receives the
// guided eps under either objective.  20 B / element with the mirror, + 4 with eps_out.  x_prev may alias x_t, eps_out net_c.
template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_ddim_step_sto_g(const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror,
                                                         float* eps_out, const float* __restrict__ coef, const float* __restrict__ sigma_tab,
                                                         const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p, uint32_t draw,
                                                         float gw, int64_t n4, int64_t per4, const int* __restrict__ step_ptr) {
  const StoRow r = sto_row(coef, sigma_tab, step_ptr, draw);
  const uint64_t seed = seed_p[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(x_t)[i];
    const float4 c = reinterpret_cast<const float4*>(net_c)[i];
    const float4 u = reinterpret_cast<const float4*>(net_u)[i];
    const float xv[4] = {x.x, x.y, x.z, x.w}, cv[4] = {c.x, c.y, c.z, c.w}, uv[4] = {u.x, u.y, u.z, u.w};
    const int64_t b = i / per4;
    const uint32_t e0 = (uint32_t)(i - b * per4) * 4u;
    const int64_t w = ids ? ids[b] : b;
    float ov[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = sto_elem<PRED_X0>(r, xv[j], guide(cv[j], uv[j], gw), seed, w, e0 + (uint32_t)j, draw, dv[j]);
    const float4 o = make_float4(ov[0], ov[1], ov[2], ov[3]);
    reinterpret_cast<float4*>(x_prev)[i] = o;
    if (x_mirror) reinterpret_cast<float4*>(x_mirror)[i] = o;
    if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
}

// the same, one element per lane and step: a per-window count that is no multiple of 4, pointers that are not 16-byte aligned
template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_ddim_step_sto_g_1(const float* x_t, const float* net_c, const float* net_u, float* x_prev,
                                                           float* x_mirror, float* eps_out, const float* __restrict__ coef,
                                                           const float* __restrict__ sigma_tab, const int64_t* __restrict__ ids,
                                                           const uint64_t* __restrict__ seed_p, uint32_t draw, float gw, int64_t n, int64_t per,
                                                           const int* __restrict__ step_ptr) {
  const StoRow r = sto_row(coef, sigma_tab, step_ptr, draw);
  const uint64_t seed = seed_p[0];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per;
    float ep;
    const float o = sto_elem<PRED_X0>(r, x_t[i], guide(net_c[i], net_u[i], gw), seed, ids ? ids[b] : b, (uint32_t)(i - b * per), draw, ep);
    x_prev[i] = o;
    if (x_mirror) x_mirror[i] = o;
    if (eps_out) eps_out[i] = ep;
  }
}

int launch_ddim_step_sto_guided(const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* eps_out,
                                const float* coef_dev, const float* sigma_dev, const int64_t* ids, const uint64_t* seed_dev, int draw, float w,
                                int pred_x0, int B, int64_t per_window, const int* step_ptr, hipStream_t s) {
  DQ_REQUIRE(x_t && net_c && net_u && x_prev && coef_dev && sigma_dev && seed_dev, "ddim_step_sto_guided: null argument");
  DQ_REQUIRE(B >= 0 && per_window >= 0 && per_window <= (int64_t)0xffffffff, "ddim_step_sto_guided: need B >= 0 and 0 <= per_window < 2^32");
  DQ_REQUIRE(draw >= 0, "ddim_step_sto_guided: the draw index must be >= 0");
  const uintptr_t bits = (uintptr_t)x_t | (uintptr_t)net_c | (uintptr_t)net_u | (uintptr_t)x_prev | (uintptr_t)x_mirror | (uintptr_t)eps_out;
  DQ_REQUIRE((bits & 3) == 0, "ddim_step_sto_guided: tensors must be 4-byte aligned");
  const int64_t n = (int64_t)B * per_window;
  if (n == 0) return 0;
  if (per_window % 4 != 0 || (bits & 15) != 0) {
    const int grid1 = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (pred_x0)
      hipLaunchKernelGGL(k_ddim_step_sto_g_1<true>, dim3(grid1), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, eps_out, coef_dev, sigma_dev,
                         ids, seed_dev, (uint32_t)draw, w, n, per_window, step_ptr);
    else
      hipLaunchKernelGGL(k_ddim_step_sto_g_1<false>, dim3(grid1), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, eps_out, coef_dev, sigma_dev,
                         ids, seed_dev, (uint32_t)draw, w, n, per_window, step_ptr);
    DQ_LAUNCH_CHECK();
    return 0;
  }
  const int grid = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  if (pred_x0)
    hipLaunchKernelGGL(k_ddim_step_sto_g<true>, dim3(grid), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, eps_out, coef_dev, sigma_dev, ids,
                       seed_dev, (uint32_t)draw, w, n / 4, per_window / 4, step_ptr);
  else
    hipLaunchKernelGGL(k_ddim_step_sto_g<false>, dim3(grid), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, eps_out, coef_dev, sigma_dev, ids,
                       seed_dev, (uint32_t)draw, w, n / 4, per_window / 4, step_ptr);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_ddim_step_sto(const float* x_t, const float* eps, float* x_prev, float* eps_out, const float* coef_dev, const float* sigma_dev,
                         const int64_t* ids, const uint64_t* seed_dev, int draw, int pred_x0, int B, int64_t per_window,
                         const int* step_ptr, hipStream_t s) {
  DQ_REQUIRE(x_t && eps && x_prev && coef_dev && sigma_dev && seed_dev, "ddim_step_sto: null argument");
  DQ_REQUIRE(B >= 0 && per_window >= 0 && per_window % 4 == 0 && per_window <= (int64_t)0xffffffff,
             "ddim_step_sto: need B >= 0 and a per-window element count that is a multiple of 4 below 2^32");
  DQ_REQUIRE(draw >= 0, "ddim_step_sto: the draw index must be >= 0");
  DQ_REQUIRE((((uintptr_t)x_t | (uintptr_t)eps | (uintptr_t)x_prev | (uintptr_t)eps_out) & 15) == 0, "ddim_step_sto: tensors must be 16-byte aligned");
  const int64_t n4 = (int64_t)B * (per_window / 4);
  if (n4 == 0) return 0;
  const int grid = (int)std::min<int64_t>((n4 + 255) / 256, 2048);
  if (pred_x0)
    hipLaunchKernelGGL(k_ddim_step_sto<true>, dim3(grid), dim3(256), 0, s, x_t, eps, x_prev, eps_out, coef_dev, sigma_dev, ids, seed_dev,
                       (uint32_t)draw, n4, per_window / 4, step_ptr);
  else
    hipLaunchKernelGGL(k_ddim_step_sto<false>, dim3(grid), dim3(256), 0, s, x_t, eps, x_prev, eps_out, coef_dev, sigma_dev, ids, seed_dev,
                       (uint32_t)draw, n4, per_window / 4, step_ptr);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
