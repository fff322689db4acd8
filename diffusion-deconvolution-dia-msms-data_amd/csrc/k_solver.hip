// Update of the step-consistent samplers: one linear multistep row per step,
//   x_prev = cx * x + c0 * x0 + c1 * x0_hist          (DPM-Solver++(2M), data prediction; c1 == 0: first order == strided DDIM, eta = 0)
// with x0 the network output (x0 objective) or (x - sb * e) / sa (eps objective), optionally clamped to [-clip, clip] before it is used and
// before it becomes the next step's history.  cx < 0 marks the last row: x_prev = x0.
//   k_solver_step    16 B per lane: reads x, net (and hist when c1 != 0), writes x_prev, hist (and eps when asked)      20 - 24 B / element
//   k_solver_step_1  the same expressions, one element per lane: counts that are no multiple of 4, pointers that are not 16-byte aligned
//   k_solver_step_g, _g_1  the same update on the guided network output, x_prev mirrored       28 - 32 B / element
// Element-wise: x_prev may alias x_t, eps_out may alias net, the history is updated in place (no __restrict__ on those).  Grid-stride, no
// LDS, no atomics, like the stream kernels next door.
#include "dq_common.h"
#include "dq_guide.h"
#include "dq_kernels.h"
#include <algorithm>

namespace dq {

struct SolverRow { float sa, sb, cx, c0, c1; };

__device__ __forceinline__ SolverRow solver_row(const float* coef, const float* c1_tab, const int* step_ptr) {
  if (step_ptr) { const int st = step_ptr[0]; coef += 4 * st; c1_tab += st; }  // graph replay: this step's row
  return SolverRow{coef[0], coef[1], coef[2], coef[3], c1_tab[0]};
}

// One element.  `h` is read by the caller only when c1 != 0.  Returns x_prev; x0 (clamped) and eps by reference.
template <bool PRED_X0>
__device__ __forceinline__ float solver_elem(const SolverRow& r, float clip, float x, float v, float h, float& x0, float& ep) {
  if (PRED_X0) { x0 = v; }
  else         { ep = v; x0 = (x - r.sb * ep) / r.sa; }
  bool clamped = false;
  if (clip > 0.f) {
    if (x0 < -clip) { x0 = -clip; clamped = true; }
    else if (x0 > clip) { x0 = clip; clamped = true; }
  }
  if (PRED_X0 || clamped) ep = (x - r.sa * x0) / r.sb;  // eps consistent with the x0 that is used
  if (r.cx < 0.f) return x0;
  const float y = r.cx * x + r.c0 * x0;
  return r.c1 != 0.f ? y + r.c1 * h : y;
}

template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_solver_step(const float* x_t, const float* net, float* x_prev, float* hist, float* eps_out,
                                                     const float* __restrict__ coef, const float* __restrict__ c1_tab, float clip,
                                                     int64_t n4, const int* __restrict__ step_ptr) {
  const SolverRow r = solver_row(coef, c1_tab, step_ptr);
  const bool rd_hist = r.c1 != 0.f && r.cx >= 0.f;  // (uniform) the first step's history is uninitialised memory: never read
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(x_t)[i];
    const float4 v = reinterpret_cast<const float4*>(net)[i];
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rd_hist) h = reinterpret_cast<const float4*>(hist)[i];
    const float xv[4] = {x.x, x.y, x.z, x.w}, vv[4] = {v.x, v.y, v.z, v.w}, hv[4] = {h.x, h.y, h.z, h.w};
    float ov[4], zv[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = solver_elem<PRED_X0>(r, clip, xv[j], vv[j], hv[j], zv[j], dv[j]);
    reinterpret_cast<float4*>(x_prev)[i] = make_float4(ov[0], ov[1], ov[2], ov[3]);
    if (hist) reinterpret_cast<float4*>(hist)[i] = make_float4(zv[0], zv[1], zv[2], zv[3]);
    if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
}

template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_solver_step_1(const float* x_t, const float* net, float* x_prev, float* hist, float* eps_out,
                                                       const float* __restrict__ coef, const float* __restrict__ c1_tab, float clip,
                                                       int64_t n, const int* __restrict__ step_ptr) {
  const SolverRow r = solver_row(coef, c1_tab, step_ptr);
  const bool rd_hist = r.c1 != 0.f && r.cx >= 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = x_t[i], v = net[i];
    const float h = rd_hist ? hist[i] : 0.f;
    float x0, ep;
    const float o = solver_elem<PRED_X0>(r, clip, x, v, h, x0, ep);
    x_prev[i] = o;
    if (hist) hist[i] = x0;
    if (eps_out) eps_out[i] = ep;
  }
}

// The guided update (dq_guide.h): solver_elem on g = u + w (c - u) in place of the network output, so the clamp, the
// history and eps_out all see the guided quantities; the result to x_prev and, when x_mirror is given, to x_mirror as well (the
// unconditional half's copy of x for the next forward).  28 - 32 B / element with the mirror (reads x, c, u and hist when c1 != 0; writes
// x_prev, x_mirror, hist), + 4 with eps_out.  A null history is never read, whatever c1.  The aliasing rules are k_solver_step's.
template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_solver_step_g(const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror,
                                                       float* hist, float* eps_out, const float* __restrict__ coef,
                                                       const float* __restrict__ c1_tab, float clip, float w, int64_t n4,
                                                       const int* __restrict__ step_ptr) {
  const SolverRow r = solver_row(coef, c1_tab, step_ptr);
  const bool rd_hist = hist && r.c1 != 0.f && r.cx >= 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(x_t)[i];
    const float4 c = reinterpret_cast<const float4*>(net_c)[i];
    const float4 u = reinterpret_cast<const float4*>(net_u)[i];
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rd_hist) h = reinterpret_cast<const float4*>(hist)[i];
    const float xv[4] = {x.x, x.y, x.z, x.w}, cv[4] = {c.x, c.y, c.z, c.w}, uv[4] = {u.x, u.y, u.z, u.w}, hv[4] = {h.x, h.y, h.z, h.w};
    float ov[4], zv[4], dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = solver_elem<PRED_X0>(r, clip, xv[j], guide(cv[j], uv[j], w), hv[j], zv[j], dv[j]);
    const float4 o = make_float4(ov[0], ov[1], ov[2], ov[3]);
    reinterpret_cast<float4*>(x_prev)[i] = o;
    if (x_mirror) reinterpret_cast<float4*>(x_mirror)[i] = o;
    if (hist) reinterpret_cast<float4*>(hist)[i] = make_float4(zv[0], zv[1], zv[2], zv[3]);
    if (eps_out) reinterpret_cast<float4*>(eps_out)[i] = make_float4(dv[0], dv[1], dv[2], dv[3]);
  }
}

template <bool PRED_X0>
__global__ void __launch_bounds__(256) k_solver_step_g_1(const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror,
                                                         float* hist, float* eps_out, const float* __restrict__ coef,
                                                         const float* __restrict__ c1_tab, float clip, float w, int64_t n,
                                                         const int* __restrict__ step_ptr) {
  const SolverRow r = solver_row(coef, c1_tab, step_ptr);
  const bool rd_hist = hist && r.c1 != 0.f && r.cx >= 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float h = rd_hist ? hist[i] : 0.f;
    float x0, ep;
    const float o = solver_elem<PRED_X0>(r, clip, x_t[i], guide(net_c[i], net_u[i], w), h, x0, ep);
    x_prev[i] = o;
    if (x_mirror) x_mirror[i] = o;
    if (hist) hist[i] = x0;
    if (eps_out) eps_out[i] = ep;
  }
}

int launch_solver_step_guided(const float* x_t, const float* net_c, const float* net_u, float* x_prev, float* x_mirror, float* hist,
                              float* eps_out, const float* coef_dev, const float* c1_dev, float clip, float w, int pred_x0, int64_t n,
                              const int* step_ptr, hipStream_t s) {
  DQ_REQUIRE(x_t && net_c && net_u && x_prev && coef_dev && c1_dev, "solver_step_guided: null argument");
  DQ_REQUIRE(n >= 0, "solver_step_guided: negative element count");
  const uintptr_t bits = (uintptr_t)x_t | (uintptr_t)net_c | (uintptr_t)net_u | (uintptr_t)x_prev | (uintptr_t)x_mirror | (uintptr_t)hist |
                         (uintptr_t)eps_out;
  DQ_REQUIRE((bits & 3) == 0, "solver_step_guided: tensors must be 4-byte aligned");
  if (n == 0) return 0;
  if (!(clip > 0.f)) clip = 0.f;  // (NaN and negatives: off)
  if (n % 4 != 0 || (bits & 15) != 0) {
    const int grid1 = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (pred_x0) hipLaunchKernelGGL(k_solver_step_g_1<true>, dim3(grid1), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, hist, eps_out, coef_dev, c1_dev, clip, w, n, step_ptr);
    else hipLaunchKernelGGL(k_solver_step_g_1<false>, dim3(grid1), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, hist, eps_out, coef_dev, c1_dev, clip, w, n, step_ptr);
    DQ_LAUNCH_CHECK();
    return 0;
  }
  const int grid = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  if (pred_x0) hipLaunchKernelGGL(k_solver_step_g<true>, dim3(grid), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, hist, eps_out, coef_dev, c1_dev, clip, w, n / 4, step_ptr);
  else hipLaunchKernelGGL(k_solver_step_g<false>, dim3(grid), dim3(256), 0, s, x_t, net_c, net_u, x_prev, x_mirror, hist, eps_out, coef_dev, c1_dev, clip, w, n / 4, step_ptr);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_solver_step(const float* x_t, const float* net, float* x_prev, float* hist, float* eps_out, const float* coef_dev,
                       const float* c1_dev, float clip, int pred_x0, int64_t n, const int* step_ptr, hipStream_t s) {
  DQ_REQUIRE(x_t && net && x_prev && coef_dev && c1_dev, "solver_step: null argument");
  DQ_REQUIRE(n >= 0, "solver_step: negative element count");
  DQ_REQUIRE((((uintptr_t)x_t | (uintptr_t)net | (uintptr_t)x_prev | (uintptr_t)hist | (uintptr_t)eps_out) & 3) == 0,
             "solver_step: tensors must be 4-byte aligned");
  if (n == 0) return 0;
  if (!(clip > 0.f)) clip = 0.f;  // (NaN and negatives: off)
  const bool vec = n % 4 == 0 && (((uintptr_t)x_t | (uintptr_t)net | (uintptr_t)x_prev | (uintptr_t)hist | (uintptr_t)eps_out) & 15) == 0;
  if (!vec) {
    const int grid1 = (int)std::min<int64_t>((n + 255) / 256, 2048);
    if (pred_x0) hipLaunchKernelGGL(k_solver_step_1<true>, dim3(grid1), dim3(256), 0, s, x_t, net, x_prev, hist, eps_out, coef_dev, c1_dev, clip, n, step_ptr);
    else hipLaunchKernelGGL(k_solver_step_1<false>, dim3(grid1), dim3(256), 0, s, x_t, net, x_prev, hist, eps_out, coef_dev, c1_dev, clip, n, step_ptr);
    DQ_LAUNCH_CHECK();
    return 0;
  }
  const int grid = (int)std::min<int64_t>((n / 4 + 255) / 256, 2048);
  if (pred_x0) hipLaunchKernelGGL(k_solver_step<true>, dim3(grid), dim3(256), 0, s, x_t, net, x_prev, hist, eps_out, coef_dev, c1_dev, clip, n / 4, step_ptr);
  else hipLaunchKernelGGL(k_solver_step<false>, dim3(grid), dim3(256), 0, s, x_t, net, x_prev, hist, eps_out, coef_dev, c1_dev, clip, n / 4, step_ptr);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
