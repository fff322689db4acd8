// Mixture consistency over the P precursors of an isolation window, sampled as one group: one streaming pass between
// the network forward and the update that redistributes a step's x0 estimates so that the group never explains more than the observed
// mixture (BOUND), or explains exactly the mixture (SUM) -- the proportional soft-mask projection of Wisdom et al. 2019, per step, on the
// clean-signal estimate.  A batch of B = G * P windows is member-major: member p of group g is row p * G + g; the group's mixture m is row g
// of `mix` (the caller's units, the tensor the network reads).  Per element, with the step's row [sa, sb]:
//   x0_p = net_x0<PRED>(sa, sb, x_p, net_p)                       dq_x0.h: the update's own arithmetic
//   y_p  = normalize ? (x0_p + 1) * 0.5f : x0_p                   the image units of mix
//   yp_p = y_p > 0 ? y_p : 0 ;  S = ((yp_0 + yp_1) + yp_2) + ... ;  m = m > 0 ? m : 0
//   BOUND  S > m: f = m / S, z_p = y_p > 0 ? y_p * f : y_p ; else z_p = y_p          (negatives are never touched)
//   SUM    S > 0: f = m / S, z_p = yp_p * f ;                 else z_p = m / P
//   y'_p = strength == 1 ? z_p : y_p + strength * (z_p - y_p)
//   x0'_p = y'_p == y_p ? x0_p : (normalize ? 2 * y'_p - 1 : y'_p)                  (an element that is not moved keeps its bits)
// Every operation is one rounded fp32 operation in this order (the library is built without FMA contraction, division correctly rounded),
// so a numpy fp32 transcription reproduces every bit.  Inputs are assumed finite.
// k_group_project<PRED, P, V>: a grid-stride loop over the G * per / V lane-steps, instantiated per member count (as mix_dispatch is per
// component count) so that the 2 P loads of a lane-step are in flight together and the y_p stay in registers between the sum and the
// scale; under the x0 objective x_t is not read.  V = 4: 16 bytes per lane and access (per % 4 == 0, every tensor 16-byte aligned); V = 1
// otherwise.  With step_ptr the row is the one the device-side step counter names (graph replay, as ddim_row).  x0_out may alias net: a
// lane reads and writes the same addresses, so that pair carries no __restrict__.  No LDS, no atomics.  HBM-bound; algorithmic bytes per
// element of a member: (3 P + 1) / P * 4 (x, net, x0' per member and the mixture once per group).
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_x0.h"
#include "../../include/dq_hip.h"
#include <algorithm>
#include <string>

namespace dq {

template <int V> __device__ __forceinline__ void group_load(const float* p, int64_t i, float (&a)[V]) {
  if constexpr (V == 4) { const float4 t = reinterpret_cast<const float4*>(p)[i]; a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; }
  else a[0] = p[i];
}
template <int V> __device__ __forceinline__ void group_store(float* p, int64_t i, const float (&a)[V]) {
  if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(a[0], a[1], a[2], a[3]);
  else p[i] = a[0];
}

// nv: the lane-steps of one member, G * per / V -- also the distance between two members of a group, in units of V floats
template <int PRED, int P, int V>
__global__ void __launch_bounds__(256) k_group_project(const float* __restrict__ x_t, const float* net, float* x0_out,
                                                       const float* __restrict__ mix, const float* __restrict__ coef,
                                                       const int* __restrict__ step_ptr, int normalize, int mode, float strength, int64_t nv) {
  if (step_ptr) coef += 4 * step_ptr[0];  // graph replay: this step's row of the coefficient table
  const float sa = coef[0], sb = coef[1];
  const bool sum_mode = mode == DQ_CONSIST_SUM, blend = strength != 1.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float x0[P][V], y[P][V], m[V];
#pragma unroll
    for (int p = 0; p < P; ++p) group_load<V>(net, p * nv + i, x0[p]);
    if constexpr (PRED != DQ_PRED_X0) {
      float x[P][V];
#pragma unroll
      for (int p = 0; p < P; ++p) group_load<V>(x_t, p * nv + i, x[p]);
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < V; ++j) x0[p][j] = net_x0<PRED>(sa, sb, x[p][j], x0[p][j]);
    }
    group_load<V>(mix, i, m);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float S = 0.f;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        y[p][j] = normalize ? (x0[p][j] + 1.f) * 0.5f : x0[p][j];
        const float yp = y[p][j] > 0.f ? y[p][j] : 0.f;
        S = p == 0 ? yp : S + yp;
      }
      const float mj = m[j] > 0.f ? m[j] : 0.f;
      const bool scale = sum_mode ? S > 0.f : S > mj;
      const float f = scale ? mj / S : 1.f;  // (uniform over the group's members: one division per element of a group)
      const float even = mj / (float)P;      // SUM with nothing positive to scale
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const float yv = y[p][j], yp = yv > 0.f ? yv : 0.f;
        float z;
        if (sum_mode) z = scale ? yp * f : even;
        else z = (scale && yv > 0.f) ? yv * f : yv;
        const float yn = blend ? yv + strength * (z - yv) : z;
        x0[p][j] = yn == yv ? x0[p][j] : (normalize ? 2.f * yn - 1.f : yn);
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) group_store<V>(x0_out, p * nv + i, x0[p]);
  }
}

template <int PRED, int P>
static int group_launch_as(const GroupProject& a, bool vec, int64_t n, hipStream_t s) {
  const int64_t nv = vec ? n / 4 : n;
  const int grid = (int)std::min<int64_t>(cdiv(nv, 256), 2048);
  const auto kernel = vec ? k_group_project<PRED, P, 4> : k_group_project<PRED, P, 1>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a.x_t, a.net, a.x0_out, a.mix, a.coef, a.step_ptr, a.normalize, a.mode, a.strength, nv);
  DQ_LAUNCH_CHECK();
  return 0;
}

template <int PRED>
static int group_launch_of(const GroupProject& a, bool vec, int64_t n, hipStream_t s) {
  switch (a.P) {
    case 1: return group_launch_as<PRED, 1>(a, vec, n, s);
    case 2: return group_launch_as<PRED, 2>(a, vec, n, s);
    case 3: return group_launch_as<PRED, 3>(a, vec, n, s);
    case 4: return group_launch_as<PRED, 4>(a, vec, n, s);
    case 5: return group_launch_as<PRED, 5>(a, vec, n, s);
    case 6: return group_launch_as<PRED, 6>(a, vec, n, s);
    case 7: return group_launch_as<PRED, 7>(a, vec, n, s);
    case 8: return group_launch_as<PRED, 8>(a, vec, n, s);
    default: return 0;
  }
}

bool group_mode_ok(int mode) { return mode == DQ_CONSIST_BOUND || mode == DQ_CONSIST_SUM; }
bool group_strength_ok(float strength) { return strength > 0.f && strength <= 1.f; }  // (false for NaN)

int launch_group_project(const GroupProject& a, hipStream_t s) {
  const std::string who = "group_project";
  DQ_REQUIRE(a.x_t && a.net && a.x0_out && a.mix && a.coef, who + ": null argument");
  DQ_REQUIRE(a.pred == DQ_PRED_EPS || a.pred == DQ_PRED_X0 || a.pred == DQ_PRED_V, who + ": Unknown pred_type");
  DQ_REQUIRE(a.P >= 1 && a.P <= DQ_GROUP_MAX, who + ": group_size must be 1..8");
  DQ_REQUIRE(a.G >= 0 && a.per >= 0, who + ": negative size");
  DQ_REQUIRE(group_mode_ok(a.mode), who + ": unknown consistency mode");
  DQ_REQUIRE(group_strength_ok(a.strength), who + ": consistency strength must satisfy 0 < strength <= 1");
  const uintptr_t bits = (uintptr_t)a.x_t | (uintptr_t)a.net | (uintptr_t)a.x0_out | (uintptr_t)a.mix;
  DQ_REQUIRE((bits & 3) == 0 && ((uintptr_t)a.coef & 3) == 0, who + ": tensors must be 4-byte aligned");
  const int64_t n = (int64_t)a.G * a.per;  // the elements of one member
  if (n == 0) return 0;
  // 16 bytes per lane iff every member starts on a 16-byte boundary (n % 4 == 0 follows from per % 4 == 0) and every tensor is aligned
  const bool vec = a.per % 4 == 0 && (bits & 15) == 0;
  switch (a.pred) {
    case DQ_PRED_V: return group_launch_of<DQ_PRED_V>(a, vec, n, s);
    case DQ_PRED_X0: return group_launch_of<DQ_PRED_X0>(a, vec, n, s);
    default: return group_launch_of<DQ_PRED_EPS>(a, vec, n, s);
  }
}

}  // namespace dq

extern "C" {

int dq_group_project(const float* x_t, const float* net, float* x0_out, const float* mix, const float* coef_dev, int pred_type,
                     int auto_normalize, int G, int P, int64_t per_window, int mode, float strength, void* stream) {
  using namespace dq;
  // (launch_group_project's refusals under this entry's name, in its order: nothing has touched the device when one is made)
  const std::string who = "dq_group_project";
  DQ_REQUIRE(x_t && net && x0_out && mix && coef_dev, who + ": null argument");
  DQ_REQUIRE(pred_type == DQ_PRED_EPS || pred_type == DQ_PRED_X0 || pred_type == DQ_PRED_V, who + ": Unknown pred_type");
  DQ_REQUIRE(P >= 1 && P <= DQ_GROUP_MAX, who + ": group_size must be 1..8");
  DQ_REQUIRE(G >= 0 && per_window >= 0, who + ": negative size");
  DQ_REQUIRE(group_mode_ok(mode), who + ": unknown consistency mode");
  DQ_REQUIRE(group_strength_ok(strength), who + ": consistency strength must satisfy 0 < strength <= 1");
  DQ_REQUIRE((((uintptr_t)x_t | (uintptr_t)net | (uintptr_t)x0_out | (uintptr_t)mix | (uintptr_t)coef_dev) & 3) == 0,
             who + ": tensors must be 4-byte aligned");
  GroupProject a;
  a.x_t = x_t; a.net = net; a.x0_out = x0_out; a.mix = mix; a.coef = coef_dev;
  a.pred = pred_type; a.normalize = auto_normalize != 0; a.G = G; a.P = P; a.per = per_window; a.mode = mode; a.strength = strength;
  return launch_group_project(a, (hipStream_t)stream);
}

}  // extern "C"
