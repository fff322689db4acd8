// What the P predictions of a group do together (dq_group_metrics): the held-out counterpart of k_group.hip's
// projection.  pred, target (P * G, RT, MZ) fp32, member-major (member p of group g is row p * G + g); mix (G, RT, MZ), the caller's image
// units throughout.  Per group, every sum in fp64 over the fp32 inputs (n = RT * MZ elements), every output rounded to fp32 once:
//   cross[g, p, q] = sum pred_p target_q / sqrt(sum pred_p^2 * sum target_q^2), 0 if either norm is 0      (G, P, P)
//   group[g]       = (excess, unexplained, mix_total): with S = ((max(pred_0, 0) + max(pred_1, 0)) + ...) and m+ = max(mix, 0) per element,
//                    sum max(S - m+, 0) / sum m+,  sum max(m+ - S, 0) / sum m+,  sum m+; the two ratios are 0 when sum m+ == 0     (G, 3)
// Two launches:
//   k_group_metric_part<P, V>  one block per (group, role, chunk of GROUP_METRIC_CHUNK elements).  Role p < P holds ONE prediction against all
//                              P targets: sum pred_p^2, sum target_p^2 and the P inner products, P + 2 fp64 accumulators per lane, so nothing
//                              leaves the registers; role P holds the P predictions against the mixture: three accumulators.  Lane t of the
//                              block takes the elements 4 (t + 256 i) .. + 3 of its chunk, as one 16-byte access (V = 4: RT * MZ % 4 == 0 and
//                              every tensor 16-byte aligned) or as four 4-byte ones (V = 1): the same elements in the same order either way, so
//                              the two forms give the same bits.  Lanes combine by the butterfly, waves in index order -> one slot of scratch.
//   k_group_metric_finish      one block per group: a lane folds one quantity's chunks in index order; then the ratios.
// No atomics; the partition depends on (RT, MZ, P) only, so a group's rows are bit for bit the same in any batch and on every repeat.
// Algorithmic bytes per group: P predictions, P targets and the mixture once, (2 P + 1) n 4 B; role p reads the P targets again ((P + 1)^2
// + P windows through L2 in all).
#include "dq_common.h"
#include "dq_kernels.h"
#include "dq_launch.h"
#include "../../include/dq_hip.h"
#include <cmath>
#include <string>

namespace dq {

constexpr int GROUP_METRIC_CHUNK = 4096;  // elements of a window per block: four passes of 256 lanes x 4 elements
constexpr int GROUP_METRIC_MAX_P = 8;

template <int V> __device__ __forceinline__ void gm_load(const float* __restrict__ p, int64_t e, int64_t end, float (&a)[4]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + e);
    a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = e + j < end ? p[e + j] : 0.f;  // (a zero adds nothing to any of the sums)
  }
}

__device__ __forceinline__ double gm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// slot layout: part[((g * (P + 1) + role) * nchunk + chunk) * (P + 2) + k]
//   role p < P: k = 0 sum pred_p^2, k = 1 sum target_p^2, k = 2 + q sum pred_p target_q;   role P: k = 0 excess, 1 unexplained, 2 sum m+
template <int P, int V>
__global__ void __launch_bounds__(256) k_group_metric_part(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const float* __restrict__ mix, double* __restrict__ part, int G, int64_t per,
                                                           int nchunk) {
  constexpr int NA = P + 2;
  const int64_t item = blockIdx.x;  // (group, role, chunk), chunk fastest
  const int chunk = (int)(item % nchunk);
  const int role = (int)((item / nchunk) % (P + 1));
  const int64_t g = item / ((int64_t)nchunk * (P + 1));
  const int64_t e0 = (int64_t)chunk * GROUP_METRIC_CHUNK;
  const int64_t e1 = e0 + GROUP_METRIC_CHUNK < per ? e0 + GROUP_METRIC_CHUNK : per;
  const int64_t member = (int64_t)G * per;  // the elements between two members of a group
  double acc[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) acc[k] = 0.0;
  if (role < P) {
    const float* __restrict__ pr = pred + role * member + g * per;
    const float* __restrict__ tg = target + g * per;
    for (int64_t e = e0 + 4 * (int64_t)threadIdx.x; e < e1; e += 1024) {
      float a[4], t[P][4];
      gm_load<V>(pr, e, e1, a);
#pragma unroll
      for (int q = 0; q < P; ++q) gm_load<V>(tg + q * member, e, e1, t[q]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double pv = (double)a[j];
        acc[0] += pv * pv;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const double tv = (double)t[q][j];
          acc[2 + q] += pv * tv;
          if (q == role) acc[1] += tv * tv;  // (role is uniform over the block)
        }
      }
    }
  } else {
    const float* __restrict__ pr = pred + g * per;
    const float* __restrict__ mx = mix + g * per;
    for (int64_t e = e0 + 4 * (int64_t)threadIdx.x; e < e1; e += 1024) {
      float a[P][4], m[4];
#pragma unroll
      for (int p = 0; p < P; ++p) gm_load<V>(pr + p * member, e, e1, a[p]);
      gm_load<V>(mx, e, e1, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double S = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) S += a[p][j] > 0.f ? (double)a[p][j] : 0.0;
        const double mp = m[j] > 0.f ? (double)m[j] : 0.0;
        const double d = S - mp;
        acc[0] += d > 0.0 ? d : 0.0;
        acc[1] += d < 0.0 ? -d : 0.0;
        acc[2] += mp;
      }
    }
  }
  __shared__ double red[4][NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) acc[k] = gm_wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NA; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < NA) part[item * NA + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one block of 128 lanes per group: lane t < (P + 1) (P + 2) folds the chunks of quantity (role, k) = (t / (P + 2), t % (P + 2)) in index order
__global__ void __launch_bounds__(128) k_group_metric_finish(const double* __restrict__ part, float* __restrict__ cross,
                                                             float* __restrict__ group, int P, int nchunk) {
  __shared__ double tot[(GROUP_METRIC_MAX_P + 1) * (GROUP_METRIC_MAX_P + 2)];
  const int64_t g = blockIdx.x;
  const int NA = P + 2, t = threadIdx.x;
  if (t < (P + 1) * NA) {
    const double* __restrict__ src = part + (g * (P + 1) + t / NA) * (int64_t)nchunk * NA + t % NA;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += src[(int64_t)c * NA];
    tot[t] = s;
  }
  __syncthreads();
  if (t < P * P) {
    const int p = t / P, q = t % P;
    const double pp = tot[p * NA], tt = tot[q * NA + 1], pt = tot[p * NA + 2 + q];
    cross[g * P * P + t] = (float)(pp > 0.0 && tt > 0.0 ? pt / sqrt(pp * tt) : 0.0);
  }
  if (t == 0) {
    const double ex = tot[P * NA], un = tot[P * NA + 1], mt = tot[P * NA + 2];
    group[g * 3 + 0] = (float)(mt > 0.0 ? ex / mt : 0.0);
    group[g * 3 + 1] = (float)(mt > 0.0 ? un / mt : 0.0);
    group[g * 3 + 2] = (float)mt;
  }
}

// what is built (dq_launch.h): key (P, V)
using GroupMetricFn = void (*)(const float*, const float*, const float*, double*, int, int64_t, int);
static const Inst<GroupMetricFn, 2> GROUP_METRIC_BUILT[] = {
    DQ_INST(k_group_metric_part, 1, 4), DQ_INST(k_group_metric_part, 2, 4), DQ_INST(k_group_metric_part, 3, 4), DQ_INST(k_group_metric_part, 4, 4),
    DQ_INST(k_group_metric_part, 5, 4), DQ_INST(k_group_metric_part, 6, 4), DQ_INST(k_group_metric_part, 7, 4), DQ_INST(k_group_metric_part, 8, 4),
    DQ_INST(k_group_metric_part, 1, 1), DQ_INST(k_group_metric_part, 2, 1), DQ_INST(k_group_metric_part, 3, 1), DQ_INST(k_group_metric_part, 4, 1),
    DQ_INST(k_group_metric_part, 5, 1), DQ_INST(k_group_metric_part, 6, 1), DQ_INST(k_group_metric_part, 7, 1), DQ_INST(k_group_metric_part, 8, 1),
};

static int64_t group_metric_nchunk(int RT, int MZ) { return ((int64_t)RT * MZ + GROUP_METRIC_CHUNK - 1) / GROUP_METRIC_CHUNK; }

}  // namespace dq

extern "C" {

int64_t dq_group_metrics_scratch_bytes(int G, int P, int RT, int MZ) {
  if (G < 1 || P < 1 || P > dq::GROUP_METRIC_MAX_P || RT < 1 || MZ < 1) return -1;
  return (int64_t)sizeof(double) * G * (P + 1) * dq::group_metric_nchunk(RT, MZ) * (P + 2);
}

int dq_group_metrics(const float* pred, const float* target, const float* mix, float* cross, float* group, void* scratch,
                     int64_t scratch_bytes, int G, int P, int RT, int MZ, void* stream) {
  using namespace dq;
  const std::string who = "dq_group_metrics";
  DQ_REQUIRE(pred && target && mix && cross && group && scratch, who + ": null argument");
  DQ_REQUIRE(P >= 1 && P <= GROUP_METRIC_MAX_P, who + ": group_size must be 1..8");
  DQ_REQUIRE(G > 0 && RT > 0 && MZ > 0, who + ": G, RT and MZ must be positive");
  DQ_REQUIRE(scratch_bytes >= dq_group_metrics_scratch_bytes(G, P, RT, MZ), who + ": scratch too small (dq_group_metrics_scratch_bytes)");
  const uintptr_t bits = (uintptr_t)pred | (uintptr_t)target | (uintptr_t)mix;
  DQ_REQUIRE((bits & 3) == 0 && (((uintptr_t)cross | (uintptr_t)group) & 3) == 0 && ((uintptr_t)scratch & 7) == 0,
             who + ": tensors must be 4-byte aligned (scratch 8-byte)");
  const int64_t per = (int64_t)RT * MZ, nchunk = group_metric_nchunk(RT, MZ);
  const int64_t items = (int64_t)G * (P + 1) * nchunk;
  DQ_REQUIRE(items <= INT32_MAX && nchunk <= INT32_MAX, who + ": too many work items for one launch");
  // 16 bytes per access iff every window starts on a 16-byte boundary
  const int key[2] = {P, per % 4 == 0 && (bits & 15) == 0 ? 4 : 1};
  const auto* row = find_inst(GROUP_METRIC_BUILT, key);
  DQ_REQUIRE(row, who + ": no kernel for this group size");
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)scratch;
  hipLaunchKernelGGL(row->fn, dim3((unsigned)items), dim3(256), 0, s, pred, target, mix, part, G, per, (int)nchunk);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_group_metric_finish, dim3(G), dim3(128), 0, s, (const double*)part, cross, group, P, (int)nchunk);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
