// Deconvolving a whole chromatogram: one observed run (RT_total, MZ) with its MS1 trace (RT_total, M1), resident in
// HBM, is cut into overlapping windows of W scans every `step` scans, each window normalised by its own statistics, sampled, and the
// predictions brought back to one intensity scale and blended where windows overlap.
//   window rule   n = ceil((RT_total - W) / step) + 1 windows, 1 <= step <= W <= RT_total; window i starts at s_i = min(i step, RT_total - W)
//                 (the last one is pulled back to end on the last scan).  Both kernels recompute s_i from (i0, b, W, step, RT_total): no
//                 index array exists, so there is no index to check on the device.
//   dq_run_windows  n = (x - lo) / (hi - lo) in fp32, k_pairs.hip's expression; MS2 lo / hi over the window's own W MZ values, MS1 lo / hi
//                 over its W M1 values.  Unlike the pair form a constant window (hi == lo: an empty stretch of a run) gives zeros, not NaN;
//                 its `scale` row still records lo == hi.  Inputs are assumed finite: fminf / fmaxf return the other operand for a NaN, so a
//                 NaN scan does not enter lo / hi and comes out as NaN, and an infinity makes the range infinite (finite values become 0,
//                 the infinity itself NaN).
//   dq_run_stitch   West's weighted running mean and variance per output element (r, m), over the batch's windows that cover r in ascending i:
//                   v = pred[i, r - s_i, m] * (hi_i - lo_i);  w = taper[r - s_i];  wn = wsum + w;  d = v - mean;
//                   mean = mean + (w / wn) * d;  m2 = m2 + (w * d) * (v - mean);  wsum = wn
//                 every operation rounded on its own (no FMA contraction, correctly rounded division).  The update is sequential in window
//                 order, so windows fed in ascending order give the same bits in any grouping into calls.
// Two launches for the windows, like the pair form: (1) k_run_minmax, grid (RUN_CHUNKS, B): each block reduces its chunk of the window to a
// partial (min, max); block 0 also reduces the window's MS1.  (2) k_run_norm, grid (blocks per window, B): folds the RUN_CHUNKS partials in
// fixed order (wave-uniform, once per block), normalises and writes; its first lane writes the window's `scale` row.  A window is W MZ
// contiguous floats of the run starting at s_i MZ: float4 when MZ % 4 == 0 (every start is then 16-byte aligned), scalar otherwise.
// One launch for the stitch: a block owns ONE scan r -- wsum[r] is read by every thread of the block, then (after a barrier) written once by
// its first lane, so no block reads a value another block writes.  No atomics, no LDS beyond the block reduce, no transcendental (the taper
// is a host table).
// HBM-bound; algorithmic bytes per window: windows read W MZ 4 B (the second read comes from L2 / Infinity Cache) and write W MZ 4 B (+ MS1);
// the stitch reads W MZ 4 B of predictions and reads and writes mean and m2 of the scans it covers (2 * 2 * step MZ 4 B per window at overlap
// W / step, each scan's state being touched once per call, not once per covering window).
#include "dq_common.h"
#include "dq_kernels.h"
#include "../../include/dq_hip.h"
#include <algorithm>

namespace dq {

constexpr int RUN_CHUNKS = 8;
constexpr int RUN_MAX_BLOCKS_X = 64;  // blocks of k_run_norm per window; a longer window is walked with this stride

__device__ __forceinline__ float run_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float run_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float run_min(float a) { return a; }
__device__ __forceinline__ float run_max(float a) { return a; }
__device__ __forceinline__ float run_min(float4 a) { return fminf(fminf(a.x, a.y), fminf(a.z, a.w)); }
__device__ __forceinline__ float run_max(float4 a) { return fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)); }
// (x - lo) / rng, or 0 for a constant window (rng == 0)
__device__ __forceinline__ float run_norm(float v, float lo, float rng) { return rng == 0.0f ? 0.0f : (v - lo) / rng; }
__device__ __forceinline__ float4 run_norm(float4 v, float lo, float rng) {
  return make_float4(run_norm(v.x, lo, rng), run_norm(v.y, lo, rng), run_norm(v.z, lo, rng), run_norm(v.w, lo, rng));
}

// the first scan of window i; last = RT_total - W
__host__ __device__ __forceinline__ int64_t run_start(int64_t i, int step, int64_t last) {
  const int64_t s = i * step;
  return s < last ? s : last;
}

// the block's (min, max) of (mn, mx) to p[0], p[1] by its first lane; red is the block's 2 x 4 floats
__device__ __forceinline__ void run_block_minmax(float mn, float mx, float (*red)[4], float* p) {
  mn = run_wave_min(mn); mx = run_wave_max(mx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    p[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

// T = float4 (MZ % 4 == 0) or float.  per: the window's MS2 length in T; per1 = W * M1.  part: B * (RUN_CHUNKS + 1) * 2 floats ((min, max)
// per chunk, last slot = MS1).
template <class T>
__global__ void __launch_bounds__(256) k_run_minmax(const float* __restrict__ ms2, const float* __restrict__ ms1, int64_t row, int M1, int W,
                                                    int step, int64_t last, int64_t i0, int64_t per, int64_t per1, float* __restrict__ part) {
  const int b = blockIdx.y, c = blockIdx.x;
  const int64_t s = run_start(i0 + b, step, last);
  const T* w = reinterpret_cast<const T*>(ms2 + s * row);
  const int64_t lo_i = per * c / RUN_CHUNKS, hi_i = per * (c + 1) / RUN_CHUNKS;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = lo_i + threadIdx.x; i < hi_i; i += blockDim.x) {
    const T a = w[i];
    mn = fminf(run_min(a), mn); mx = fmaxf(run_max(a), mx);
  }
  __shared__ float red[2][4];
  run_block_minmax(mn, mx, red, part + ((int64_t)b * (RUN_CHUNKS + 1) + c) * 2);
  if (c != 0) return;
  __syncthreads();
  const float* m = ms1 + s * M1;
  mn = INFINITY; mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < per1; i += blockDim.x) { mn = fminf(mn, m[i]); mx = fmaxf(mx, m[i]); }
  run_block_minmax(mn, mx, red, part + ((int64_t)b * (RUN_CHUNKS + 1) + RUN_CHUNKS) * 2);
}

template <class T>
__global__ void __launch_bounds__(256) k_run_norm(const float* __restrict__ ms2, const float* __restrict__ ms1, int64_t row, int M1, int W,
                                                  int step, int64_t last, int64_t i0, int64_t per, int64_t per1,
                                                  const float* __restrict__ part, float* __restrict__ o_ms2, float* __restrict__ o_ms1,
                                                  float* __restrict__ o_scale) {
  const int b = blockIdx.y;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t s = run_start(i0 + b, step, last);
  const float* pp = part + (int64_t)b * (RUN_CHUNKS + 1) * 2;
  float lo = pp[0], hi = pp[1];
#pragma unroll
  for (int c = 1; c < RUN_CHUNKS; ++c) { lo = fminf(lo, pp[2 * c]); hi = fmaxf(hi, pp[2 * c + 1]); }
  const float lo1 = pp[2 * RUN_CHUNKS], hi1 = pp[2 * RUN_CHUNKS + 1];
  if (first == 0) {
    float* sc = o_scale + (int64_t)b * 4;
    sc[0] = lo; sc[1] = hi; sc[2] = lo1; sc[3] = hi1;
  }
  {
    const float rng1 = hi1 - lo1;
    const float* src = ms1 + s * M1;
    float* dst = o_ms1 + (int64_t)b * per1;
    for (int64_t e = first; e < per1; e += stride) dst[e] = run_norm(src[e], lo1, rng1);
  }
  const float rng = hi - lo;
  const T* src = reinterpret_cast<const T*>(ms2 + s * row);
  T* dst = reinterpret_cast<T*>(o_ms2) + (int64_t)b * per;
  for (int64_t e = first; e < per; e += stride) dst[e] = run_norm(src[e], lo, rng);
}

__device__ __forceinline__ float run_ld(const float* p, int64_t i, float) { return p[i]; }
__device__ __forceinline__ float4 run_ld(const float* p, int64_t i, float4) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ void run_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void run_st(float* p, int64_t i, float4 v) { reinterpret_cast<float4*>(p)[i] = v; }

// one step of West's update for one element; f = w / wn is the scan's, formed once
__device__ __forceinline__ void run_fold(float p, float rng, float w, float f, float& mean, float& m2) {
  const float v = p * rng;
  const float d = v - mean;
  mean = mean + f * d;
  m2 = m2 + (w * d) * (v - mean);
}
__device__ __forceinline__ void run_fold(float4 p, float rng, float w, float f, float4& mean, float4& m2) {
  run_fold(p.x, rng, w, f, mean.x, m2.x);
  run_fold(p.y, rng, w, f, mean.y, m2.y);
  run_fold(p.z, rng, w, f, mean.z, m2.z);
  run_fold(p.w, rng, w, f, mean.w, m2.w);
}

// grid: one block per scan of [r0, r0 + gridDim.x), the scans windows i0 .. i0 + B - 1 cover (consecutive windows abut or overlap, step <= W:
// every scan in between is covered).  rowT: MZ in T.  The windows of the batch that cover scan r: s_i <= i step, so i >= ilo = the first i
// with i step > r - W; from there while s_i <= r.  All of that is the block's, i.e. wave-uniform.
template <class T>
__global__ void __launch_bounds__(256) k_run_stitch(const float* __restrict__ pred, const float* __restrict__ scale,
                                                    const float* __restrict__ taper, int64_t r0, int rowT, int W, int step, int64_t last,
                                                    int64_t i0, int B, float* __restrict__ mean, float* __restrict__ m2,
                                                    float* __restrict__ wsum) {
  const int64_t r = r0 + blockIdx.x;
  const int64_t ilo = r >= W ? (r - W) / step + 1 : 0;
  const int64_t ibeg = ilo > i0 ? ilo : i0, iend = i0 + B;
  const float ws0 = wsum[r];
  __syncthreads();  // every thread of the scan has read wsum[r] before the first lane writes it below
  float ws = ws0;
  for (int m = threadIdx.x; m < rowT; m += blockDim.x) {
    T mu = run_ld(mean, r * rowT + m, T{}), q = run_ld(m2, r * rowT + m, T{});
    ws = ws0;
    for (int64_t i = ibeg; i < iend; ++i) {
      const int64_t s = run_start(i, step, last);
      if (s > r) break;
      const int b = (int)(i - i0), k = (int)(r - s);
      const float rng = scale[4 * b + 1] - scale[4 * b], w = taper[k];
      const float wn = ws + w;
      run_fold(run_ld(pred, ((int64_t)b * W + k) * rowT + m, T{}), rng, w, w / wn, mu, q);
      ws = wn;
    }
    run_st(mean, r * rowT + m, mu);
    run_st(m2, r * rowT + m, q);
  }
  if (threadIdx.x == 0) {  // (the first lane always has an element: rowT >= 1)
    wsum[r] = ws;
  }
}

}  // namespace dq

extern "C" {

int64_t dq_run_window_count(int RT_total, int W, int step) {
  if (!(1 <= step && step <= W && W <= RT_total)) return 0;
  return ((int64_t)RT_total - W + step - 1) / step + 1;
}

int64_t dq_run_windows_scratch_bytes(int B) {
  return (B <= 0 || B > 65535) ? 0 : (int64_t)B * (dq::RUN_CHUNKS + 1) * 2 * (int64_t)sizeof(float);
}

int dq_run_windows(const float* ms2_run, const float* ms1_run, int RT_total, int MZ, int M1, int W, int step, int64_t i0, int B,
                   float* ms2_win, float* ms1_win, float* scale, void* scratch, int64_t scratch_bytes, void* stream) {
  using namespace dq;
  DQ_REQUIRE(ms2_run && ms1_run && ms2_win && ms1_win && scale && scratch, "dq_run_windows: null argument");
  DQ_REQUIRE(MZ >= 1 && M1 >= 1, "dq_run_windows: MZ and M1 must be >= 1");
  DQ_REQUIRE(1 <= step && step <= W && W <= RT_total, "dq_run_windows: need 1 <= step <= W <= RT_total");
  const int64_t n = dq_run_window_count(RT_total, W, step);
  DQ_REQUIRE(i0 >= 0 && B >= 1 && B <= n && i0 <= n - B,  // (i0 + B <= n without forming a sum that can overflow)
             "dq_run_windows: windows i0 .. i0 + B - 1 must lie in 0 .. n - 1 (dq_run_window_count)");
  DQ_REQUIRE(B <= 65535, "dq_run_windows: at most 65535 windows per call");
  DQ_REQUIRE(scratch_bytes >= dq_run_windows_scratch_bytes(B), "dq_run_windows: scratch too small (dq_run_windows_scratch_bytes)");
  hipStream_t s = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(scratch);
  const int64_t last = (int64_t)RT_total - W, per = (int64_t)W * MZ, per1 = (int64_t)W * M1;
  if (MZ % 4 == 0) {
    hipLaunchKernelGGL(k_run_minmax<float4>, dim3(RUN_CHUNKS, B), dim3(256), 0, s, ms2_run, ms1_run, (int64_t)MZ, M1, W, step, last, i0,
                       per / 4, per1, part);
    DQ_LAUNCH_CHECK();
    const int gx = (int)std::min<int64_t>(cdiv(std::max(per / 4, per1), 256), RUN_MAX_BLOCKS_X);
    hipLaunchKernelGGL(k_run_norm<float4>, dim3(gx, B), dim3(256), 0, s, ms2_run, ms1_run, (int64_t)MZ, M1, W, step, last, i0, per / 4,
                       per1, part, ms2_win, ms1_win, scale);
    DQ_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(k_run_minmax<float>, dim3(RUN_CHUNKS, B), dim3(256), 0, s, ms2_run, ms1_run, (int64_t)MZ, M1, W, step, last, i0, per,
                       per1, part);
    DQ_LAUNCH_CHECK();
    const int gx = (int)std::min<int64_t>(cdiv(std::max(per, per1), 256), RUN_MAX_BLOCKS_X);
    hipLaunchKernelGGL(k_run_norm<float>, dim3(gx, B), dim3(256), 0, s, ms2_run, ms1_run, (int64_t)MZ, M1, W, step, last, i0, per, per1,
                       part, ms2_win, ms1_win, scale);
    DQ_LAUNCH_CHECK();
  }
  return 0;
}

int dq_run_stitch(const float* pred, const float* scale, const float* taper, int RT_total, int MZ, int W, int step, int64_t i0, int B,
                  float* mean, float* m2, float* wsum, void* stream) {
  using namespace dq;
  DQ_REQUIRE(pred && scale && taper && mean && m2 && wsum, "dq_run_stitch: null argument");
  DQ_REQUIRE(MZ >= 1, "dq_run_stitch: MZ must be >= 1");
  DQ_REQUIRE(1 <= step && step <= W && W <= RT_total, "dq_run_stitch: need 1 <= step <= W <= RT_total");
  const int64_t n = dq_run_window_count(RT_total, W, step);
  DQ_REQUIRE(i0 >= 0 && B >= 1 && B <= n && i0 <= n - B,  // (i0 + B <= n without forming a sum that can overflow)
             "dq_run_stitch: windows i0 .. i0 + B - 1 must lie in 0 .. n - 1 (dq_run_window_count)");
  DQ_REQUIRE(B <= 65535, "dq_run_stitch: at most 65535 windows per call");
  hipStream_t s = (hipStream_t)stream;
  const int64_t last = (int64_t)RT_total - W;
  const int64_t r0 = run_start(i0, step, last), r1 = run_start(i0 + B - 1, step, last) + W;  // r1 <= RT_total
  const int rows = (int)(r1 - r0);
  const int rowT = MZ % 4 == 0 ? MZ / 4 : MZ;
  const int threads = std::min(256, 64 * cdiv(rowT, 64));
  if (MZ % 4 == 0)
    hipLaunchKernelGGL(k_run_stitch<float4>, dim3(rows), dim3(threads), 0, s, pred, scale, taper, r0, rowT, W, step, last, i0, B, mean, m2,
                       wsum);
  else
    hipLaunchKernelGGL(k_run_stitch<float>, dim3(rows), dim3(threads), 0, s, pred, scale, taper, r0, rowT, W, step, last, i0, B, mean, m2,
                       wsum);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
