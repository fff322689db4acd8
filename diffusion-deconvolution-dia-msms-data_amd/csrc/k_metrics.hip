// Reconstruction metrics of a sampled MS2 window against its target (dq_recon_metrics; no reference counterpart: the reference's TODOS
// list "eval metrics ... separate from training").  pred, target (B, RT, MZ) fp32 -> out (B, METRIC_COUNT) fp32, per window:
//   mse, mae, cosine, sa (spectral angle), pearson over all n = RT * MZ elements; scan_sa / scan_count: mean spectral angle over the
//   scans (RT rows) whose target row is not all zero; xic_r / xic_count: mean Pearson r along RT over the XICs (m/z columns) whose
//   target column is not constant.  Definitions: include/dq_hip.h, DESIGN.md section 24.
// Every sum is taken in fp64 over the fp32 inputs and every output is rounded to fp32 once.  Three launches:
//   k_metric_rows   one wave per (window, scan, segment of METRIC_ROW_SEG m/z columns), lanes along m/z (coalesced): ten moments per item
//                   -> scratch.  Five are raw (sum P^2, T^2, P T, (P - T)^2, |P - T|), five are taken on p' = P - P[b,0,0], t' = T - T[b,0,0]
//                   (sum p', t', p'^2, t'^2, p' t'): a shift common to the window keeps plain sums mergeable and makes a constant window's
//                   variance exactly 0.
//   k_metric_cols   one wave per (window, chunk of METRIC_COL_ROWS scans, tile of 64 m/z columns), lane = column (coalesced across
//                   lanes), looping over the chunk's scans: five moments per column on p' = P - P[b,0,c], t' = T - T[b,0,c] -> scratch.
//   k_metric_finish one block per window: the items are added up in a fixed order (a thread takes every 256th scan / column, its items
//                   in index order; the 256 threads combine by the same butterfly + four-wave sum every time).
// No atomics; the partition depends on (RT, MZ) only, so a window's nine numbers do not depend on the batch it is computed in.
// Algorithmic bytes per element: 16 B (P and T are read once by each of the two passes) + the moment slots:
// 80 B / METRIC_ROW_SEG-column row segment and 40 B / (column x scan chunk), each written once and read once.
#include "dq_common.h"
#include "dq_kernels.h"
#include <cmath>

namespace dq {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) k_metric_rows(const float* __restrict__ P, const float* __restrict__ T, double* __restrict__ rowpart,
                                                     int64_t items, int RT, int MZ, int nseg) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (window, scan, segment), segment fastest
  if (item >= items) return;
  const int lane = threadIdx.x & 63;
  const int seg = (int)(item % nseg);
  const int64_t row = item / nseg;  // b * RT + r
  const int64_t b = row / RT;
  const int64_t per = (int64_t)RT * MZ;
  const double p0 = (double)P[b * per], t0 = (double)T[b * per];
  const float* __restrict__ pr = P + row * MZ;
  const float* __restrict__ tr = T + row * MZ;
  const int c1 = min(MZ, (seg + 1) * METRIC_ROW_SEG);
  double a[METRIC_ROW_MOMENTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = seg * METRIC_ROW_SEG + lane; c < c1; c += 64) {
    const double p = (double)pr[c], t = (double)tr[c];
    const double d = p - t, ps = p - p0, ts = t - t0;
    a[0] += p * p; a[1] += t * t; a[2] += p * t; a[3] += d * d; a[4] += fabs(d);
    a[5] += ps; a[6] += ts; a[7] += ps * ps; a[8] += ts * ts; a[9] += ps * ts;
  }
#pragma unroll
  for (int k = 0; k < METRIC_ROW_MOMENTS; ++k) a[k] = wave_sum_d(a[k]);
  if (lane < METRIC_ROW_MOMENTS) {
    double v = a[0];
#pragma unroll
    for (int k = 1; k < METRIC_ROW_MOMENTS; ++k) v = lane == k ? a[k] : v;
    rowpart[item * METRIC_ROW_MOMENTS + lane] = v;
  }
}

__global__ void __launch_bounds__(256) k_metric_cols(const float* __restrict__ P, const float* __restrict__ T, double* __restrict__ colpart,
                                                     int64_t items, int RT, int MZ, int nchunk, int ntile) {
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (window, scan chunk, column tile), tile fastest
  if (item >= items) return;
  const int c = (int)(item % ntile) * 64 + (threadIdx.x & 63);
  if (c >= MZ) return;
  const int chunk = (int)((item / ntile) % nchunk);
  const int64_t b = item / ((int64_t)ntile * nchunk);
  const float* __restrict__ pc = P + b * (int64_t)RT * MZ + c;
  const float* __restrict__ tc = T + b * (int64_t)RT * MZ + c;
  const double p0 = (double)pc[0], t0 = (double)tc[0];  // the column's value in scan 0: the shift of every chunk of this column
  const int r1 = min(RT, (chunk + 1) * METRIC_COL_ROWS);
  double sp = 0, st = 0, spp = 0, stt = 0, spt = 0;
#pragma unroll 4
  for (int r = chunk * METRIC_COL_ROWS; r < r1; ++r) {
    const double ps = (double)pc[(int64_t)r * MZ] - p0, ts = (double)tc[(int64_t)r * MZ] - t0;
    sp += ps; st += ts; spp += ps * ps; stt += ts * ts; spt += ps * ts;
  }
  double* o = colpart + ((b * nchunk + chunk) * METRIC_COL_MOMENTS) * MZ + c;  // (window, chunk, moment, column): column contiguous
  o[0] = sp; o[MZ] = st; o[2 * (int64_t)MZ] = spp; o[3 * (int64_t)MZ] = stt; o[4 * (int64_t)MZ] = spt;
}

// sum over the 256 threads, every thread receives it; `red` 4 doubles of LDS
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// 1 - 2 acos(clamp(cos)) / pi of the vectors with squared norms pp, tt and inner product pt; 0 when a norm is 0
__device__ __forceinline__ double cosine_d(double pp, double tt, double pt) { return pp > 0.0 && tt > 0.0 ? pt / sqrt(pp * tt) : 0.0; }
__device__ __forceinline__ double spectral_angle_d(double cosv) {
  return 1.0 - 2.0 * acos(fmin(1.0, fmax(-1.0, cosv))) / 3.14159265358979323846;
}
// Pearson r from sums of shifted values over m elements; *valid_t: the target's variance is positive
__device__ __forceinline__ double pearson_d(double sp, double st, double spp, double stt, double spt, double m, bool* valid_t) {
  const double vp = spp - sp * sp / m, vt = stt - st * st / m, cv = spt - sp * st / m;
  *valid_t = vt > 0.0;
  return vp > 0.0 && vt > 0.0 ? cv / sqrt(vp * vt) : 0.0;
}

__global__ void __launch_bounds__(256) k_metric_finish(const double* __restrict__ rowpart, const double* __restrict__ colpart,
                                                       float* __restrict__ out, int RT, int MZ, int nseg, int nchunk) {
  __shared__ double red[4];
  const int64_t b = blockIdx.x;
  const double* __restrict__ rp = rowpart + b * RT * nseg * METRIC_ROW_MOMENTS;
  const double* __restrict__ cp = colpart + b * nchunk * METRIC_COL_MOMENTS * MZ;
  double a[METRIC_ROW_MOMENTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double sa_sum = 0, sa_cnt = 0;
  for (int r = threadIdx.x; r < RT; r += 256) {
    double s[METRIC_ROW_MOMENTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < nseg; ++g)
#pragma unroll
      for (int k = 0; k < METRIC_ROW_MOMENTS; ++k) s[k] += rp[((int64_t)r * nseg + g) * METRIC_ROW_MOMENTS + k];
#pragma unroll
    for (int k = 0; k < METRIC_ROW_MOMENTS; ++k) a[k] += s[k];
    if (s[1] > 0.0) {  // a valid scan: its target row is not all zero
      sa_cnt += 1.0;
      if (s[0] > 0.0) sa_sum += spectral_angle_d(cosine_d(s[0], s[1], s[2]));
    }
  }
  double xr_sum = 0, xr_cnt = 0;
  for (int c = threadIdx.x; c < MZ; c += 256) {
    double s[METRIC_COL_MOMENTS] = {0, 0, 0, 0, 0};
    for (int h = 0; h < nchunk; ++h)
#pragma unroll
      for (int k = 0; k < METRIC_COL_MOMENTS; ++k) s[k] += cp[((int64_t)h * METRIC_COL_MOMENTS + k) * MZ + c];
    bool valid;
    const double r = pearson_d(s[0], s[1], s[2], s[3], s[4], (double)RT, &valid);
    if (valid) { xr_cnt += 1.0; xr_sum += fmin(1.0, fmax(-1.0, r)); }
  }
#pragma unroll
  for (int k = 0; k < METRIC_ROW_MOMENTS; ++k) a[k] = block_sum_d(a[k], red);
  sa_sum = block_sum_d(sa_sum, red); sa_cnt = block_sum_d(sa_cnt, red);
  xr_sum = block_sum_d(xr_sum, red); xr_cnt = block_sum_d(xr_cnt, red);
  if (threadIdx.x == 0) {
    const double n = (double)RT * (double)MZ;
    const double cosv = cosine_d(a[0], a[1], a[2]);
    bool valid;
    const double r = pearson_d(a[5], a[6], a[7], a[8], a[9], n, &valid);
    float* o = out + b * METRIC_COUNT;
    o[0] = (float)(a[3] / n);
    o[1] = (float)(a[4] / n);
    o[2] = (float)cosv;
    o[3] = (float)spectral_angle_d(cosv);
    o[4] = (float)fmin(1.0, fmax(-1.0, r));
    o[5] = (float)(sa_cnt > 0.0 ? sa_sum / sa_cnt : 0.0);
    o[6] = (float)sa_cnt;
    o[7] = (float)(xr_cnt > 0.0 ? xr_sum / xr_cnt : 0.0);
    o[8] = (float)xr_cnt;
  }
}

static int metric_nseg(int MZ) { return (MZ + METRIC_ROW_SEG - 1) / METRIC_ROW_SEG; }
static int metric_nchunk(int RT) { return (RT + METRIC_COL_ROWS - 1) / METRIC_COL_ROWS; }

int64_t recon_metrics_scratch_bytes(int B, int RT, int MZ) {
  if (B < 1 || RT < 1 || MZ < 1) return -1;
  const int64_t per_window = (int64_t)RT * metric_nseg(MZ) * METRIC_ROW_MOMENTS + (int64_t)metric_nchunk(RT) * METRIC_COL_MOMENTS * MZ;
  return (int64_t)sizeof(double) * B * per_window;
}

int launch_recon_metrics(const float* pred, const float* target, float* out, void* scratch, int64_t scratch_bytes, int B, int RT, int MZ,
                         hipStream_t s) {
  DQ_REQUIRE(pred && target && out && scratch, "recon_metrics: null argument");
  DQ_REQUIRE(B > 0 && RT > 0 && MZ > 0, "recon_metrics: B, RT and MZ must be positive");
  DQ_REQUIRE(scratch_bytes >= recon_metrics_scratch_bytes(B, RT, MZ), "recon_metrics: scratch too small (dq_recon_metrics_scratch_bytes)");
  DQ_REQUIRE(((uintptr_t)scratch & 7) == 0, "recon_metrics: scratch must be 8-byte aligned");
  const int nseg = metric_nseg(MZ), nchunk = metric_nchunk(RT), ntile = (MZ + 63) / 64;
  const int64_t row_items = (int64_t)B * RT * nseg, col_items = (int64_t)B * nchunk * ntile;
  DQ_REQUIRE((row_items + 3) / 4 <= INT32_MAX && (col_items + 3) / 4 <= INT32_MAX, "recon_metrics: too many work items for one launch");
  double* rowpart = (double*)scratch;
  double* colpart = rowpart + row_items * METRIC_ROW_MOMENTS;
  hipLaunchKernelGGL(k_metric_rows, dim3((unsigned)((row_items + 3) / 4)), dim3(256), 0, s, pred, target, rowpart, row_items, RT, MZ, nseg);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_metric_cols, dim3((unsigned)((col_items + 3) / 4)), dim3(256), 0, s, pred, target, colpart, col_items, RT, MZ, nchunk,
                     ntile);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_metric_finish, dim3(B), dim3(256), 0, s, rowpart, colpart, out, RT, MZ, nseg, nchunk);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
