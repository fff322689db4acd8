// Per-window statistics of one sampling step, between the network forward and the update: the two scalars per
// window that rescaled guidance and dynamic x0 thresholding need, written to a (B, 4) table [m_b, s_b, rho_b, -] the per-window form of
// k_step_update (k_update.hip) reads.  A window of `per` elements is cut into chunks of WS_CHUNK elements, one block each, grid
// (chunks, B): the partition follows `per` alone, so a window's numbers do not depend on the batch it is computed in.
//   k_win_moments         c, u -> fp64 partials per chunk of the window's c and of its fp32 g = guide(c, u, w), shifted by the window's first
//                         element (k_metrics.hip's form: a constant window has variance exactly 0): sum c', c'^2, g', g'^2.
//   k_win_rescale_finish  one wave per window folds the chunks in index order (lane l: chunks l, l + 64, ..; then the butterfly) and writes
//                         m_b = (float)(phi * sqrt(var_c / var_g) + (1 - phi)), 1 when var_g <= 0.
//   k_win_select          one pass of an exact radix select on key = bits(|x0|) (non-negative floats order as unsigned integers), 8 bits per
//                         pass from the top, for the two ranks j and j + 1 at once: at its head every block folds the previous pass's
//                         per-chunk histograms of its window (thread = bin, chunks in index order; the digit by a serial scan) and so knows
//                         the prefixes found so far; then it counts its chunk's keys under them into an LDS histogram (integer LDS atomics:
//                         counts do not depend on the order) and stores it.  While both ranks share a prefix one histogram serves both.
//   k_win_quantile_finish folds the last pass: the keys ARE a_j and a_{j+1}, bit for bit; Q = a_j + (a_{j+1} - a_j) * frac in fp64, each
//                         operation rounded on its own (the library is built with -ffp-contract=off), rounded to fp32 once;
//                         s_b = min(max(Q, f), cap), rho_b = f / s_b.
// x0 is re-formed per element in every select pass from (x, c, u, w, m_b, row) by dq_guide.h / dq_x0.h, the functions the update calls: both
// see the same bits and no n-sized scratch is needed.  No floating-point atomics, no global atomics, no cross-lane operation beyond
// wave_sum_d's butterfly.
// Algorithmic bytes per element: moments 8 (c, u); select 4 passes x (4 plain | 4 x0 objective unguided | 8 eps, v unguided | 12 guided);
// per chunk and pass 2 KiB of histogram written once and read once per block of the window, 32 B of moments.
#include "dq_common.h"
#include "dq_guide.h"
#include "dq_kernels.h"
#include "dq_x0.h"
#include <cmath>
#include <string>

namespace dq {

namespace {

constexpr int WS_BINS = 256;  // 8 bits per radix pass

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) k_win_moments(const float* __restrict__ c, const float* __restrict__ u, float w, double* __restrict__ part,
                                                     int64_t per) {
  __shared__ double red[4][WS_MOMENTS];
  const int64_t b = blockIdx.y;
  const int chunk = blockIdx.x, nch = gridDim.x;
  const float* __restrict__ cb = c + b * per;
  const float* __restrict__ ub = u + b * per;
  const double c0 = (double)cb[0], g0 = (double)guide(cb[0], ub[0], w);  // the window's shift
  const int64_t e0 = (int64_t)chunk * WS_CHUNK, e1 = min(per, e0 + (int64_t)WS_CHUNK);
  double a[WS_MOMENTS] = {0, 0, 0, 0};
#pragma unroll 4
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const float cv = cb[e];
    const float gv = guide(cv, ub[e], w);
    const double cs = (double)cv - c0, gs = (double)gv - g0;
    a[0] += cs; a[1] += cs * cs; a[2] += gs; a[3] += gs * gs;
  }
#pragma unroll
  for (int k = 0; k < WS_MOMENTS; ++k) a[k] = wave_sum_d(a[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < WS_MOMENTS; ++k) red[threadIdx.x >> 6][k] = a[k];
  }
  __syncthreads();
  if (threadIdx.x < WS_MOMENTS) {
    const int k = threadIdx.x;
    part[(b * nch + chunk) * WS_MOMENTS + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// s_init: the clamp of a step without thresholding (+inf: none); init_rest: this launch writes the whole row
__global__ void __launch_bounds__(64) k_win_rescale_finish(const double* __restrict__ part, float* __restrict__ tab, float* __restrict__ m_out,
                                                           double phi, int nch, int64_t per, float s_init, int init_rest) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double a[WS_MOMENTS] = {0, 0, 0, 0};
  for (int ch = lane; ch < nch; ch += 64)
#pragma unroll
    for (int k = 0; k < WS_MOMENTS; ++k) a[k] += part[(b * nch + ch) * WS_MOMENTS + k];
#pragma unroll
  for (int k = 0; k < WS_MOMENTS; ++k) a[k] = wave_sum_d(a[k]);
  if (lane == 0) {
    const double n = (double)per;
    const double vc = fmax(a[1] - a[0] * a[0] / n, 0.0), vg = a[3] - a[2] * a[2] / n;  // (n times the variances: the ratio is what counts)
    float m = 1.f;
    if (vg > 0.0) m = (float)(phi * sqrt(vc / vg) + (1.0 - phi));
    if (m_out) m_out[b] = m;
    if (tab) {
      tab[4 * b] = m;
      if (init_rest) { tab[4 * b + 1] = s_init; tab[4 * b + 2] = 1.f; tab[4 * b + 3] = 0.f; }
    }
  }
}

// Where the keys come from.  prepare(b): the window's scalars; key(idx): bits of |value| of element idx of the whole tensor
struct SrcPlain {
  const float* __restrict__ x;
  __device__ __forceinline__ void prepare(int64_t) {}
  __device__ __forceinline__ uint32_t key(int64_t idx) const { return __float_as_uint(x[idx]) & 0x7fffffffu; }
};
// the step's x0 estimate: g = guide(c, u, w) (GUIDED), times m_b (tab non-null), through the objective with this step's [sa, sb]
template <int PRED, bool GUIDED>
struct SrcX0 {
  const float* x; const float* c; const float* u;  // (x may be the tensor the update then writes: no __restrict__)
  const float* coef; const int* step_ptr; const float* tab;
  float w;
  float sa, sb, m;
  __device__ __forceinline__ void prepare(int64_t b) {
    const float* r = step_ptr ? coef + 4 * step_ptr[0] : coef;  // graph replay: this step's row
    sa = r[0]; sb = r[1];
    m = tab ? tab[4 * b] : 1.f;
  }
  __device__ __forceinline__ uint32_t key(int64_t idx) const {
    float g = c[idx];
    if constexpr (GUIDED) {
      g = guide(g, u[idx], w);
      if (tab) g = m * g;
    }
    const float xv = PRED == DQ_PRED_X0 ? 0.f : x[idx];
    return __float_as_uint(net_x0<PRED>(sa, sb, xv, g)) & 0x7fffffffu;
  }
};

// The fold at the head of a pass (and in the finish): `hist` is the window's nch x (2 * WS_BINS) counts of the pass whose digit sits at
// `shift`; st the state that pass counted under.  Returns the state with that digit appended to both prefixes.  256 threads; uniform result.
__device__ __forceinline__ WinSelState select_fold(const uint32_t* __restrict__ hist, int nch, WinSelState st, int shift, uint32_t* lds,
                                                   WinSelState* res) {
  const int t = threadIdx.x;
  const bool same = st.prefA == st.prefB;
  uint32_t sa = 0, sb = 0;
  for (int ch = 0; ch < nch; ++ch) sa += hist[(int64_t)ch * (2 * WS_BINS) + t];
  if (same) sb = sa;
  else
    for (int ch = 0; ch < nch; ++ch) sb += hist[(int64_t)ch * (2 * WS_BINS) + WS_BINS + t];
  __syncthreads();  // (lds may still be read by the caller's previous use)
  lds[t] = sa; lds[WS_BINS + t] = sb;
  __syncthreads();
  if (t == 0 || t == 64) {  // one lane of wave 0 for rank j, one of wave 1 for rank j + 1
    const uint32_t* h = t == 0 ? lds : lds + WS_BINS;
    const uint32_t rank = t == 0 ? st.rankA : st.rankB;
    uint32_t cum = 0, digit = WS_BINS - 1;
    for (int d = 0; d < WS_BINS; ++d) {
      const uint32_t cnt = h[d];
      if (rank < cum + cnt) { digit = d; break; }
      cum += cnt;
    }
    if (t == 0) { res->prefA = st.prefA | (digit << shift); res->rankA = rank - cum; }
    else        { res->prefB = st.prefB | (digit << shift); res->rankB = rank - cum; }
  }
  __syncthreads();
  return *res;
}

// pass p in 0..3: digit at shift 24 - 8 p.  hist_prev / st_prev: pass p - 1's (unused at p == 0; at p == 1 the state is {0, rank_j, 0, rank_j1}).
template <class Src>
__global__ void __launch_bounds__(256) k_win_select(Src src, const uint32_t* __restrict__ hist_prev, uint32_t* __restrict__ hist_cur,
                                                    const WinSelState* __restrict__ st_prev, WinSelState* __restrict__ st_cur, int pass,
                                                    uint32_t rank_j, uint32_t rank_j1, int64_t per) {
  __shared__ uint32_t lds[2 * WS_BINS];
  __shared__ WinSelState res;
  const int64_t b = blockIdx.y;
  const int chunk = blockIdx.x, nch = gridDim.x, t = threadIdx.x;
  const int shift = 24 - 8 * pass;
  WinSelState st{0u, rank_j, 0u, rank_j1};
  if (pass > 0) {
    if (pass > 1) st = st_prev[b];
    st = select_fold(hist_prev + b * nch * (2 * WS_BINS), nch, st, shift + 8, lds, &res);
    if (chunk == 0 && t == 0) st_cur[b] = st;
    __syncthreads();
  }
  lds[t] = 0u; lds[WS_BINS + t] = 0u;
  __syncthreads();
  const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);  // the digits already fixed
  const bool same = st.prefA == st.prefB;
  src.prepare(b);
  const int64_t e0 = (int64_t)chunk * WS_CHUNK, e1 = min(per, e0 + (int64_t)WS_CHUNK);
#pragma unroll 4
  for (int64_t e = e0 + t; e < e1; e += 256) {
    const uint32_t key = src.key(b * per + e);
    const uint32_t d = (key >> shift) & (WS_BINS - 1);
    if ((key & mask) == st.prefA) atomicAdd(&lds[d], 1u);
    if (!same && (key & mask) == st.prefB) atomicAdd(&lds[WS_BINS + d], 1u);
  }
  __syncthreads();
  uint32_t* __restrict__ o = hist_cur + (b * nch + chunk) * (2 * WS_BINS);
  o[t] = lds[t]; o[WS_BINS + t] = lds[WS_BINS + t];
}

// frac = h - j of h = (double)q (n - 1).  q_out (nullable): Q per window; tab (nullable): [., s_b, rho_b, .], the whole row with init_m
__global__ void __launch_bounds__(256) k_win_quantile_finish(const uint32_t* __restrict__ hist, const WinSelState* __restrict__ st_prev, int nch,
                                                             double frac, float floor_f, float cap, float* __restrict__ q_out,
                                                             float* __restrict__ tab, int init_m) {
  __shared__ uint32_t lds[2 * WS_BINS];
  __shared__ WinSelState res;
  const int64_t b = blockIdx.x;
  const WinSelState st = select_fold(hist + b * nch * (2 * WS_BINS), nch, st_prev[b], 0, lds, &res);
  if (threadIdx.x == 0) {
    const double aj = (double)__uint_as_float(st.prefA), aj1 = (double)__uint_as_float(st.prefB);  // the two order statistics, bit for bit
    const double d = aj1 - aj, p = d * frac;  // (j == n - 1: both ranks are j, d == 0 and Q == a_j)
    const float Q = (float)(aj + p);
    if (q_out) q_out[b] = Q;
    if (tab) {
      const float s = fminf(fmaxf(Q, floor_f), cap);
      tab[4 * b + 1] = s; tab[4 * b + 2] = floor_f / s;
      if (init_m) { tab[4 * b] = 1.f; tab[4 * b + 3] = 0.f; }
    }
  }
}

int64_t win_chunks(int64_t per) { return (per + WS_CHUNK - 1) / WS_CHUNK; }

template <class Src>
int select_passes(const Src& src, const WinQuantile& qa, int B, int64_t per, const WinStatScratch& S, hipStream_t s) {
  const int nch = S.nch;
  const double h = (double)qa.q * (double)(per - 1);
  const double jf = std::floor(h);
  const uint32_t j = (uint32_t)jf, j1 = (uint32_t)std::min<int64_t>((int64_t)j + 1, per - 1);
  for (int p = 0; p < 4; ++p) {
    hipLaunchKernelGGL(k_win_select<Src>, dim3(nch, B), dim3(256), 0, s, src, (const uint32_t*)S.hist[(p + 1) & 1], S.hist[p & 1],
                       (const WinSelState*)(S.st + (int64_t)(p > 0 ? p - 1 : 0) * B), S.st + (int64_t)p * B, p, j, j1, per);
    DQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_win_quantile_finish, dim3(B), dim3(256), 0, s, (const uint32_t*)S.hist[1], (const WinSelState*)(S.st + 3 * (int64_t)B), nch,
                     h - jf, qa.floor, qa.cap, qa.q_out, qa.tab, qa.init_m ? 1 : 0);
  DQ_LAUNCH_CHECK();
  return 0;
}

template <int PRED>
int select_x0(const WinQuantile& qa, int B, int64_t per, const WinStatScratch& S, hipStream_t s) {
  if (qa.guided) return select_passes(SrcX0<PRED, true>{qa.x, qa.c, qa.u, qa.coef, qa.step_ptr, qa.m_tab, qa.w, 0.f, 0.f, 1.f}, qa, B, per, S, s);
  return select_passes(SrcX0<PRED, false>{qa.x, qa.c, nullptr, qa.coef, qa.step_ptr, nullptr, 1.f, 0.f, 0.f, 1.f}, qa, B, per, S, s);
}

}  // namespace

int64_t win_stat_scratch_bytes(int B, int64_t per) {
  if (B < 1 || per < 1) return -1;
  const int64_t nch = win_chunks(per);
  // the table, the select states of the four passes, the moment partials, two histogram buffers (ping-pong over the passes)
  return (int64_t)B * (16 + 4 * (int64_t)sizeof(WinSelState)) +
         (int64_t)B * nch * ((int64_t)sizeof(double) * WS_MOMENTS + 2 * (int64_t)sizeof(uint32_t) * 2 * WS_BINS);
}

int win_stat_carve(const std::string& who, void* scratch, int64_t scratch_bytes, int B, int64_t per, WinStatScratch* out) {
  DQ_REQUIRE(B >= 1 && B <= 65535 && per >= 1 && per <= (int64_t)INT32_MAX, who + ": need 1 <= B <= 65535 and 1 <= per_window < 2^31");
  DQ_REQUIRE(scratch, who + ": null argument");
  DQ_REQUIRE(scratch_bytes >= win_stat_scratch_bytes(B, per), who + ": statistics scratch too small (dq_sample_stat_scratch_bytes)");
  DQ_REQUIRE(((uintptr_t)scratch & 15) == 0, who + ": the statistics scratch must be 16-byte aligned");
  const int64_t nch = win_chunks(per);
  DQ_REQUIRE(nch <= INT32_MAX / (2 * WS_BINS), who + ": window too large");
  char* p = (char*)scratch;
  out->nch = (int)nch;
  out->tab = (float*)p; p += 16 * (int64_t)B;
  out->st = (WinSelState*)p; p += 4 * (int64_t)sizeof(WinSelState) * B;
  out->part = (double*)p; p += (int64_t)sizeof(double) * WS_MOMENTS * B * nch;
  out->hist[0] = (uint32_t*)p; p += (int64_t)sizeof(uint32_t) * 2 * WS_BINS * B * nch;
  out->hist[1] = (uint32_t*)p;
  return 0;
}

int launch_win_rescale(const float* c, const float* u, float w, double phi, int B, int64_t per, const WinStatScratch& S, float* tab, float s_init,
                       bool init_rest, float* m_out, hipStream_t s) {
  hipLaunchKernelGGL(k_win_moments, dim3(S.nch, B), dim3(256), 0, s, c, u, w, S.part, per);
  DQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_win_rescale_finish, dim3(B), dim3(64), 0, s, (const double*)S.part, tab, m_out, phi, S.nch, per, s_init, init_rest ? 1 : 0);
  DQ_LAUNCH_CHECK();
  return 0;
}

int launch_win_quantile(const WinQuantile& qa, int B, int64_t per, const WinStatScratch& S, hipStream_t s) {
  if (!qa.c) return select_passes(SrcPlain{qa.x}, qa, B, per, S, s);  // |x| itself
  switch (qa.pred) {
    case DQ_PRED_V: return select_x0<DQ_PRED_V>(qa, B, per, S, s);
    case DQ_PRED_X0: return select_x0<DQ_PRED_X0>(qa, B, per, S, s);
    default: return select_x0<DQ_PRED_EPS>(qa, B, per, S, s);
  }
}

}  // namespace dq
