// The update of one sampling step behind the network forward (model.py:265-289; DESIGN.md sections 22, 26, 32, 33): x_prev from x and the
// network output, element-wise.  Three families, each stated once as a policy struct -- its coefficient row, how the row is loaded (with
// step_ptr, graph replay: the row the device-side step counter names), and the arithmetic of one element:
//   Ddim    x0 = (x - sb*eps)/sa ; x_prev = sap*x0 + sbp*eps (t > 0) else x0                                    rows [sa, sb, sap, sbp]
//   Sto     the same plus sigma * z, z drawn in the kernel (dq_philox.h) keyed by (seed, window id, element, draw)  rows [sa, sb, sap, c], sigma
//   Solver  x_prev = cx*x + c0*x0 + c1*x0_hist, x0 optionally clamped (DPM-Solver++(2M); c1 == 0: first order)      rows [sa, sb, cx, c0], c1
// and ONE kernel around them, k_step_update<family, PRED, GUIDED, V>: the grid-stride loop that loads x, the network output (GUIDED:
// its two halves, combined by guide() of dq_guide.h) and the history, and stores x_prev, its mirror, the history and eps.  V = 4: 16 bytes
// per lane and access; V = 1: one element, for counts that are no multiple of 4 and pointers that are not 16-byte aligned.  No LDS, no
// atomics.  Bytes per element: 12 (Ddim, Sto), 20 - 24 (Solver); guided + 8 (the second half read, the mirror written); + 4 with eps_out.
// The fused head-launch form of the Ddim update lives in k_level.hip.
// The per-window form (the trailing parameter pack Win = one `const float*`): a (B, 4) table [m_b, s_b, rho_b, -] of
// k_winstat.hip, row i / perv.  Guided, g <- m_b * g (rescaled guidance); Solver, x0 <- clamp(x0, -s_b, s_b) * rho_b (dynamic thresholding;
// s_b = +inf, rho_b = 1: no clamp).  + 16 bytes per lane-step from the table (L2: a window's lanes read one row).  With an empty pack the
// parameter list, and so every instantiation above, is what it was.
#include "dq_common.h"
#include "dq_guide.h"
#include "dq_kernels.h"
#include "dq_philox.h"
#include "dq_x0.h"
#include "../../include/dq_hip.h"  // DQ_PRED_*
#include <algorithm>
#include <string>

namespace dq {

// What an element may need beside its row: the clamp (Solver); seed, window id and draw index (Sto)
struct UpdateLane { float clip; uint64_t seed; int64_t win; uint32_t draw; float rho = 1.f; };  // rho: the per-window form's rho_b (clip is then s_b)

// ``coef`` is a device table of 4 floats per step [sa, sb, sap, sbp]; sap < 0 marks the t == 0 step.
// PRED (DQ_PRED_*): DQ_PRED_X0 (model.py:274-278): the network output is its x0 prediction, eps = (x_t - sa*x0)/sb is derived.
// DQ_PRED_V: the network output is v = sa*eps - sb*x0; x0 = sa*x_t - sb*v and eps = sb*x_t + sa*v, no division.
struct DdimRow { float sa, sb, sap, sbp; bool last; };

__device__ __forceinline__ DdimRow ddim_row(const float* coef, const int* step_ptr) {
  if (step_ptr) coef += 4 * step_ptr[0];  // graph replay: this step's row of the coefficient table
  return DdimRow{coef[0], coef[1], coef[2], coef[3], coef[2] < 0.f};
}

// One element: x_prev from x and the network output v (or, guided, from g in its place: dq_guide.h); the step's eps by reference
template <int PRED>
__device__ __forceinline__ float ddim_elem(const DdimRow& r, float x, float v, float& ep) {
  float x0;
  if (PRED == DQ_PRED_V)       { x0 = r.sa * x - r.sb * v; ep = r.sb * x + r.sa * v; }
  else if (PRED == DQ_PRED_X0) { x0 = v; ep = (x - r.sa * x0) / r.sb; }
  else                         { ep = v; x0 = (x - r.sb * ep) / r.sa; }
  return r.last ? x0 : r.sap * x0 + r.sbp * ep;
}

// ddim_elem's arithmetic for x0 and eps (every objective), then x_prev = (sap*x0 + c*eps) + sigma*z on a step with t > 0, x0 on the t == 0
// step (sap < 0: no noise drawn, ddim_elem's result bit for bit).  coef: rows [sa, sb, sap, c]; sigma: one float per row.
struct StoRow { float sa, sb, sap, c, sigma; bool last; };

// the step's row; with step_ptr (graph replay) the row AND the draw index 1 + step come from the device step counter
__device__ __forceinline__ StoRow sto_row(const float* coef, const float* sigma_tab, const int* step_ptr, uint32_t& draw) {
  if (step_ptr) { const int st = step_ptr[0]; coef += 4 * st; sigma_tab += st; draw = 1u + (uint32_t)st; }
  return StoRow{coef[0], coef[1], coef[2], coef[3], sigma_tab[0], coef[2] < 0.f};
}

// One element: x_prev from x, the network output v (or, guided, g in its place) and the noise of element e of window w; the step's eps by
// reference.  Guided, the noise of a window is drawn ONCE and the result goes through both stores: the two halves never see different noise.
template <int PRED>
__device__ __forceinline__ float sto_elem(const StoRow& r, float x, float v, uint64_t seed, int64_t w, uint32_t e, uint32_t draw, float& ep) {
  float x0;
  if (PRED == DQ_PRED_V)       { x0 = r.sa * x - r.sb * v; ep = r.sb * x + r.sa * v; }
  else if (PRED == DQ_PRED_X0) { x0 = v; ep = (x - r.sa * x0) / r.sb; }
  else                         { ep = v; x0 = (x - r.sb * ep) / r.sa; }
  float z = 0.f;
  if (!r.last) z = philox_normal(seed, w, e, draw);  // (uniform: the t == 0 step draws nothing)
  return r.last ? x0 : (r.sap * x0 + r.c * ep) + r.sigma * z;
}

// One linear multistep row per step; x0 is the network output (x0 objective), (x - sb * e) / sa (eps objective) or sa*x - sb*v (v objective), optionally clamped to
// [-clip, clip] before it is used and before it becomes the next step's history.  cx < 0 marks the last row: x_prev = x0.
struct SolverRow { float sa, sb, cx, c0, c1; };

__device__ __forceinline__ SolverRow solver_row(const float* coef, const float* c1_tab, const int* step_ptr) {
  if (step_ptr) { const int st = step_ptr[0]; coef += 4 * st; c1_tab += st; }  // graph replay: this step's row
  return SolverRow{coef[0], coef[1], coef[2], coef[3], c1_tab[0]};
}

// One element.  `h` is read by the caller only when c1 != 0.  Returns x_prev; x0 (clamped) and eps by reference.
template <int PRED>
__device__ __forceinline__ float solver_elem(const SolverRow& r, float clip, float x, float v, float h, float& x0, float& ep) {
  if (PRED == DQ_PRED_V)       { x0 = r.sa * x - r.sb * v; ep = r.sb * x + r.sa * v; }
  else if (PRED == DQ_PRED_X0) { x0 = v; }
  else                         { ep = v; x0 = (x - r.sb * ep) / r.sa; }
  bool clamped = false;
  if (clip > 0.f) {
    if (x0 < -clip) { x0 = -clip; clamped = true; }
    else if (x0 > clip) { x0 = clip; clamped = true; }
  }
  if (PRED == DQ_PRED_X0 || clamped) ep = (x - r.sa * x0) / r.sb;  // eps consistent with the x0 that is used
  if (r.cx < 0.f) return x0;
  const float y = r.cx * x + r.c0 * x0;
  return r.c1 != 0.f ? y + r.c1 * h : y;
}

// The per-window form of one element: the same with x0 <- clamp(x0, -s, s) * rho (s > 0; +inf: no clamp) and eps re-derived wherever x0 was
// changed, i.e. where it was clamped or rho != 1.  (s, rho) = (clip, 1) is solver_elem bit for bit: x0 * 1 is exact.
template <int PRED>
__device__ __forceinline__ float solver_elem_win(const SolverRow& r, float s, float rho, float x, float v, float h, float& x0, float& ep) {
  x0 = net_x0<PRED>(r.sa, r.sb, x, v);
  if (PRED == DQ_PRED_V) ep = r.sb * x + r.sa * v;
  else if (PRED == DQ_PRED_EPS) ep = v;
  bool changed = rho != 1.f;
  if (x0 < -s) { x0 = -s; changed = true; }
  else if (x0 > s) { x0 = s; changed = true; }
  x0 = x0 * rho;
  if (PRED == DQ_PRED_X0 || changed) ep = (x - r.sa * x0) / r.sb;  // eps consistent with the x0 that is used
  if (r.cx < 0.f) return x0;
  const float y = r.cx * x + r.c0 * x0;
  return r.c1 != 0.f ? y + r.c1 * h : y;
}

// The families as the kernel sees them.  HIST: the update keeps an x0 history (read when reads_hist(row), written whenever it is given);
// WINDOW: elem needs the window and the element inside it (and the kernel the seed); EPS_IS_NET: under the eps objective the unguided
// step's eps is the network output itself and is not stored again; RESTRICT: the unguided form's tensors never alias.
struct Ddim {
  using Row = DdimRow;
  static constexpr bool HIST = false, WINDOW = false, EPS_IS_NET = true, RESTRICT = true;
  static __device__ __forceinline__ Row row(const float* coef, const float*, const int* step_ptr, uint32_t&) { return ddim_row(coef, step_ptr); }
  template <int PRED>
  static __device__ __forceinline__ float elem(const Row& r, const UpdateLane&, float x, float v, float, uint32_t, float&, float& ep) {
    return ddim_elem<PRED>(r, x, v, ep);
  }
};
struct Sto {
  using Row = StoRow;
  static constexpr bool HIST = false, WINDOW = true, EPS_IS_NET = true, RESTRICT = true;
  static __device__ __forceinline__ Row row(const float* coef, const float* sigma_tab, const int* step_ptr, uint32_t& draw) {
    return sto_row(coef, sigma_tab, step_ptr, draw);
  }
  template <int PRED>
  static __device__ __forceinline__ float elem(const Row& r, const UpdateLane& k, float x, float v, float, uint32_t e, float&, float& ep) {
    return sto_elem<PRED>(r, x, v, k.seed, k.win, e, k.draw, ep);
  }
};
struct Solver {
  using Row = SolverRow;
  static constexpr bool HIST = true, WINDOW = false, EPS_IS_NET = false, RESTRICT = false;
  static __device__ __forceinline__ Row row(const float* coef, const float* c1_tab, const int* step_ptr, uint32_t&) {
    return solver_row(coef, c1_tab, step_ptr);
  }
  static __device__ __forceinline__ bool reads_hist(const Row& r) { return r.c1 != 0.f && r.cx >= 0.f; }  // the first step's history is uninitialised memory
  template <int PRED>
  static __device__ __forceinline__ float elem(const Row& r, const UpdateLane& k, float x, float v, float h, uint32_t, float& x0, float& ep) {
    return solver_elem<PRED>(r, k.clip, x, v, h, x0, ep);
  }
  template <int PRED>
  static __device__ __forceinline__ float elem_win(const Row& r, const UpdateLane& k, float x, float v, float h, uint32_t, float& x0, float& ep) {
    return solver_elem_win<PRED>(r, k.clip, k.rho, x, v, h, x0, ep);
  }
};

// V floats of p at index i (in units of V floats)
template <int V> __device__ __forceinline__ void load_v(const float* p, int64_t i, float (&a)[V]) {
  if constexpr (V == 4) { const float4 t = reinterpret_cast<const float4*>(p)[i]; a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; }
  else a[0] = p[i];
}
template <int V> __device__ __forceinline__ void store_v(float* p, int64_t i, const float (&a)[V]) {
  if constexpr (V == 4) reinterpret_cast<float4*>(p)[i] = make_float4(a[0], a[1], a[2], a[3]);
  else p[i] = a[0];
}

// The tensors of an instantiation: __restrict__ for the unguided Ddim and Sto forms.  Everywhere else the update is element-wise over
// tensors that may alias: x_prev x_t, eps_out the network output (and net_u net_c), the history updated in place.
template <bool R> struct UpdatePtr { using in = const float*; using out = float*; };
template <> struct UpdatePtr<true> { using in = const float* __restrict__; using out = float* __restrict__; };

// nv, perv: the element count and the per-window count in units of V.  The window of lane-step i is i / perv, its first element
// V * (i % perv): a lane's elements never straddle two windows (V == 4 runs only when the per-window count is a multiple of 4).
// Win: empty, or the per-window table (one `const float*`; V == 4 then runs only when the per-window count is a multiple of 4, as for Sto).
__device__ __forceinline__ const float* win_table() { return nullptr; }
__device__ __forceinline__ const float* win_table(const float* t) { return t; }

template <class F, int PRED, bool GUIDED, int V, class... Win>
__global__ void __launch_bounds__(256) k_step_update(typename UpdatePtr<F::RESTRICT && !GUIDED>::in x_t, typename UpdatePtr<F::RESTRICT && !GUIDED>::in net_c,
                                                     typename UpdatePtr<F::RESTRICT && !GUIDED>::in net_u, typename UpdatePtr<F::RESTRICT && !GUIDED>::out x_prev,
                                                     typename UpdatePtr<F::RESTRICT && !GUIDED>::out x_mirror, typename UpdatePtr<F::RESTRICT && !GUIDED>::out hist,
                                                     typename UpdatePtr<F::RESTRICT && !GUIDED>::out eps_out, const float* __restrict__ coef,
                                                     const float* __restrict__ extra, const int64_t* __restrict__ ids, const uint64_t* __restrict__ seed_p,
                                                     uint32_t draw, float clip, float gw, int64_t nv, int64_t perv, const int* __restrict__ step_ptr, Win... win) {
  constexpr bool WIN = sizeof...(Win) != 0;
  const float* __restrict__ tab = win_table(win...);
  const typename F::Row r = F::row(coef, extra, step_ptr, draw);
  UpdateLane k{clip, 0, 0, draw};
  if constexpr (F::WINDOW) k.seed = seed_p[0];
  bool rd_hist = false;  // (uniform)
  if constexpr (F::HIST) rd_hist = hist && F::reads_hist(r);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float xv[V], nv_[V], hv[V], ov[V], zv[V], dv[V];
    load_v<V>(x_t, i, xv);
    load_v<V>(net_c, i, nv_);
    if constexpr (GUIDED) {
      float uv[V];
      load_v<V>(net_u, i, uv);
#pragma unroll
      for (int j = 0; j < V; ++j) nv_[j] = guide(nv_[j], uv[j], gw);
    }
    if constexpr (WIN) {
      const float* __restrict__ t = tab + 4 * (i / perv);  // this window's [m, s, rho, -]
      if constexpr (GUIDED) {
        const float m = t[0];
#pragma unroll
        for (int j = 0; j < V; ++j) nv_[j] = m * nv_[j];
      }
      if constexpr (F::HIST) { k.clip = t[1]; k.rho = t[2]; }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) hv[j] = 0.f;
    if constexpr (F::HIST) { if (rd_hist) load_v<V>(hist, i, hv); }
    uint32_t e0 = 0;
    if constexpr (F::WINDOW) {
      const int64_t b = i / perv;
      e0 = (uint32_t)(i - b * perv) * (uint32_t)V;
      k.win = ids ? ids[b] : b;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if constexpr (WIN && F::HIST) ov[j] = F::template elem_win<PRED>(r, k, xv[j], nv_[j], hv[j], e0 + (uint32_t)j, zv[j], dv[j]);
      else ov[j] = F::template elem<PRED>(r, k, xv[j], nv_[j], hv[j], e0 + (uint32_t)j, zv[j], dv[j]);
    }
    store_v<V>(x_prev, i, ov);
    if constexpr (GUIDED) { if (x_mirror) store_v<V>(x_mirror, i, ov); }
    if constexpr (F::HIST) { if (hist) store_v<V>(hist, i, zv); }
    if constexpr (PRED != DQ_PRED_EPS || GUIDED || !F::EPS_IS_NET) { if (eps_out) store_v<V>(eps_out, i, dv); }
  }
}

template <class F, bool GUIDED, int V, class... Win>
static int launch_update_as(const StepUpdateLaunch& a, int64_t nv, hipStream_t s, Win... win) {
  const int grid = (int)std::min<int64_t>(cdiv(nv, 256), 2048);
  const auto kernel = a.pred == DQ_PRED_V    ? k_step_update<F, DQ_PRED_V, GUIDED, V, Win...>
                      : a.pred == DQ_PRED_X0 ? k_step_update<F, DQ_PRED_X0, GUIDED, V, Win...>
                                             : k_step_update<F, DQ_PRED_EPS, GUIDED, V, Win...>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, a.x_t, a.net, a.net_u, a.x_prev, a.x_mirror, a.hist, a.eps_out, a.coef, a.extra, a.ids,
                     a.seed, (uint32_t)a.draw, a.clip > 0.f ? a.clip : 0.f /* (NaN and negatives: off) */, a.w, nv, a.per / V, a.step_ptr, win...);
  DQ_LAUNCH_CHECK();
  return 0;
}

template <class F>
static int launch_update_of(const StepUpdateLaunch& a, bool vec, int64_t n, hipStream_t s) {
  if (a.win) {  // the per-window form: guided (reads m_b), or the Solver family (reads s_b, rho_b); anything else was refused
    if (a.guided) return vec ? launch_update_as<F, true, 4>(a, n / 4, s, a.win) : launch_update_as<F, true, 1>(a, n, s, a.win);
    if constexpr (F::HIST) return vec ? launch_update_as<F, false, 4>(a, n / 4, s, a.win) : launch_update_as<F, false, 1>(a, n, s, a.win);
  }
  if (a.guided) return vec ? launch_update_as<F, true, 4>(a, n / 4, s) : launch_update_as<F, true, 1>(a, n, s);
  return vec ? launch_update_as<F, false, 4>(a, n / 4, s) : launch_update_as<F, false, 1>(a, n, s);
}

int launch_update(const StepUpdateLaunch& a, hipStream_t s) {
  const bool sto = a.family == UpdateFamily::STOCHASTIC, solver = a.family == UpdateFamily::SOLVER;
  const std::string who = std::string(sto ? "ddim_step_sto" : solver ? "solver_step" : "ddim_step") + (a.guided ? "_guided" : "");
  if (sto || solver || a.guided)  // (the unguided DDIM entries make their own)
    DQ_REQUIRE(a.x_t && a.net && (a.net_u || !a.guided) && a.x_prev && a.coef && (a.extra || !(sto || solver)) && (a.seed || !sto),
               who + ": null argument");
  if (!sto) DQ_REQUIRE(a.B >= 0 && a.per >= 0, who + ": negative element count");
  else if (a.guided) DQ_REQUIRE(a.B >= 0 && a.per >= 0 && a.per <= (int64_t)0xffffffff, who + ": need B >= 0 and 0 <= per_window < 2^32");
  else DQ_REQUIRE(a.B >= 0 && a.per >= 0 && a.per % 4 == 0 && a.per <= (int64_t)0xffffffff,
                  who + ": need B >= 0 and a per-window element count that is a multiple of 4 below 2^32");
  if (sto) DQ_REQUIRE(a.draw >= 0, who + ": the draw index must be >= 0");
  DQ_REQUIRE(!a.win || a.guided || solver, who + ": the per-window table needs a guided or a Solver update");
  const uintptr_t bits = (uintptr_t)a.x_t | (uintptr_t)a.net | (uintptr_t)a.net_u | (uintptr_t)a.x_prev | (uintptr_t)a.x_mirror | (uintptr_t)a.hist |
                         (uintptr_t)a.eps_out | ((uintptr_t)a.win & 3);
  if (sto && !a.guided) DQ_REQUIRE((bits & 15) == 0, who + ": tensors must be 16-byte aligned");
  else DQ_REQUIRE((bits & 3) == 0, who + ": tensors must be 4-byte aligned");
  const int64_t n = (int64_t)a.B * a.per;
  if (n == 0) return 0;
  // 16 bytes per lane iff no lane's four elements straddle two windows (Sto, the per-window form) or the end (the others) and every tensor is 16-byte aligned
  const bool vec = (sto || a.win ? a.per : n) % 4 == 0 && (bits & 15) == 0;
  switch (a.family) {
    case UpdateFamily::DDIM: return launch_update_of<Ddim>(a, vec, n, s);
    case UpdateFamily::STOCHASTIC: return launch_update_of<Sto>(a, vec, n, s);
    case UpdateFamily::SOLVER: return launch_update_of<Solver>(a, vec, n, s);
  }
  return 0;
}

__global__ void k_inc_step(int* p) { p[0] += 1; }

int launch_inc_step(int* p, hipStream_t s) {
  hipLaunchKernelGGL(k_inc_step, dim3(1), dim3(1), 0, s, p);
  DQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace dq
