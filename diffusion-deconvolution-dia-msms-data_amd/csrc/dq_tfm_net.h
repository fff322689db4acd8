// The CustomTransformer handle and what its passes share (dq_tfm.hip: the network -- layout, the one forward walk, backward;
// dq_tfm_sample.hip: the sampling loop and held-out evaluation; dq_tfm_api.hip: the stand-alone entries).
// Internal: not installed.
#pragma once
#include "dq_common.h"
#include "dq_tfm.h"
#include "dq_unet.h"  // StepUpdate, StepGraph
#include <string>
#include <vector>

namespace dq {

struct TfmParam { std::string name; int64_t offset; int ndim; int64_t shape[2]; int64_t numel; };
struct TfmLayer { int64_t in_w, in_b, out_w, out_b, n1_g, n1_b, f0_w, f0_b, f2_w, f2_b, n2_g, n2_b; };

// Everything a captured sampling step of the transformer has baked into its kernel arguments or its dispatch (StepKey's counterpart).
// num_steps: the workspace is carved by it (the time table sits in front of the sampler's state), so the baked addresses move with it
struct TfmStepKey {
  const void* params = nullptr; const void* ws = nullptr; const void* rope_sin = nullptr; const void* rope_cos = nullptr;
  int B = 0, S1 = 0, S2 = 0, num_steps = 0, normalize = -1, pred = -1, precision = -1;
  StepUpdate update = StepUpdate::DDIM;
  float clip = 0.f;
  unsigned opt_epoch = 0;
  bool operator==(const TfmStepKey& o) const {
    return params == o.params && ws == o.ws && rope_sin == o.rope_sin && rope_cos == o.rope_cos && B == o.B && S1 == o.S1 && S2 == o.S2 && num_steps == o.num_steps &&
           normalize == o.normalize && pred == o.pred && precision == o.precision && update == o.update && clip == o.clip && opt_epoch == o.opt_epoch;
  }
};

}  // namespace dq

struct dq_tfm {
  int D = 0, H = 0, heads = 0, layers = 0;
  std::vector<dq::TfmParam> params;
  int64_t total = 0;
  int64_t in_w, in_b, out_w, out_b, c_w, c_b, t1_w, t1_b, t2_w, t2_b;
  std::vector<dq::TfmLayer> L;
  // which training workspaces hold a forward's saved activations (one entry per workspace; several forwards may be in flight before
  // their backwards run: micro-batches whose losses are summed).  An entry stays until the same workspace takes another forward.
  struct Saved { const void* ws; int B, S1, S2; };
  std::vector<Saved> saved;
  int precision = dq::GEMM_FP32;  // arithmetic of the dense products (dq_tfm_set_precision)
  dq::StepGraph step;  // the captured sampling step of dq_tfm_sample; valid while step_key holds
  dq::TfmStepKey step_key;
};

namespace dq {

constexpr int64_t TFM_PARTIAL_FLOATS = (int64_t)(768 + 256) * 128 * 128;  // bound of launch_gemm's split-K scratch (k_gemm.hip: choose())
inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// A workspace is carved from `base` in a fixed order, every piece rounded up to 4 floats; a null base only counts (the size queries)
struct Carver {
  float* base;
  int64_t off = 0;  // floats taken so far
  template <class T = float> T* take(int64_t n) {  // n elements of T
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += up4(n * (int64_t)(sizeof(T) / sizeof(float)));
    return r;
  }
};

// the time MLP's buffers over n timesteps: features (n, H), Linear (n, 4H), GELU (n, 4H), Linear (n, H)
struct TimeBufs { float *tfeat, *th, *tg, *temb; };

// workspace of the network: `training` keeps one set of layer buffers per layer (read by the backward)
struct Ws {
  float* cp;
  TimeBufs time;
  float *x0, *tmp, *partial, *colscr, *lnscr;
  struct Layer { float *comb, *q, *kv, *prob, *ao, *y1, *st1, *x1, *hpre, *hact, *y2, *st2, *xo; };
  std::vector<Layer> L;
  // backward only
  float *dxa, *dxb, *dh, *dq, *dkv, *dprob, *dao, *dcomb, *dcp, *dtemb, *dtg;
};
Ws carve(const dq_tfm& p, Carver& c, int B, int S1, int S2, bool training);
// the per-layer K | V buffers (B, Sk, 2H) of a pass that caches the conditional rows (sampling, evaluation)
std::vector<float*> carve_kv(const dq_tfm& p, Carver& c, int B, int Sk);

// y (M, N) = x (M, K) W^T + b   with W an nn.Linear weight (N, K); partial: TFM_PARTIAL_FLOATS floats of split-K scratch
int tfm_linear(const float* x, const float* w, const float* b, float* y, int M, int N, int K, float* partial, hipStream_t s);

struct AttnDims { int B, S1, Sk, H, heads, dh; int64_t ldp; };
// batched (sample, head) products of the attention; `which`: 0 scores = Q K^T, 1 O = P V, 2 dP = dO V^T, 3 dV = P^T dO,
// 4 dQ = dS K, 5 dK = dS^T Q
int attn_gemm(int which, const AttnDims& d, const float* q, const float* kv, float* prob, float* o, float* partial, hipStream_t s);
// the attention of an inference pass by form (TfmAttnForm): one fused launch, or scores GEMM -> softmax rows -> PV GEMM through `prob`
// ((B heads S1) rows of up4(Sk) floats; unused by the fused form)
int tfm_attention_fwd(int form, const AttnDims& d, const float* q, const float* kv, float* prob, float* o, float* partial, hipStream_t s);

// time embedding (building_blocks.py:92-112) of the n timesteps at t: features -> Linear -> GELU -> Linear into b.temb
int tfm_time_mlp(const dq_tfm& p, const float* P, const int64_t* t, const float* time_freqs, const TimeBufs& b, int n, float* partial, hipStream_t s);

// One forward of the network from x_in (B, S1, D) to out (B, S1, D): input projection, RoPE + time, the L layers, output projection.
// Every pass goes through it; they differ in where a layer's K | V rows come from, the attention form and how the time row is named.
struct TfmWalk {
  const dq_tfm* p; const float* P; const float* sin_t; const float* cos_t;
  const Ws* w;  // carved at (B, S1, S2)
  int B, S1, S2;
  bool per_layer = false;  // layer l works in w->L[l] (the saving forward: the backward reads them); else every layer in w->L[0]
  bool ln_stats = false;   // the LayerNorms keep mean | rstd in the layer's st1, st2
  // K | V.  x_cond non-null: "own" -- the conditional embedding of x_cond (B, S2) into w->cp, then per layer [cp ; x] gathered into the
  // layer's comb and one product into its kv.  Null: "cached" -- kv[l] (B, Sk, 2H) holds the conditional rows [0, S2) already
  // (tfm_kv_rows by the caller), the walk fills rows [S2, Sk) from x
  const float* x_cond = nullptr;
  float* const* kv = nullptr;
  int attn_form = TFM_ATTN_GEMM;
  // time: temb (B, H), every sample its own row (launch_rope_add); or a (steps, H) table whose row time_row -- with step_ptr the row the
  // device-side counter names -- every sample adds (launch_rope_add_row)
  const float* temb = nullptr;
  bool time_per_sample = false;
  int time_row = 0; const int* step_ptr = nullptr;
};
int tfm_walk(const TfmWalk& k, const float* x_in, float* out, hipStream_t s);
// K | V rows of `rows` (batch, M, H) under layer l's projection into rows [row0, row0 + M) of kv_l's (Sk-row) first `batch` samples: one
// product batched over the samples (batch == 1: a plain product, which the launcher may split along the reduction)
int tfm_kv_rows(const dq_tfm& p, const float* P, int l, const float* rows, int M, int row0, int batch, float* kv_l, int Sk, float* partial,
                hipStream_t s);

// the handle's precision as the thread's GEMM default for the duration of one call
struct PrecisionScope {
  int old;
  explicit PrecisionScope(int p) : old(set_gemm_precision(p)) {}
  ~PrecisionScope() { set_gemm_precision(old); }
};

}  // namespace dq
